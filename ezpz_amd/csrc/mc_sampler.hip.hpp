// The keyed sampler of the Monte-Carlo entries (include/ezpz_amd.h: THE DRAW): Philox4x32-10 and the draw of one
// dimension for one sample -- one __host__ __device__ body behind ezpz_mc_sample, the Monte-Carlo sampler kernel
// (tolerance_mc.hip.hpp) and the start kernel of the solution branches (branches.hip.hpp) -- and, host only, the check of a list
// of distributions and the body of ezpz_mc_sample.  A flagged dimension's draw (EZPZ_MC_SEQUENCE) is built from mc_sequence.hip.hpp.
//
// Built without contraction (build.py: -ffp-contract=off for every unit): no product below becomes an fma, on either side.  Only
// log, cos and sqrt can differ between the host and the device build.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ezpz_amd.h"
#include "mc_sequence.hip.hpp"

namespace ezpz {
namespace mc {

#define EZPZ_MC_HD __host__ __device__ inline

struct Words {
    uint32_t w[4];
};

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
EZPZ_MC_HD Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

EZPZ_MC_HD Words words_of(uint64_t seed, uint64_t b, uint32_t j, uint32_t attempt) {
    return philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), j, attempt, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// 53 bits of two words as an integer-valued double (exact), then u = k * 2^-53 in [0, 1) and u1 = (k + 1) * 2^-53 in (0, 1]
EZPZ_MC_HD double bits53(uint32_t hi, uint32_t lo) { return (double)(hi >> 5) * 67108864.0 + (double)(lo >> 6); }
constexpr double kTwoM53 = 1.1102230246251565404236316680908203125e-16;  // 2^-53
constexpr double kTwoPi = 6.283185307179586476925286766559;              // the double nearest 2 pi

EZPZ_MC_HD double uniform_of(const Words& w) { return bits53(w.w[0], w.w[1]) * kTwoM53; }
EZPZ_MC_HD double normal_of(const Words& w) {
    const double u1 = (bits53(w.w[0], w.w[1]) + 1.0) * kTwoM53, u2 = bits53(w.w[2], w.w[3]) * kTwoM53;
    const double angle = kTwoPi * u2;
    return sqrt(-2.0 * log(u1)) * cos(angle);
}

constexpr uint32_t kMaxAttempts = 16;
constexpr uint32_t kMaxCorners = 20;

// A distribution as the sampler reads it: EzpzMcDist with the rank among the CORNER dimensions in place of `reserved`, the nominal
// value beside it, and for a flagged dimension (EZPZ_MC_SEQUENCE) the flag and the ends of the truncated probability range.
struct Dist {
    uint32_t kind, rank;
    double a, b, nominal;
    double p_lo, p_hi;  // flagged NORMAL with a truncation T: Phi(-T) and 1 - Phi(-T), computed once on the host
    uint32_t sequence, pad;
};

// The plain draw: Philox words per (seed, b, j) and attempt.
EZPZ_MC_HD double draw_plain(uint64_t seed, uint64_t b, uint32_t j, const Dist& d) {
    switch (d.kind) {
        case EZPZ_MC_UNIFORM:
            return d.nominal + (d.a + (d.b - d.a) * uniform_of(words_of(seed, b, j, 0)));
        case EZPZ_MC_NORMAL: {
            double z = 0.0;
            bool taken = false;
            for (uint32_t t = 0; t < kMaxAttempts && !taken; ++t) {
                z = normal_of(words_of(seed, b, j, t));
                taken = d.b == 0.0 || fabs(z) <= d.b;
            }
            if (!taken) z = copysign(d.b, z);
            return d.nominal + d.a * z;
        }
        case EZPZ_MC_CORNER:
            return d.nominal + (((b >> d.rank) & 1u) ? d.b : d.a);
        default:
            return d.nominal;
    }
}

// The flagged draw (UNIFORM or NORMAL) from the shifted point k = x(b) ^ shift: no loop, no rejection.
EZPZ_MC_HD uint32_t sequence_shift(uint64_t seed, uint32_t j) { return words_of(seed, 0, j, kShiftAttempt).w[0]; }
EZPZ_MC_HD double sequence_value(uint32_t k, const Dist& d) {
    const double u = sequence_unit(k);
    if (d.kind == EZPZ_MC_UNIFORM) return d.nominal + (d.a + (d.b - d.a) * u);
    double z;
    if (d.b == 0.0) {
        z = normal_inverse(u);
    } else {
        z = normal_inverse(d.p_lo + (d.p_hi - d.p_lo) * u);
        z = z < -d.b ? -d.b : z > d.b ? d.b : z;
    }
    return d.nominal + d.a * z;
}

// The value of dimension j (distribution d) for sample b: depends on (seed, b, j) alone.  (A flagged dimension has j < 64 and
// b < 2^32: check_dists has seen to both.)
EZPZ_MC_HD double draw(uint64_t seed, uint64_t b, uint32_t j, const Dist& d) {
    if (d.sequence) return sequence_value(sequence_point(sequence_row(j), (uint32_t)b) ^ sequence_shift(seed, j), d);
    return draw_plain(seed, b, j, d);
}

// ---- the host side: the check of a list and ezpz_mc_sample's body ----------------------------------------------------------------
inline bool sequenced(const EzpzMcDist& d) {
    return (d.reserved & EZPZ_MC_SEQUENCE) && (d.kind == EZPZ_MC_UNIFORM || d.kind == EZPZ_MC_NORMAL);
}

// `d` (checked) as the sampler reads it
inline Dist dist_of(const EzpzMcDist& d, uint32_t rank, double nominal) {
    Dist out{d.kind, rank, d.a, d.b, nominal, 0.0, 1.0, sequenced(d) ? 1u : 0u, 0u};
    if (out.sequence && d.kind == EZPZ_MC_NORMAL && d.b != 0.0) {
        out.p_lo = 0.5 * std::erfc(d.b / std::sqrt(2.0));
        out.p_hi = 1.0 - out.p_lo;
    }
    return out;
}

// The argument errors of the distributions, and the sampler's table.  `first` and `count`: the samples that will be drawn (a
// flagged dimension has 2^32 of them).
inline int check_dists(const EzpzMcDist* dist, const double* nominal, size_t n_param, uint64_t first, uint64_t count, std::vector<Dist>& out) {
    out.clear();
    if (n_param == 0) return EZPZ_OK;
    if (!dist || !nominal || n_param > 0xFFFFFFFEull) return EZPZ_ERR_INVALID_ARGUMENT;
    constexpr uint64_t kGrid = 1ull << 32;
    const bool past_grid = count > kGrid || first > kGrid - count;
    out.resize(n_param);
    uint32_t corners = 0;
    for (size_t j = 0; j < n_param; ++j) {
        const EzpzMcDist& d = dist[j];
        if (d.kind > EZPZ_MC_CORNER || !std::isfinite(d.a) || !std::isfinite(d.b) || !std::isfinite(nominal[j]))
            return EZPZ_ERR_INVALID_ARGUMENT;
        if (d.kind == EZPZ_MC_UNIFORM && d.a > d.b) return EZPZ_ERR_INVALID_ARGUMENT;
        if (d.kind == EZPZ_MC_NORMAL && (d.a < 0.0 || d.b < 0.0 || (d.b > 0.0 && d.b < 1.0))) return EZPZ_ERR_INVALID_ARGUMENT;
        if (sequenced(d) && (j >= kSequenceDims || past_grid)) return EZPZ_ERR_INVALID_ARGUMENT;
        uint32_t rank = 0;
        if (d.kind == EZPZ_MC_CORNER) {
            if (corners == kMaxCorners) return EZPZ_ERR_INVALID_ARGUMENT;
            rank = corners++;
        }
        out[j] = dist_of(d, rank, nominal[j]);
    }
    return EZPZ_OK;
}

inline int sample_host(uint64_t seed, const EzpzMcDist* dist, const double* nominal, size_t n_param, uint64_t first, size_t count,
                       double* params_out) {
    std::vector<Dist> dists;
    if (int rc = check_dists(dist, nominal, n_param, first, count, dists)) return rc;
    if (count && n_param && !params_out) return EZPZ_ERR_INVALID_ARGUMENT;
    for (size_t s = 0; s < count; ++s)
        for (size_t j = 0; j < n_param; ++j) params_out[s * n_param + j] = draw(seed, first + s, (uint32_t)j, dists[j]);
    return EZPZ_OK;
}

}  // namespace mc
}  // namespace ezpz
