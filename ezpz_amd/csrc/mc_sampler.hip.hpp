// The keyed sampler of the Monte-Carlo entries (include/ezpz_amd.h: THE DRAW): Philox4x32-10 and the draw of one
// dimension for one sample -- one __host__ __device__ body behind ezpz_mc_sample, the Monte-Carlo sampler kernel
// (tolerance_mc.hip.hpp) and the start kernel of the solution branches (branches.hip.hpp).
//
// Built without contraction (build.py: -ffp-contract=off for every unit): no product below becomes an fma, on either side.  Only
// log, cos and sqrt can differ between the host and the device build.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ezpz_amd.h"

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

// A distribution as the sampler reads it: EzpzMcDist with the rank among the CORNER dimensions in place of `reserved`, and the
// nominal value beside it.
struct Dist {
    uint32_t kind, rank;
    double a, b, nominal;
};

// The value of dimension j (distribution d) for sample b: depends on (seed, b, j) alone.
EZPZ_MC_HD double draw(uint64_t seed, uint64_t b, uint32_t j, const Dist& d) {
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

}  // namespace mc
}  // namespace ezpz
