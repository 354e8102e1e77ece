// Monte-Carlo main effects (include/ezpz_amd.h: ezpz_mc_effects[_device], ezpz_mc_effect_indices, ezpz_system_tolerance_mc_effects[_device];
// DESIGN.md 3q): the closing step -- ONE __host__ __device__ body behind the host entry (one caller) and mc_effects_close_kernel (the
// threads of one workgroup) -- the host form of the reduction (plain C++: no device), and the kernels: mc_effects_kernel (a round's
// blocks of the cells' sums and counts, folded into the running ones) and mc_effects_close_kernel.  The process-wide plan and the
// entries of the reduction are in mc_effects.hip; the run is in tolerance_mc.hip, on its plan.
//
// Built without contraction (build.py: -ffp-contract=off for every unit); the closing step is + - * /, comparisons and
// integer-to-double conversions alone, every output element computed by one caller with ascending loops: the same bits on both sides.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ezpz_amd.h"
#include "mc_block_sum.hip.hpp"  // (a host-only user, EZPZ_MCE_HOST_ONLY, takes the closing step and the host reduction alone: tools/asan_effects.cpp)

namespace ezpz {
namespace mce {

#define EZPZ_MCE_HD __host__ __device__ inline

constexpr uint32_t kMaxDim = 32;  // k and m
constexpr uint32_t kMaxBins = EZPZ_MC_EFFECT_MAX_BINS;
constexpr uint32_t kMaxCells = EZPZ_MC_EFFECT_MAX_CELLS;
using mcb::kBlock;  // samples per block of the sums

// Cell (j, c, i) -- dimension, bin, record -- is number e = (j * B + c) * m + i: sums [k][B][m][2], counts [k][B][m].
EZPZ_MCE_HD uint32_t cell_at(uint32_t B, uint32_t m, uint32_t j, uint32_t c, uint32_t i) { return (j * B + c) * m + i; }

EZPZ_MCE_HD double quiet_nan() {
#ifdef __HIP_DEVICE_COMPILE__
    return __longlong_as_double(0x7FF8000000000000ll);
#else
    const uint64_t bits = 0x7FF8000000000000ull;
    double v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
#endif
}

// the bin of a drawn value: how many of the dimension's B - 1 edges are <= p (comparisons alone: a NaN counts nothing)
EZPZ_MCE_HD uint32_t bin_of(const double* edges, uint32_t n_edges, double p) {
    uint32_t bin = 0;
    for (uint32_t e = 0; e < n_edges; ++e) bin += edges[e] <= p ? 1u : 0u;
    return bin;
}

// ---- the closing step ------------------------------------------------------------------------------------------------------------
// Elements are dealt out by the caller's id: first the k B m cells (cond_mean, cond_var), then the m k pairs (eta2, first,
// bins_used); every caller of a pair walks the pair's B cells itself, so an element's value never depends on who computed it.
template <class Team>
EZPZ_MCE_HD void indices(const Team team, const double* sums, const uint64_t* counts, const double* nominal_m, uint32_t k, uint32_t m,
                         uint32_t B, double* cond_mean, double* cond_var, double* eta2, double* first, uint32_t* bins_used) {
    const uint32_t cells = k * B * m;
    for (uint32_t e = team.id(); e < cells + m * k; e += team.count()) {
        if (e < cells) {
            const uint32_t i = e % m;
            const uint64_t n = counts[e];
            const double s = sums[2 * (size_t)e], q = sums[2 * (size_t)e + 1];
            cond_mean[e] = n ? nominal_m[i] + s / (double)n : quiet_nan();
            cond_var[e] = n < 2 ? quiet_nan() : (q - s * s / (double)n) / (double)(n - 1);
            continue;
        }
        const uint32_t pair = e - cells, i = pair / k, j = pair - i * k;
        uint64_t N = 0;
        uint32_t used = 0;
        double S = 0.0, Q = 0.0;
        for (uint32_t c = 0; c < B; ++c) {
            const uint32_t at = cell_at(B, m, j, c, i);
            if (!counts[at]) continue;
            N += counts[at];
            S = S + sums[2 * (size_t)at];
            Q = Q + sums[2 * (size_t)at + 1];
            ++used;
        }
        bins_used[pair] = used;
        if (used < 2) {
            eta2[pair] = first[pair] = 0.0;
            continue;
        }
        const double n = (double)N;
        const double dbar = S / n;
        const double SST = Q - S * S / n;
        double SSB = 0.0, SSW = 0.0;
        for (uint32_t c = 0; c < B; ++c) {
            const uint32_t at = cell_at(B, m, j, c, i);
            if (!counts[at]) continue;
            const double nc = (double)counts[at], s = sums[2 * (size_t)at], q = sums[2 * (size_t)at + 1];
            const double mu = s / nc;
            const double t = mu - dbar;
            SSB = SSB + nc * (t * t);
            const double w = q - s * s / nc;
            SSW = SSW + w;
        }
        if (!(SST > 0.0) || N - used < 1) {
            eta2[pair] = first[pair] = quiet_nan();
            continue;
        }
        eta2[pair] = SSB / SST;
        first[pair] = (SSB - (double)(used - 1) * (SSW / (double)(N - used))) / SST;
    }
}

// ---- the argument checks shared by every entry -------------------------------------------------------------------------------------
inline int check_shape(size_t n_param, size_t n_meas, uint32_t bins) {
    if (n_param == 0 || n_meas == 0 || n_param > kMaxDim || n_meas > kMaxDim || bins < 2 || bins > kMaxBins) return EZPZ_ERR_INVALID_ARGUMENT;
    return n_param * bins * n_meas > kMaxCells ? EZPZ_ERR_INVALID_ARGUMENT : EZPZ_OK;
}

// edges [k][B - 1] in host memory: no NaN, non-decreasing per dimension (+-inf may stand)
inline int check_edges(const double* edges, size_t n_param, uint32_t bins) {
    for (size_t j = 0; j < n_param; ++j)
        for (uint32_t e = 0; e + 1 < bins; ++e) {
            const double v = edges[j * (bins - 1) + e];
            if (v != v || (e && v < edges[j * (bins - 1) + e - 1])) return EZPZ_ERR_INVALID_ARGUMENT;
        }
    return EZPZ_OK;
}

inline void default_config(EzpzMcEffectConfig* ec) {
    ec->bins = 8;
    ec->reserved = 0;
}

// ---- the host entries, whole: ezpz_mc_effect_indices and ezpz_mc_effects forward to them (tools/asan_effects.cpp drives them) --------
inline int indices_host(const double* sums, const uint64_t* counts, const double* nominal_m, size_t n_param, size_t n_meas, uint32_t bins,
                        double* cond_mean, double* cond_var, double* eta2, double* first, uint32_t* bins_used) {
    if (int rc = check_shape(n_param, n_meas, bins)) return rc;
    if (!sums || !counts || !nominal_m || !cond_mean || !cond_var || !eta2 || !first || !bins_used) return EZPZ_ERR_INVALID_ARGUMENT;
    indices(mcb::OneCaller{}, sums, counts, nominal_m, (uint32_t)n_param, (uint32_t)n_meas, bins, cond_mean, cond_var, eta2, first, bins_used);
    return EZPZ_OK;
}

inline int effects_host(const double* params, const double* m_in, const uint8_t* flags, const uint8_t* ok, const double* nominal_m,
                        const double* edges, uint64_t samples, size_t n_param, size_t n_meas, uint32_t bins, double* sums, uint64_t* counts) {
    if (int rc = check_shape(n_param, n_meas, bins)) return rc;
    if (samples && (!params || !m_in || !nominal_m || !edges || !sums || !counts)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (edges)
        if (int rc = check_edges(edges, n_param, bins)) return rc;
    if (samples == 0) return EZPZ_OK;
    const uint32_t k = (uint32_t)n_param, m = (uint32_t)n_meas, B = bins, cells = k * B * m;
    for (uint32_t e = 0; e < cells; ++e) sums[2 * e] = sums[2 * e + 1] = 0.0, counts[e] = 0;
    std::vector<uint32_t> bad(kBlock);
    std::vector<uint8_t> bin((size_t)kBlock * k);
    std::vector<double> d((size_t)kBlock * m), leaves(2 * kBlock);
    for (uint64_t first = 0; first < samples; first += kBlock) {
        for (uint32_t t = 0; t < kBlock; ++t) {
            const uint64_t b = first + t;
            bad[t] = 0xFFFFFFFFu;
            if (b >= samples) continue;
            bad[t] = ok && !ok[b] ? 0xFFFFFFFFu : 0u;
            for (uint32_t i = 0; i < m; ++i) {
                const double v = m_in[b * m + i];
                if ((flags && (flags[b * m + i] & 1u)) || !std::isfinite(v)) bad[t] |= 1u << i;
                d[(size_t)t * m + i] = v - nominal_m[i];
            }
            for (uint32_t j = 0; j < k; ++j) bin[(size_t)t * k + j] = (uint8_t)bin_of(edges + (size_t)j * (B - 1), B - 1, params[b * k + j]);
        }
        for (uint32_t j = 0; j < k; ++j)
            for (uint32_t c = 0; c < B; ++c)
                for (uint32_t i = 0; i < m; ++i) {
                    uint64_t n = 0;
                    for (uint32_t t = 0; t < kBlock; ++t) {
                        const bool hit = !((bad[t] >> i) & 1u) && bin[(size_t)t * k + j] == c;
                        const double v = hit ? d[(size_t)t * m + i] : 0.0;
                        leaves[t] = v;
                        leaves[kBlock + t] = hit ? v * v : 0.0;
                        n += hit;
                    }
                    const uint32_t at = cell_at(B, m, j, c, i);
                    sums[2 * at] = sums[2 * at] + mcb::pair_tree_256(leaves.data());
                    sums[2 * at + 1] = sums[2 * at + 1] + mcb::pair_tree_256(leaves.data() + kBlock);
                    counts[at] += n;
                }
    }
    return EZPZ_OK;
}

#if defined(__HIPCC__) && !defined(EZPZ_MCE_HOST_ONLY)

// ---- the kernels' arguments (filled by the host side: mc_effects.hip and the run of tolerance_mc.hip) ------------------------------
struct EffectArgs {  // mc_effects_kernel: one round
    const double* params;  // [count][k]
    const double* m;       // [count][n_meas]
    const uint8_t* flags;  // [count][n_meas] (NULL: every bit clear)
    const uint8_t* ok;     // [count] (NULL: every one set)
    const double* nominal_m;  // [n_meas]
    const double* edges;      // [k][bins - 1]
    uint64_t count;
    uint32_t k, n_meas, bins, first_round;
    double* part;          // [blocks][cells][2]
    uint32_t* part_n;      // [blocks][cells]
    unsigned int* ticket;  // 0 between launches
    double* sums;
    uint64_t* counts;
};

struct CloseArgs {  // mc_effects_close_kernel: the closing step's, on the sums and counts where the last round left them
    const double* sums;
    const uint64_t* counts;
    const double* nominal_m;
    uint32_t k, m, bins;
    double *cond_mean, *cond_var, *eta2, *first;
    uint32_t* bins_used;
};

#ifdef EZPZ_MCE_KERNELS  // (mc_effects.hip alone: the kernels have one home; the run of tolerance_mc.hip takes the host side below)
__global__ __launch_bounds__(256) void mc_effects_close_kernel(CloseArgs a) {
    indices(mcb::WorkgroupCallers{}, a.sums, a.counts, a.nominal_m, a.k, a.m, a.bins, a.cond_mean, a.cond_var, a.eta2, a.first, a.bins_used);
}

// ---- a round's cells ---------------------------------------------------------------------------------------------------------------
// Workgroup q of a round takes the samples [256 q, 256 q + 256) of the round, which starts at a multiple of 256: the blocks of the
// interface whatever the round.  The block is staged in LDS once -- the deviations d [256][m] (one rounded subtraction each), the
// bins [256][k] as bytes (B <= 64) and a validity word per sample, bit i set when the sample does not count for record i -- and then
// CELLS ACROSS LANES: a lane owns the cells e = t, t + 256, .. (mce::cell_at: i fastest, so the lanes of a wavefront read
// consecutive doubles of a sample's row of d and share its bin byte) and walks the 256 samples, a leaf being d or d * d where the
// sample counts for the record and lies in the cell's bin and +0.0 where not: eight leaves by the explicit adjacent-pair tree, the
// eights through a five-deep binary counter, which is that tree.  The count is the lane's own integer.  One partial per block and
// cell; the workgroup that draws the last ticket folds the round's partials, left to right, into the caller's sums and counts (the
// first round starts them), threads over cells.  No floating-point atomics; nothing in LDS is read before it is written.
struct Pair {
    double a, b;
};
__device__ inline Pair operator+(const Pair& x, const Pair& y) { return Pair{x.a + y.a, x.b + y.b}; }

struct Cell {
    const double* d;       // the record's column of the staged deviations
    const uint8_t* bin;    // the dimension's column of the staged bins
    const uint32_t* bad;   // the validity words
    uint32_t m, k, c, bit;
    uint32_t n;            // the samples counted so far
    __device__ inline Pair operator()(uint32_t s) {
        const bool hit = bin[s * k] == c && !(bad[s] & bit);
        const double v = d[s * m];
        n += hit ? 1u : 0u;
        return Pair{hit ? v : 0.0, hit ? v * v : 0.0};
    }
};

inline size_t effects_lds_bytes(uint32_t k, uint32_t m) { return (size_t)kBlock * m * sizeof(double) + (size_t)kBlock * k; }

__global__ __launch_bounds__(256) void mc_effects_kernel(EffectArgs a) {
    extern __shared__ double s_stage[];  // d [256][m] | bins [256][k] bytes
    __shared__ uint32_t s_bad[kBlock];
    const uint32_t t = threadIdx.x, q = blockIdx.x, k = a.k, m = a.n_meas, B = a.bins, cells = k * B * m;
    double* s_d = s_stage;
    uint8_t* s_bin = reinterpret_cast<uint8_t*>(s_d + (size_t)kBlock * m);
    const uint64_t base = (uint64_t)q * kBlock;  // the block's first sample, in the round
    const uint32_t in_block = (uint32_t)(a.count - base < kBlock ? a.count - base : kBlock);
    s_bad[t] = t < in_block && (!a.ok || a.ok[base + t]) ? 0u : 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t idx = t; idx < kBlock * m; idx += 256) {
        const uint32_t s = idx / m, i = idx - s * m;
        double d = 0.0;
        if (s < in_block) {
            const uint64_t at = (base + s) * m + i;
            const double v = a.m[at];
            if ((a.flags && (a.flags[at] & 1u)) || !isfinite(v)) atomicOr(&s_bad[s], 1u << i);
            d = v - a.nominal_m[i];
        }
        s_d[idx] = d;
    }
    for (uint32_t idx = t; idx < kBlock * k; idx += 256) {
        const uint32_t s = idx / k, j = idx - s * k;
        s_bin[idx] = s < in_block ? (uint8_t)bin_of(a.edges + (size_t)j * (B - 1), B - 1, a.params[(base + s) * k + j]) : (uint8_t)0;
    }
    __syncthreads();
    double* part = a.part + (uint64_t)q * cells * 2;
    uint32_t* part_n = a.part_n + (uint64_t)q * cells;
    for (uint32_t e = t; e < cells; e += 256) {
        const uint32_t j = e / (B * m), rest = e - j * (B * m), c = rest / m, i = rest - c * m;
        Cell u{s_d + i, s_bin + j, s_bad, m, k, c, 1u << i, 0};
        const Pair v = mcb::tree_sum<Pair>(u, 0, kBlock / 8);
        part[2 * e] = v.a, part[2 * e + 1] = v.b;
        part_n[e] = u.n;
    }
    if (!mcb::last_block(a.ticket)) return;
    const uint32_t blocks = gridDim.x;
    mcb::fold_partials(a.part, 2 * cells, a.first_round, a.sums);
    for (uint32_t e = t; e < cells; e += 256) {
        uint64_t n = a.first_round ? 0 : a.counts[e];
#pragma unroll 8
        for (uint32_t b = 0; b < blocks; ++b) n += a.part_n[(uint64_t)b * cells + e];
        a.counts[e] = n;
    }
    if (t == 0) *a.ticket = 0;
}

#endif  // EZPZ_MCE_KERNELS

// ---- the host side (mc_effects.hip), shared with the run of tolerance_mc.hip -------------------------------------------------------
// one round: `a` with the samples' arrays, the edges, count, k, n_meas, bins, first_round, sums and counts set; the workspace holds
// blocks * cells * 2 partials and blocks * cells counts
int enqueue_effects(mcb::Work& work, EffectArgs a, hipStream_t stream);
int enqueue_close(const CloseArgs& a, hipStream_t stream);

#endif  // __HIPCC__ && !EZPZ_MCE_HOST_ONLY

}  // namespace mce
}  // namespace ezpz
