// Tolerance contributors (include/ezpz_amd.h: ezpz_mc_moments[_device], ezpz_mc_contributors, ezpz_system_tolerance_mc_contrib[_device];
// DESIGN.md 3n): the closing step -- ONE __host__ __device__ body behind the host entry (one caller) and mc_contrib_kernel (the
// threads of one workgroup) -- and the two kernels: mc_moments_kernel (a round's blocks of the second-moment sums, folded into the
// running moments) and mc_contrib_kernel.  The host plan and the entries are in mc_moments.hip; the run shares tolerance_mc.hip's.
//
// Built without contraction (build.py: -ffp-contract=off for every unit); the closing step is + - * / and comparisons alone, every
// output element computed by one caller with ascending loops: the same bits on both sides.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/ezpz_amd.h"
#include "mc_block_sum.hip.hpp"  // (a host-only user, EZPZ_MCM_HOST_ONLY, takes the closing step alone: tools/asan_contrib.cpp)

namespace ezpz {
namespace mcm {

#define EZPZ_MCM_HD __host__ __device__ inline

constexpr uint32_t kMaxK = EZPZ_MC_MOMENT_MAX;
constexpr uint32_t kMaxEntries = kMaxK + kMaxK * (kMaxK + 1) / 2;  // 2144

EZPZ_MCM_HD uint32_t entries_of(uint32_t K) { return K + K * (K + 1) / 2; }
// the place of G[a][b], a <= b, in `moments`: behind the K sums, the upper triangle row-major
EZPZ_MCM_HD uint32_t g_at(uint32_t K, uint32_t a, uint32_t b) { return K + a * K - a * (a - 1) / 2 + (b - a); }

EZPZ_MCM_HD double quiet_nan() {
#ifdef __HIP_DEVICE_COMPILE__
    return __longlong_as_double(0x7FF8000000000000ll);
#else
    const uint64_t bits = 0x7FF8000000000000ull;
    double v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
#endif
}

// ---- the closing step ------------------------------------------------------------------------------------------------------------
// cov [K][K], beta and contrib [m][k], r2 [m], dropped [1]: the outputs.  L [k][k] (the unit lower factor, its strict lower part
// used), d [k] (the pivots; 0 for a dropped dimension) and kept [k]: the workspace, shared by the callers.  Elements are dealt out
// by the caller's id; an element's value never depends on who computed it.
template <class Team>
EZPZ_MCM_HD void contributors(const Team team, const double* moments, uint64_t n_complete, uint32_t k, uint32_t m, double pivot_rel,
                              double* cov, double* beta, double* contrib, double* r2, uint64_t* dropped, double* L, double* d,
                              uint8_t* kept) {
    const uint32_t K = k + m, me = team.id(), step = team.count();
    if (n_complete < 2) {
        for (uint32_t e = me; e < K * K; e += step) cov[e] = quiet_nan();
        for (uint32_t e = me; e < m * k; e += step) beta[e] = contrib[e] = quiet_nan();
        for (uint32_t i = me; i < m; i += step) r2[i] = quiet_nan();
        if (me == 0) *dropped = ~0ull;
        return;
    }
    const double n = (double)n_complete, n1 = n - 1.0;
    for (uint32_t e = me; e < K * K; e += step) {
        const uint32_t r = e / K, c = e - r * K, a = r < c ? r : c, b = r < c ? c : r;
        cov[e] = (moments[g_at(K, a, b)] - moments[a] * moments[b] / n) / n1;
    }
    team.sync();
    // LDL^T of the input block, dimensions ascending; a dropped dimension is left out
    for (uint32_t j = 0; j < k; ++j) {
        const double cjj = cov[j * K + j];
        double dj = cjj;  // (every caller forms the pivot: the same loop, the same bits)
        for (uint32_t l = 0; l < j; ++l) {
            if (!kept[l]) continue;
            const double t = L[j * k + l] * d[l];
            dj = dj - L[j * k + l] * t;
        }
        const bool keep = cjj > 0.0 && dj > pivot_rel * cjj;
        if (keep) {
            for (uint32_t i = j + 1 + me; i < k; i += step) {
                double acc = cov[i * K + j];
                for (uint32_t l = 0; l < j; ++l) {
                    if (!kept[l]) continue;
                    const double t = L[j * k + l] * d[l];
                    acc = acc - L[i * k + l] * t;
                }
                L[i * k + j] = acc / dj;
            }
        }
        if (me == 0) d[j] = keep ? dj : 0.0, kept[j] = keep ? 1 : 0;
        team.sync();
    }
    if (me == 0) {
        uint64_t bits = 0;
        for (uint32_t j = 0; j < k; ++j)
            if (!kept[j]) bits |= 1ull << j;
        *dropped = bits;
    }
    // one caller per reference dimension: L y = c, w = y / d, L^T beta = w -- in place in the record's row of beta
    for (uint32_t i = me; i < m; i += step) {
        double* bi = beta + (size_t)i * k;
        for (uint32_t j = 0; j < k; ++j) {
            if (!kept[j]) {
                bi[j] = 0.0;
                continue;
            }
            double y = cov[j * K + k + i];
            for (uint32_t l = 0; l < j; ++l)
                if (kept[l]) y = y - L[j * k + l] * bi[l];
            bi[j] = y;
        }
        for (uint32_t j = 0; j < k; ++j)
            if (kept[j]) bi[j] = bi[j] / d[j];
        for (uint32_t jj = k; jj-- > 0;) {
            if (!kept[jj]) continue;
            double w = bi[jj];
            for (uint32_t l = jj + 1; l < k; ++l)
                if (kept[l]) w = w - L[l * k + jj] * bi[l];
            bi[jj] = w;
        }
        const double vm = cov[(k + i) * K + k + i];
        double explained = 0.0;
        for (uint32_t j = 0; j < k; ++j)
            if (kept[j]) explained = explained + bi[j] * cov[j * K + k + i];
        const bool has_var = vm > 0.0;
        r2[i] = has_var ? explained / vm : quiet_nan();
        for (uint32_t j = 0; j < k; ++j)
            contrib[(size_t)i * k + j] = !has_var ? quiet_nan() : kept[j] ? bi[j] * bi[j] * cov[j * K + j] / vm : 0.0;
    }
}

// ---- the host entry, whole: ezpz_mc_contributors forwards to it (and tools/asan_contrib.cpp drives it, host only) -----------------
inline int check_shape(size_t n_param, size_t n_meas) {  // K == 0, K > EZPZ_MC_MOMENT_MAX
    if (n_param > kMaxK || n_meas > kMaxK) return EZPZ_ERR_INVALID_ARGUMENT;
    const size_t K = n_param + n_meas;
    return K == 0 || K > kMaxK ? EZPZ_ERR_INVALID_ARGUMENT : EZPZ_OK;
}

inline void default_config(EzpzMcContribConfig* cc) {
    cc->pivot_rel = 0x1p-26;
    cc->reserved = 0;
}

inline int check_config(const EzpzMcContribConfig* cc, double& pivot_rel) {  // cc == NULL: the default
    EzpzMcContribConfig c;
    default_config(&c);
    if (cc) c = *cc;
    if (!(c.pivot_rel >= 0.0 && c.pivot_rel <= 1.7976931348623157e308)) return EZPZ_ERR_INVALID_ARGUMENT;
    pivot_rel = c.pivot_rel;
    return EZPZ_OK;
}

inline int contributors_host(const double* moments, uint64_t n_complete, size_t n_param, size_t n_meas, const EzpzMcContribConfig* cc,
                             double* cov, double* beta, double* contrib, double* r2, uint64_t* dropped) {
    if (int rc = check_shape(n_param, n_meas)) return rc;
    double pivot_rel = 0.0;
    if (int rc = check_config(cc, pivot_rel)) return rc;
    if (!moments || !cov || !dropped || (n_meas && !r2) || (n_meas && n_param && (!beta || !contrib))) return EZPZ_ERR_INVALID_ARGUMENT;
    double* L = new double[n_param * n_param + n_param + 1];  // the factor | the pivots
    uint8_t* kept = new uint8_t[n_param + 1];
    contributors(mcb::OneCaller{}, moments, n_complete, (uint32_t)n_param, (uint32_t)n_meas, pivot_rel, cov, beta, contrib, r2, dropped, L,
                 L + n_param * n_param, kept);
    delete[] L;
    delete[] kept;
    return EZPZ_OK;
}

#if defined(__HIPCC__) && !defined(EZPZ_MCM_HOST_ONLY)

// ---- the kernels' arguments (filled by the host side: mc_moments.hip and the run of tolerance_mc.hip) ----------------------------
struct ContribArgs {  // mc_contrib_kernel: the closing step's, n_complete read from `info` where the last round left it
    const double* moments;
    const EzpzMcMomentsInfo* info;
    uint32_t k, m;
    double pivot_rel;
    double *cov, *beta, *contrib, *r2;
    uint64_t* dropped;
};

struct MomentArgs {  // mc_moments_kernel: one round
    const double* params;   // [count][k]
    const double* m;        // [count][n_meas]
    const uint8_t* flags;   // [count][n_meas] (NULL: every bit clear)
    const uint8_t* ok;      // [count] (NULL: every one set)
    const double *nominal_p, *nominal_m;  // [k], [n_meas]
    uint64_t first, count, samples;
    uint32_t k, n_meas, first_round;
    double* part;         // [blocks][entries]
    uint32_t* part_n;     // [blocks]
    unsigned int* ticket;  // 0 between launches
    double* moments;
    EzpzMcMomentsInfo* info;
};

#ifdef EZPZ_MCM_KERNELS  // (mc_moments.hip alone: the kernels have one home; the run of tolerance_mc.hip takes the host side below)
// The factor and the pivots live in LDS (k <= 64: 32.5 KiB); the covariance and the coefficients are read where they are written,
// in the caller's arrays.
__global__ __launch_bounds__(256) void mc_contrib_kernel(ContribArgs a) {
    extern __shared__ double s_work[];
    double* L = s_work;
    double* d = L + (size_t)a.k * a.k;
    uint8_t* kept = (uint8_t*)(d + a.k);
    contributors(mcb::WorkgroupCallers{}, a.moments, a.info->n_complete, a.k, a.m, a.pivot_rel, a.cov, a.beta, a.contrib, a.r2, a.dropped, L, d, kept);
}

// ---- a round's second-moment sums --------------------------------------------------------------------------------------------------
// Workgroup q of a round takes the samples [first + 256 q, first + 256 q + 256): `first` is a multiple of 256, so these are the blocks
// of the interface whatever the round.  The block's 256 leaves of an entry split into four aligned sub-trees of 64 samples: a TILE of
// 64 samples' z is staged in LDS, sample-major ([s][K]: at K = 64 that is 32 KiB, not the block's 128), every thread sums its entries
// e = t, t + 256, .. over the tile by the adjacent-pair tree -- eight leaves at a time, their sums pushed through a three-deep binary
// counter, which is that tree -- and the four tiles' sums are joined as the tree's two upper levels, (T0 + T1) + (T2 + T3).  One
// partial per block and entry; the workgroup that draws the last ticket folds the round's partials, left to right, into the running
// moments the caller's buffer holds between rounds (the first round starts them), threads over entries.  No floating-point atomics.

constexpr uint32_t kTile = 64;  // samples staged at once
constexpr uint32_t kRounds = (kMaxEntries + 255) / 256;  // entries per thread at most: 9

// the adjacent-pair tree over N consecutive samples of the staged tile, N a power of two: the left half's sum + the right half's
template <int N>
__device__ inline double pair_sum(const double* za, const double* zb, uint32_t K, bool product) {
    if constexpr (N == 1) {
        return product ? *za * *zb : *za;
    } else {
        const double left = pair_sum<N / 2>(za, zb, K, product);
        return left + pair_sum<N / 2>(za + (N / 2) * K, zb + (N / 2) * K, K, product);
    }
}

// the tile's 64 leaves of one entry: eight leaves at a time through the binary counter (l0, l1, l2: the pending sums of 8, 16, 32).
// (mcb::tree_sum is this tree; the kernel keeps its own copy, on which it takes 190 VGPRs for the shared one's 194)
__device__ inline double tile_sum(const double* za, const double* zb, uint32_t K, bool product) {
    double l0 = 0.0, l1 = 0.0, l2 = 0.0, out = 0.0;
#pragma unroll 1
    for (uint32_t g = 0; g < kTile / 8; ++g) {
        double v = pair_sum<8>(za + g * 8 * K, zb + g * 8 * K, K, product);
        if (!(g & 1u)) {
            l0 = v;
            continue;
        }
        v = l0 + v;
        if (!(g & 2u)) {
            l1 = v;
            continue;
        }
        v = l1 + v;
        if (!(g & 4u)) {
            l2 = v;
            continue;
        }
        out = l2 + v;
    }
    return out;
}

__global__ __launch_bounds__(256) void mc_moments_kernel(MomentArgs a) {
    extern __shared__ double s_z[];  // [kTile][K]
    __shared__ uint32_t s_bad[kTile];
    __shared__ uint32_t s_complete;
    const uint32_t t = threadIdx.x, q = blockIdx.x, k = a.k, n_meas = a.n_meas, K = k + n_meas, E = entries_of(K);
    // this thread's entries: row ea and column eb of the triangle, or the sum of z[ea] (eb == ea, no product)
    uint32_t ea[kRounds], eb[kRounds];
    bool prod[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = t + 256 * r;
        ea[r] = eb[r] = 0;
        prod[r] = false;
        if (e >= K && e < E) {
            uint32_t row = 0, at = e - K;
            while (at >= K - row) at -= K - row, ++row;
            ea[r] = row, eb[r] = row + at, prod[r] = true;
        } else if (e < K) {
            ea[r] = eb[r] = e;
        }
    }
    double half[kRounds], acc[kRounds];  // (T0 + T1), and the block's sum
    if (t == 0) s_complete = 0;
    for (uint32_t tile = 0; tile < 256 / kTile; ++tile) {
        const uint64_t base = (uint64_t)q * 256 + tile * kTile;  // the tile's first sample, in the round
        __syncthreads();  // (the last tile's sums are read)
        if (t < kTile) {
            const uint64_t s = base + t;
            s_bad[t] = s < a.count && (!a.ok || a.ok[s]) ? 0u : 1u;
        }
        __syncthreads();
        for (uint32_t idx = t; idx < kTile * n_meas; idx += 256) {
            const uint32_t sl = idx / n_meas, i = idx - sl * n_meas;
            const uint64_t s = base + sl;
            if (s >= a.count) continue;
            const bool bad = (a.flags && (a.flags[s * n_meas + i] & 1u)) || !isfinite(a.m[s * n_meas + i]);
            if (bad) atomicOr(&s_bad[sl], 1u);
        }
        __syncthreads();
        for (uint32_t idx = t; idx < kTile * K; idx += 256) {
            const uint32_t sl = idx / K, c = idx - sl * K;
            const uint64_t s = base + sl;
            double z = 0.0;
            if (!s_bad[sl]) z = c < k ? a.params[s * k + c] - a.nominal_p[c] : a.m[s * n_meas + (c - k)] - a.nominal_m[c - k];
            s_z[idx] = z;
        }
        if (t < kTile && !s_bad[t]) atomicAdd(&s_complete, 1u);
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r) {
            if (t + 256 * r >= E) continue;
            const double v = tile_sum(s_z + ea[r], s_z + eb[r], K, prod[r]);
            if (tile == 0)
                half[r] = v;
            else if (tile == 1)
                half[r] = half[r] + v;
            else if (tile == 2)
                acc[r] = v;
            else
                acc[r] = half[r] + (acc[r] + v);
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r)
        if (t + 256 * r < E) a.part[(uint64_t)q * E + t + 256 * r] = acc[r];
    if (t == 0) a.part_n[q] = s_complete;
    if (!mcb::last_block(a.ticket)) return;
    mcb::fold_partials(a.part, E, a.first_round, a.moments);
    if (t == 0) {
        EzpzMcMomentsInfo info;
        info.n_complete = a.first_round ? 0 : a.info->n_complete;
        info.samples = a.samples;
        for (uint32_t b = 0; b < gridDim.x; ++b) info.n_complete += a.part_n[b];
        *a.info = info;
        *a.ticket = 0;
    }
}

#endif  // EZPZ_MCM_KERNELS

// ---- the host side (mc_moments.hip), shared with the run of tolerance_mc.hip ---------------------------------------------------------
// one round: `a` with the samples' arrays, first, count, samples, k, n_meas, first_round, moments and info set; the workspace holds
// blocks * entries_of(K) partials and `blocks` counts
int enqueue_moments(mcb::Work& work, MomentArgs a, hipStream_t stream);
int enqueue_contributors(const ContribArgs& a, hipStream_t stream);

#endif  // __HIPCC__ && !EZPZ_MCM_HOST_ONLY

}  // namespace mcm
}  // namespace ezpz
