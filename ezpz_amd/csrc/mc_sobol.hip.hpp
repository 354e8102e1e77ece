// Sobol tolerance indices (include/ezpz_amd.h: ezpz_mc_sobol_indices, ezpz_mc_sobol_sums[_device], ezpz_system_tolerance_sobol[_device];
// DESIGN.md 3o): the closing step -- ONE __host__ __device__ body behind the host entry (one caller) and mc_sobol_close_kernel (the
// threads of one workgroup) -- the host form of the reduction (plain C++: no device), and the kernels: mc_sobol_kernel (a round's
// blocks of the pick-freeze sums, folded into the running sums) and mc_sobol_ok_kernel (a sub-round's ok bytes).  The process-wide
// plan and the entries of the reduction are in mc_sobol.hip; the run is in tolerance_mc.hip, on its plan.
//
// Built without contraction (build.py: -ffp-contract=off for every unit); the closing step is + - * / and comparisons alone, every
// output element computed by one caller: the same bits on both sides.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ezpz_amd.h"
#include "mc_block_sum.hip.hpp"  // (a host-only user, EZPZ_SOBOL_HOST_ONLY, takes the closing step and the host reduction alone: tools/asan_sobol.cpp)

namespace ezpz {
namespace sobol {

#define EZPZ_SOBOL_HD __host__ __device__ inline

constexpr uint32_t kMax = EZPZ_SOBOL_MAX;
using mcb::kBlock;  // samples per block of the sums

EZPZ_SOBOL_HD uint32_t width_of(uint32_t k) { return 4 + 4 * k; }  // the sums of one record
// A UNIT is what one lane sums: the pair (record i, dimension j) with its four sums P, Q, P2, Q2 -- or, for j == k, the record's
// own four: sA, sB, sAA, sBB.  Units are numbered u = j * m + i, so that row 2 + j of a sample lies at f[.. 2 m + u].
// the place of sum c (0 .. 3) of unit (i, j) in sums [m][4 + 4 k]
EZPZ_SOBOL_HD uint32_t sum_at(uint32_t k, uint32_t i, uint32_t j, uint32_t c) {
    return i * width_of(k) + (j == k ? c : 4 + c * k + j);
}

EZPZ_SOBOL_HD double quiet_nan() {
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
// Elements are dealt out by the caller's id: element e < m * (k + 1) is var[i] (j == k) or the four indices of (i, j); every caller
// forms the record's variance itself, with the same operations, so an element's value never depends on who computed it.
template <class Team>
EZPZ_SOBOL_HD void indices(const Team team, const double* sums, const uint64_t* n_complete, uint32_t k, uint32_t m, double* var,
                           double* first, double* total, double* first_var, double* total_var) {
    const uint32_t W = width_of(k);
    for (uint32_t e = team.id(); e < m * (k + 1); e += team.count()) {
        const uint32_t i = e / (k + 1), j = e - i * (k + 1);
        const double* s = sums + (size_t)i * W;
        double v = quiet_nan();
        const bool few = n_complete[i] < 2;
        const double n = (double)n_complete[i], n2 = 2.0 * n;
        if (!few) {
            const double sab = s[0] + s[1];
            const double mean = sab / n2;
            v = ((s[2] + s[3]) - sab * mean) / (n2 - 1.0);
        }
        if (j == k) {
            var[i] = v;
            continue;
        }
        const size_t at = (size_t)i * k + j;
        if (few || !(v > 0.0)) {
            first[at] = total[at] = first_var[at] = total_var[at] = quiet_nan();
            continue;
        }
        const double P = s[4 + j], Q = s[4 + k + j], P2 = s[4 + 2 * k + j], Q2 = s[4 + 3 * k + j];
        const double vv = v * v;
        const double pm = P / n;
        first[at] = pm / v;
        first_var[at] = ((P2 / n - pm * pm) / (n - 1.0)) / vv;
        const double qm = (Q / 2.0) / n;
        total[at] = (Q / n2) / v;
        total_var[at] = (((Q2 / 4.0) / n - qm * qm) / (n - 1.0)) / vv;
    }
}

// ---- the argument checks shared by every entry ---------------------------------------------------------------------------------------
inline int check_shape(size_t n_param, size_t n_meas) { return n_param > kMax || n_meas == 0 || n_meas > kMax ? EZPZ_ERR_INVALID_ARGUMENT : EZPZ_OK; }
inline int check_mask(uint32_t fixed_mask, size_t n_param) {
    return n_param < 32 && (fixed_mask >> n_param) ? EZPZ_ERR_INVALID_ARGUMENT : EZPZ_OK;
}

inline void default_config(EzpzSobolConfig* c) {
    c->seed_b = 0x9E3779B97F4A7C15ull;
    c->reserved = 0;
}

// ---- the host entries, whole: ezpz_mc_sobol_indices and ezpz_mc_sobol_sums forward to them (tools/asan_sobol.cpp drives them) --------
inline int indices_host(const double* sums, const uint64_t* n_complete, size_t n_param, size_t n_meas, double* var, double* first,
                        double* total, double* first_var, double* total_var) {
    if (int rc = check_shape(n_param, n_meas)) return rc;
    if (!sums || !n_complete || !var || (n_param && (!first || !total || !first_var || !total_var))) return EZPZ_ERR_INVALID_ARGUMENT;
    indices(mcb::OneCaller{}, sums, n_complete, (uint32_t)n_param, (uint32_t)n_meas, var, first, total, first_var, total_var);
    return EZPZ_OK;
}

// bit i of the answer: sample b (which exists) is INCOMPLETE for record i
inline uint32_t incomplete_host(const double* f, const uint8_t* flags, const uint8_t* ok, uint32_t fixed_mask, uint64_t b, uint32_t k, uint32_t m) {
    uint32_t bad = 0;
    const uint32_t all = m == 32 ? 0xFFFFFFFFu : (1u << m) - 1u;
    for (uint32_t r = 0; r < k + 2; ++r) {
        if (r >= 2 && ((fixed_mask >> (r - 2)) & 1u)) continue;
        if (ok && !ok[b * (k + 2) + r]) bad = all;
        for (uint32_t i = 0; i < m; ++i) {
            const uint64_t at = (b * (k + 2) + r) * m + i;
            if ((flags && (flags[at] & 1u)) || !std::isfinite(f[at])) bad |= 1u << i;
        }
    }
    return bad;
}

inline int sums_host(const double* f, const uint8_t* flags, const uint8_t* ok, const double* nominal_m, uint32_t fixed_mask, uint64_t samples,
                     size_t n_param, size_t n_meas, double* sums, uint64_t* n_complete) {
    if (int rc = check_shape(n_param, n_meas)) return rc;
    if (int rc = check_mask(fixed_mask, n_param)) return rc;
    if (samples && (!sums || !n_complete || !f || !nominal_m)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (samples == 0) return EZPZ_OK;
    const uint32_t k = (uint32_t)n_param, m = (uint32_t)n_meas, W = width_of(k), R = k + 2;
    for (size_t e = 0; e < (size_t)m * W; ++e) sums[e] = 0.0;
    for (uint32_t i = 0; i < m; ++i) n_complete[i] = 0;
    std::vector<uint32_t> bad(kBlock);
    std::vector<double> leaves(4 * kBlock);
    for (uint64_t first = 0; first < samples; first += kBlock) {
        for (uint32_t t = 0; t < kBlock; ++t) {
            bad[t] = first + t < samples ? incomplete_host(f, flags, ok, fixed_mask, first + t, k, m) : 0xFFFFFFFFu;
            if (first + t < samples)
                for (uint32_t i = 0; i < m; ++i) n_complete[i] += !((bad[t] >> i) & 1u);
        }
        for (uint32_t i = 0; i < m; ++i) {
            for (uint32_t j = 0; j <= k; ++j) {
                if (j < k && ((fixed_mask >> j) & 1u)) continue;  // (its four entries stay the +0.0 they were written as)
                for (uint32_t t = 0; t < kBlock; ++t) {
                    double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0;
                    if (!((bad[t] >> i) & 1u)) {
                        const double* row = f + (first + t) * R * m;
                        const double dA = row[i] - nominal_m[i], dB = row[m + i] - nominal_m[i];
                        if (j == k) {
                            l0 = dA, l1 = dB, l2 = dA * dA, l3 = dB * dB;
                        } else {
                            const double dj = row[(size_t)(2 + j) * m + i] - nominal_m[i];
                            const double d = dj - dA;
                            l0 = dB * d, l1 = d * d, l2 = l0 * l0, l3 = l1 * l1;
                        }
                    }
                    leaves[t] = l0, leaves[kBlock + t] = l1, leaves[2 * kBlock + t] = l2, leaves[3 * kBlock + t] = l3;
                }
                for (uint32_t c = 0; c < 4; ++c) {
                    double& s = sums[sum_at(k, i, j, c)];
                    s = s + mcb::pair_tree_256(leaves.data() + c * kBlock);
                }
            }
        }
    }
    return EZPZ_OK;
}

#if defined(__HIPCC__) && !defined(EZPZ_SOBOL_HOST_ONLY)

// ---- the kernels' arguments (filled by the host side: mc_sobol.hip and the run of tolerance_mc.hip) --------------------------------
struct SumArgs {  // mc_sobol_kernel: one round.  Element (s, r, i) of the round's rows is at s * stride_s + r * stride_r + i
    const double* f;
    const uint8_t* flags;  // (NULL: every bit clear)
    const uint8_t* ok;     // [s * ok_stride_s + r * ok_stride_r] (NULL: every one set)
    const double* nominal_m;
    uint64_t stride_s, stride_r, ok_stride_s, ok_stride_r;
    uint64_t count;
    uint32_t k, m, fixed_mask, first_round;
    double* part;         // [blocks][m (4 + 4 k)]
    uint32_t* part_n;     // [blocks][m]
    unsigned int* ticket;  // 0 between launches
    double* sums;
    uint64_t* n_complete;
};

struct CloseArgs {  // mc_sobol_close_kernel: the closing step's, on the sums where the last round left them
    const double* sums;
    const uint64_t* n_complete;
    uint32_t k, m;
    double *var, *first, *total, *first_var, *total_var;
};

#ifdef EZPZ_SOBOL_KERNELS  // (mc_sobol.hip alone: the kernels have one home; the run of tolerance_mc.hip takes the host side below)
__global__ __launch_bounds__(256) void mc_sobol_close_kernel(CloseArgs a) {
    indices(mcb::WorkgroupCallers{}, a.sums, a.n_complete, a.k, a.m, a.var, a.first, a.total, a.first_var, a.total_var);
}

// a sub-round's ok bytes, by the Monte-Carlo section's rule (row A's come from mc_reduce_kernel)
__global__ __launch_bounds__(256) void mc_sobol_ok_kernel(const EzpzStatus* __restrict__ status, uint64_t count, uint8_t* __restrict__ ok) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < count) ok[s] = status[s].converged != 0 && status[s].n_unsatisfied == 0 ? 1 : 0;
}

// ---- a round's pick-freeze sums ------------------------------------------------------------------------------------------------------
// Workgroup q of a round takes the samples [256 q, 256 q + 256) of the round, which starts at a multiple of 256: the blocks of the
// interface whatever the round.  First the block's completeness: 256 words in LDS, bit i of word s set when sample s is incomplete
// for record i, OR-ed with integer atomics by threads that walk the block's rows.  Then UNITS ACROSS LANES (sobol::sum_at): a lane
// owns a unit and walks samples, forming the four leaves of each from three values -- no cross-lane traffic, and a wavefront's
// lanes read consecutive doubles of row 2 + j.  The shape has U = m (k + 1) units, 1056 at most and 72 at (8, 8): where U <= 128 the
// block's samples are split into G = 256 / W aligned sub-trees (W: the power of two >= U, G <= 32), group g of W lanes sums the
// samples [g S, g S + S), S = 256 / G >= 8, and the G sums are joined in LDS as the tree's upper levels -- exactly the adjacent-pair
// tree, as mc_moments_kernel's tiles.  Inside a sub-tree: eight leaves by the explicit tree, the eights through a binary counter.
// One partial per block and sum; the workgroup that draws the last ticket folds the round's partials, left to right, into the
// caller's sums and n_complete (the first round starts them), threads over sums.  No floating-point atomics.
struct Quad {
    double a, b, c, d;
};
__device__ inline Quad operator+(const Quad& x, const Quad& y) { return Quad{x.a + y.a, x.b + y.b, x.c + y.c, x.d + y.d}; }

struct Unit {
    const double *fa, *fj;  // the unit's element of row 0 and of row 2 + j (row 1: fa + stride_r) of the block's first sample
    uint64_t stride_s, stride_r;
    double nominal;
    const uint32_t* bad;  // the completeness words
    uint32_t bit;         // the record's bit in them
    bool base;            // j == k: sA, sB, sAA, sBB
    __device__ inline Quad operator()(uint32_t s) const {
        if (bad[s] & bit) return Quad{0.0, 0.0, 0.0, 0.0};
        const double dA = fa[s * stride_s] - nominal, dB = fa[s * stride_s + stride_r] - nominal;
        if (base) return Quad{dA, dB, dA * dA, dB * dB};
        const double dj = fj[s * stride_s] - nominal;
        const double t = dj - dA;
        const double p = dB * t, q = t * t;
        return Quad{p, q, p * p, q * q};
    }
};

__global__ __launch_bounds__(256) void mc_sobol_kernel(SumArgs a) {
    __shared__ uint32_t s_bad[kBlock];
    __shared__ uint32_t s_n[kMax];
    __shared__ double s_join[kBlock * 4];  // [c][g][w]: group g's sum c of the unit of lane w
    const uint32_t t = threadIdx.x, q = blockIdx.x, k = a.k, m = a.m, R = k + 2, U = m * (k + 1), E = m * width_of(k);
    const uint64_t base = (uint64_t)q * kBlock;  // the block's first sample, in the round
    const uint32_t all = m == 32 ? 0xFFFFFFFFu : (1u << m) - 1u;
    // ---- completeness ----
    {
        uint32_t bad = base + t < a.count ? 0u : 0xFFFFFFFFu;
        if (a.ok && base + t < a.count)
            for (uint32_t r = 0; r < R; ++r)
                if (!(r >= 2 && ((a.fixed_mask >> (r - 2)) & 1u)) && !a.ok[(base + t) * a.ok_stride_s + r * a.ok_stride_r]) bad = all;
        s_bad[t] = bad;
        if (t < kMax) s_n[t] = 0;
    }
    __syncthreads();
    const uint32_t in_block = (uint32_t)(a.count - base < kBlock ? a.count - base : kBlock);
    for (uint32_t idx = t; idx < in_block * R * m; idx += 256) {  // (i fastest, then the row: a wavefront reads along the rows)
        const uint32_t s = idx / (R * m), rest = idx - s * (R * m), r = rest / m, i = rest - r * m;
        if (r >= 2 && ((a.fixed_mask >> (r - 2)) & 1u)) continue;
        const uint64_t at = (base + s) * a.stride_s + r * a.stride_r + i;
        if ((a.flags && (a.flags[at] & 1u)) || !isfinite(a.f[at])) atomicOr(&s_bad[s], 1u << i);
    }
    __syncthreads();
    {
        const uint32_t mine = s_bad[t];
        for (uint32_t i = 0; i < m; ++i) {
            const uint32_t n = (uint32_t)__popcll(__ballot(!((mine >> i) & 1u)));
            if ((t & 63u) == 0 && n) atomicAdd(&s_n[i], n);
        }
    }
    // ---- the sums ----
    uint32_t W = 256;  // lanes per group
    while (W / 2 >= U && W > 8) W /= 2;
    const uint32_t G = 256 / W, S = kBlock / G, g = t / W, w = t - g * W;
    double* part = a.part + (uint64_t)q * E;
    for (uint32_t u = w; u < U; u += W) {  // (G > 1: at most one turn)
        const uint32_t j = u / m, i = u - j * m;
        const bool fixed = j < k && ((a.fixed_mask >> j) & 1u);
        Quad v{0.0, 0.0, 0.0, 0.0};  // (a FIXED dimension: written as +0.0, not summed)
        if (!fixed) {
            Unit un;
            un.fa = a.f + base * a.stride_s + i;
            un.fj = un.fa + (uint64_t)(2 + (j < k ? j : 0)) * a.stride_r;
            un.stride_s = a.stride_s, un.stride_r = a.stride_r;
            un.nominal = a.nominal_m[i];
            un.bad = s_bad, un.bit = 1u << i;
            un.base = j == k;
            v = mcb::tree_sum<Quad>(un, g * S, S / 8);
        }
        if (G == 1) {
            part[sum_at(k, i, j, 0)] = v.a, part[sum_at(k, i, j, 1)] = v.b, part[sum_at(k, i, j, 2)] = v.c, part[sum_at(k, i, j, 3)] = v.d;
        } else {
            s_join[(0 * G + g) * W + w] = v.a, s_join[(1 * G + g) * W + w] = v.b;
            s_join[(2 * G + g) * W + w] = v.c, s_join[(3 * G + g) * W + w] = v.d;
        }
    }
    if (G > 1) {  // the tree's upper levels, one thread per unit and sum
        __syncthreads();
        for (uint32_t e = t; e < 4 * U; e += 256) {
            const uint32_t c = e / U, u = e - c * U, j = u / m, i = u - j * m;
            double* col = s_join + (size_t)c * G * W + u;
            for (uint32_t h = 1; h < G; h *= 2)
                for (uint32_t gg = 0; gg < G; gg += 2 * h) col[gg * W] = col[gg * W] + col[(gg + h) * W];
            part[sum_at(k, i, j, c)] = col[0];
        }
    }
    __syncthreads();  // (the counts are whole)
    if (t < m) a.part_n[(uint64_t)q * m + t] = s_n[t];
    if (!mcb::last_block(a.ticket)) return;
    const uint32_t blocks = gridDim.x;
    mcb::fold_partials(a.part, E, a.first_round, a.sums);
    if (t < m) {
        uint64_t n = a.first_round ? 0 : a.n_complete[t];
        for (uint32_t b = 0; b < blocks; ++b) n += a.part_n[(uint64_t)b * m + t];
        a.n_complete[t] = n;
    }
    if (t == 0) *a.ticket = 0;
}

#endif  // EZPZ_SOBOL_KERNELS

// ---- the host side (mc_sobol.hip), shared with the run of tolerance_mc.hip -------------------------------------------------------
// one round: `a` with the rows' arrays and strides, count, k, m, fixed_mask, first_round, sums and n_complete set; the workspace
// holds blocks * m * width_of(k) partials and blocks * m counts
int enqueue_sums(mcb::Work& work, SumArgs a, hipStream_t stream);
int enqueue_ok(const EzpzStatus* status, uint64_t count, uint8_t* ok, hipStream_t stream);
int enqueue_close(const CloseArgs& a, hipStream_t stream);

#endif  // __HIPCC__ && !EZPZ_SOBOL_HOST_ONLY

}  // namespace sobol
}  // namespace ezpz
