// Monte-Carlo tolerance analysis (include/ezpz_amd.h: ezpz_mc_sample, ezpz_system_tolerance_mc[_device]): the three
// kernels of a round -- mc_sample_kernel (the round's driven values), mc_broadcast_kernel (its copies of x0) and mc_reduce_kernel
// (the round's statistics, folded into the running results) -- and mc_sample_pick_kernel, the sampler of the Sobol indices' pick-freeze
// matrices, and mc_sample_walk_kernel, the sampler of a list with low-discrepancy dimensions.  The sampler itself -- one __host__ __device__ body behind the host
// entry and the sampler kernel -- is in mc_sampler.hip.hpp; the host plan and the entries are in tolerance_mc.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ezpz_amd.h"
#include "mc_sampler.hip.hpp"

namespace ezpz {
namespace mc {

#ifdef __HIPCC__

// ---- the round's driven values: params[s][j] for the samples first + s, s < count ------------------------------------------------
__global__ __launch_bounds__(256) void mc_sample_kernel(const Dist* __restrict__ dist, uint64_t seed, uint64_t first, uint64_t count,
                                                        uint32_t n_param, double* __restrict__ params) {
    const uint64_t total = count * n_param, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const uint64_t s = idx / n_param;
        const uint32_t j = (uint32_t)(idx - s * n_param);
        params[idx] = draw_plain(seed, first + s, j, dist[j]);
    }
}

// ---- the same for a list with flagged dimensions (EZPZ_MC_SEQUENCE) -----------------------------------------------
// A work item is kWalkRun consecutive samples of one dimension, and neighbouring lanes take neighbouring dimensions of the same
// samples, so a wavefront's stores of one step are whole runs of a row.  A flagged dimension evaluates its first point directly --
// one table word per set bit of the Gray code -- and steps to each next one with one word and one XOR; the shift is one Philox
// block per work item.  The arithmetic is integer: the walk gives the bits of the direct evaluation wherever it starts, so the
// rounds and the grid stride do not show.  An unflagged dimension of the list is the plain draw.  kLds: the first min(n_param, 64)
// rows of the table are staged in LDS (8 KiB at most) and the steps read them there; else every read goes to constant memory.
constexpr uint32_t kWalkRun = 8;
template <bool kLds>
__global__ __launch_bounds__(256) void mc_sample_walk_kernel(const Dist* __restrict__ dist, uint64_t seed, uint64_t first, uint64_t count,
                                                             uint32_t n_param, double* __restrict__ params) {
    __shared__ uint32_t s_v[kLds ? kSequenceDims * kSequenceBits : 1];
    if (kLds) {
        const uint32_t words = (n_param < kSequenceDims ? n_param : kSequenceDims) * kSequenceBits;
        for (uint32_t i = threadIdx.x; i < words; i += 256) s_v[i] = kSequenceDevice[0][i];
        __syncthreads();
    }
    const uint64_t runs = (count + kWalkRun - 1) / kWalkRun, total = runs * n_param, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const uint64_t run = idx / n_param;
        const uint32_t j = (uint32_t)(idx - run * n_param);
        const uint64_t s0 = run * kWalkRun, s1 = s0 + kWalkRun < count ? s0 + kWalkRun : count;
        const Dist d = dist[j];
        double* out = params + s0 * n_param + j;
        if (!d.sequence) {
            for (uint64_t s = s0; s < s1; ++s, out += n_param) *out = draw_plain(seed, first + s, j, d);
            continue;
        }
        // (a flagged dimension: j < 64 and first + count <= 2^32, by check_dists)
        const uint32_t* v = kLds ? s_v + j * kSequenceBits : kSequenceDevice[j];
        const uint32_t shift = sequence_shift(seed, j);
        uint32_t b = (uint32_t)(first + s0), x = sequence_point(v, b);
        for (uint64_t s = s0;; out += n_param) {
            *out = sequence_value(x ^ shift, d);
            if (++s == s1) break;
            x = sequence_step(v, x, ++b);
        }
    }
}

// ... and with every point evaluated directly, one draw per work item as in mc_sample_kernel: the measurements' other side
__global__ __launch_bounds__(256) void mc_sample_direct_kernel(const Dist* __restrict__ dist, uint64_t seed, uint64_t first, uint64_t count,
                                                               uint32_t n_param, double* __restrict__ params) {
    const uint64_t total = count * n_param, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const uint64_t s = idx / n_param;
        const uint32_t j = (uint32_t)(idx - s * n_param);
        params[idx] = draw(seed, first + s, j, dist[j]);
    }
}

// ---- the same with the seed chosen per column (the pick-freeze matrices of the Sobol indices): column `pick` is
// drawn with seed_b and every other one with seed_a -- kPickNone: all of them with seed_a (matrix A), kPickAll: all with seed_b (B)
constexpr uint32_t kPickNone = 0xFFFFFFFFu, kPickAll = 0xFFFFFFFEu;
__global__ __launch_bounds__(256) void mc_sample_pick_kernel(const Dist* __restrict__ dist, uint64_t seed_a, uint64_t seed_b, uint32_t pick,
                                                             uint64_t first, uint64_t count, uint32_t n_param, double* __restrict__ params) {
    const uint64_t total = count * n_param, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const uint64_t s = idx / n_param;
        const uint32_t j = (uint32_t)(idx - s * n_param);
        params[idx] = draw_plain(pick == kPickAll || j == pick ? seed_b : seed_a, first + s, j, dist[j]);  // (no flagged dimension: SobolOut::check)
    }
}

// ---- `count` copies of x0 ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mc_broadcast_kernel(const double* __restrict__ x0, uint32_t n_vars, uint64_t count,
                                                           double* __restrict__ x) {
    const uint64_t total = count * n_vars, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) x[idx] = x0[idx % n_vars];
}

// ---- the round's statistics ----------------------------------------------------------------------------------------------------------
// Workgroup q of a round takes the samples [first + 256 q, first + 256 q + 256): `first` is a multiple of 256, so these are the blocks
// of the interface whatever the round.  Per measurement it sums d and d * d over the block by the adjacent-pair tree -- the
// wavefront's butterfly (lane 0 of a shift-down by 1, 2, .. 32 holds exactly that tree), then the four wavefronts' sums folded the
// same way -- and leaves one partial per block; the workgroup that finishes last folds the round's partials, left to right, into
// the running results the caller's `stats` and `totals` hold between rounds (the first round starts them).  Counts ride along as
// integers; the histogram is counted in LDS and added to the caller's with integer atomics.  No floating-point atomics.
struct ReduceArgs {
    const double* m;           // [count][n_meas]
    const uint8_t* flags;      // [count][n_meas]
    const EzpzStatus* status;  // [count]
    const double* nominal;     // [n_meas]
    const double *lim_lo, *lim_hi, *hist_lo, *hist_scale;  // [n_meas] each; the limits and the histogram's tables optional
    uint64_t first, count, samples;
    uint32_t n_meas, hist_bins, first_round;
    // per block of the round: [blocks][n_meas], and [blocks] for the two totals
    double *part_d, *part_d2, *part_min, *part_max;
    uint64_t *part_argmin, *part_argmax;
    uint32_t *part_valid, *part_in, *part_ok, *part_all_in;
    unsigned int* ticket;  // 0 between launches
    uint8_t* ok;           // [count]: the round's ok bytes
    EzpzMcStats* stats;
    EzpzMcTotals* totals;
    uint64_t* hist;  // [n_meas][hist_bins + 2]
};

__device__ inline double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

__global__ __launch_bounds__(256) void mc_reduce_kernel(ReduceArgs a) {
    __shared__ double s_d[4], s_d2[4], s_min[4], s_max[4];
    __shared__ uint32_t s_imin[4], s_imax[4], s_valid[4], s_in[4];
    __shared__ uint32_t s_hist[66];
    __shared__ uint32_t s_last;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, q = blockIdx.x, n_meas = a.n_meas;
    const uint64_t local = (uint64_t)q * 256 + t;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    bool ok = false;
    if (local < a.count) {
        const EzpzStatus st = a.status[local];
        ok = st.converged != 0 && st.n_unsatisfied == 0;
        a.ok[local] = ok ? 1 : 0;
    }
    bool all_in = ok;
    for (uint32_t i = 0; i < n_meas; ++i) {
        __syncthreads();  // (thread 0 has read the last record's partials, the histogram's slots are flushed)
        if (a.hist_bins && t < a.hist_bins + 2) s_hist[t] = 0;
        if (a.hist_bins) __syncthreads();
        double m = 0.0;
        bool valid = false;
        if (ok) {
            m = a.m[local * n_meas + i];
            valid = !(a.flags[local * n_meas + i] & 1u) && isfinite(m);
        }
        const bool in = valid && (!a.lim_lo || (a.lim_lo[i] <= m && m <= a.lim_hi[i]));
        all_in = all_in && in;
        const double dev = m - a.nominal[i];
        double d = valid ? dev : 0.0, d2 = valid ? dev * dev : 0.0;
        double vmin = valid ? m : inf, vmax = valid ? m : -inf;
        uint32_t imin = valid ? t : 0xFFFFFFFFu, imax = imin;
        if (valid && a.hist_bins) {
            uint32_t slot = 0;
            if (!(m < a.hist_lo[i])) {
                const double bin = floor((m - a.hist_lo[i]) * a.hist_scale[i]);
                slot = bin >= (double)a.hist_bins ? a.hist_bins + 1 : 1 + (uint32_t)bin;
            }
            atomicAdd(&s_hist[slot], 1u);
        }
        for (uint32_t h = 1; h < 64; h <<= 1) {
            d += __shfl_down(d, h);
            d2 += __shfl_down(d2, h);
            const double omin = __shfl_down(vmin, h), omax = __shfl_down(vmax, h);
            const uint32_t oimin = __shfl_down(imin, h), oimax = __shfl_down(imax, h);
            if (omin < vmin || (omin == vmin && oimin < imin)) vmin = omin, imin = oimin;
            if (omax > vmax || (omax == vmax && oimax < imax)) vmax = omax, imax = oimax;
        }
        const uint32_t n_valid = (uint32_t)__popcll(__ballot(valid)), n_in = (uint32_t)__popcll(__ballot(in));
        if (lane == 0) {
            s_d[wave] = d, s_d2[wave] = d2, s_min[wave] = vmin, s_max[wave] = vmax;
            s_imin[wave] = imin, s_imax[wave] = imax, s_valid[wave] = n_valid, s_in[wave] = n_in;
        }
        __syncthreads();
        if (t == 0) {
            const uint64_t at = (uint64_t)q * n_meas + i, base = a.first + (uint64_t)q * 256;
            a.part_d[at] = (s_d[0] + s_d[1]) + (s_d[2] + s_d[3]);
            a.part_d2[at] = (s_d2[0] + s_d2[1]) + (s_d2[2] + s_d2[3]);
            double bmin = s_min[0], bmax = s_max[0];
            uint32_t bimin = s_imin[0], bimax = s_imax[0];
            for (uint32_t w = 1; w < 4; ++w) {  // (ascending sample index: a strict comparison keeps the lowest among equals)
                if (s_min[w] < bmin) bmin = s_min[w], bimin = s_imin[w];
                if (s_max[w] > bmax) bmax = s_max[w], bimax = s_imax[w];
            }
            a.part_min[at] = bmin, a.part_max[at] = bmax;
            a.part_argmin[at] = bimin == 0xFFFFFFFFu ? ~0ull : base + bimin;
            a.part_argmax[at] = bimax == 0xFFFFFFFFu ? ~0ull : base + bimax;
            a.part_valid[at] = s_valid[0] + s_valid[1] + s_valid[2] + s_valid[3];
            a.part_in[at] = s_in[0] + s_in[1] + s_in[2] + s_in[3];
        }
        if (a.hist_bins && t < a.hist_bins + 2 && s_hist[t])
            atomicAdd((unsigned long long*)&a.hist[(uint64_t)i * (a.hist_bins + 2) + t], (unsigned long long)s_hist[t]);
    }
    __syncthreads();
    {
        const uint32_t n_ok = (uint32_t)__popcll(__ballot(ok)), n_all = (uint32_t)__popcll(__ballot(all_in));
        if (lane == 0) s_valid[wave] = n_ok, s_in[wave] = n_all;
    }
    __syncthreads();
    if (t == 0) {
        a.part_ok[q] = s_valid[0] + s_valid[1] + s_valid[2] + s_valid[3];
        a.part_all_in[q] = s_in[0] + s_in[1] + s_in[2] + s_in[3];
        // the partials are out before the ticket is drawn; whoever draws the last one sees every block's.  (mcb::last_block's
        // step, with the fence in the one thread that wrote them: with it in all four wavefronts a run measured some 10 us a
        // round slower; profiles/mc_block_sum_ab.txt, section 2)
        __threadfence();
        s_last = atomicAdd(a.ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    const uint32_t blocks = gridDim.x;
    for (uint32_t i = t; i < n_meas; i += 256) {
        EzpzMcStats s;
        if (a.first_round) {
            s.n_valid = s.n_in = 0;
            s.argmin = s.argmax = ~0ull;
            s.sum_d = s.sum_d2 = 0.0;
            s.min = inf, s.max = -inf;
        } else {
            s = a.stats[i];
        }
        s.nominal = a.nominal[i];
        // (the sums depend on each other, the loads do not: unrolled, several blocks' partials are in flight at once)
#pragma unroll 8
        for (uint32_t b = 0; b < blocks; ++b) {
            const uint64_t at = (uint64_t)b * n_meas + i;
            s.sum_d += a.part_d[at];
            s.sum_d2 += a.part_d2[at];
            if (a.part_min[at] < s.min) s.min = a.part_min[at], s.argmin = a.part_argmin[at];
            if (a.part_max[at] > s.max) s.max = a.part_max[at], s.argmax = a.part_argmax[at];
            s.n_valid += a.part_valid[at];
            s.n_in += a.part_in[at];
        }
        const double n = (double)s.n_valid;
        s.mean = s.n_valid ? s.nominal + s.sum_d / n : quiet_nan();
        s.var = s.n_valid > 1 ? (s.sum_d2 - s.sum_d * s.sum_d / n) / (n - 1.0) : quiet_nan();
        a.stats[i] = s;
    }
    if (t == 0) {
        EzpzMcTotals tot;
        if (a.first_round)
            tot.n_ok = tot.n_all_in = 0;
        else
            tot = *a.totals;
        tot.samples = a.samples;
        for (uint32_t b = 0; b < blocks; ++b) tot.n_ok += a.part_ok[b], tot.n_all_in += a.part_all_in[b];
        *a.totals = tot;
        *a.ticket = 0;
    }
}

#endif  // __HIPCC__

}  // namespace mc
}  // namespace ezpz
