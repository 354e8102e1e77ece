// Factorial effects of a corner run (include/ezpz_amd.h: ezpz_mc_factorial[_device], ezpz_system_tolerance_mc_factorial[_device];
// DESIGN.md 3r): the closing body -- the masks, var, first, total and the record, ONE __host__ __device__ body behind the host form
// and the closing kernel's thread -- the host form (plain C++, explicit loops: no device), and the kernels of the device form: the
// gather (validity counts, the nominal taken off, the first kTa levels, the transposed store), the strided levels (kG at a launch),
// the walk (scale, coef, the masked block sums) and the close (the blocks left to right, main, pair, the closing body).  The
// process-wide plan and the entries of the reduction alone are in mc_factorial.hip; the run is in tolerance_mc.hip, on its plan.
//
// Built without contraction (build.py: -ffp-contract=off for every unit).  A butterfly is two single rounded operations on its two
// inputs, and IEEE addition commutes bit for bit on the finite values a complete record holds: no tiling, lane mapping or pass
// structure can change a bit of the transform.  The sums have the family's fixed order.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ezpz_amd.h"
#include "mc_block_sum.hip.hpp"  // (a host-only user, EZPZ_MCF_HOST_ONLY, takes the closing body and the host form alone: tools/asan_factorial.cpp)

namespace ezpz {
namespace mcf {

#define EZPZ_MCF_HD __host__ __device__ inline

constexpr uint32_t kMaxCorners = EZPZ_MC_FACTORIAL_MAX_CORNERS;
constexpr uint32_t kMaxMeas = EZPZ_MC_FACTORIAL_MAX_MEAS;
using mcb::kBlock;                                   // leaves per block of the sums
constexpr uint32_t kMaxSums = 2 * kMaxCorners + 1;  // ss_order [kc + 1] | ss_total [kc]

EZPZ_MCF_HD double quiet_nan() {
#ifdef __HIP_DEVICE_COMPILE__
    return __longlong_as_double(0x7FF8000000000000ll);
#else
    const uint64_t bits = 0x7FF8000000000000ull;
    double v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
#endif
}
EZPZ_MCF_HD bool finite_value(double v) {
#ifdef __HIP_DEVICE_COMPILE__
    return (__double_as_longlong(v) & 0x7FF0000000000000ll) != 0x7FF0000000000000ll;
#else
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return (b & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
#endif
}
EZPZ_MCF_HD uint32_t popcount32(uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}

// does coefficient S count in sum `k` of a record: k <= kc: the order popcount(S) == k; else: bit k - kc - 1 of S set
EZPZ_MCF_HD bool in_class(uint32_t S, uint32_t k, uint32_t kc) { return k <= kc ? popcount32(S) == k : ((S >> (k - kc - 1)) & 1u) != 0; }

// ---- the closing body ----------------------------------------------------------------------------------------------------------------
// One caller per record i.  main [kc], ss_order [kc + 1], ss_total [kc]: the record's, already written (NaN for an incomplete one);
// first, total [kc]: written here.  m [N][n_meas]: the rows, for the two predicted corners.
EZPZ_MCF_HD EzpzMcFactorial record_of(uint64_t n_valid, uint32_t kc, uint32_t n_meas, uint32_t i, const double* m, double mean_dev,
                                      const double* main, const double* ss_order, const double* ss_total, double* first, double* total) {
    EzpzMcFactorial r;
    r.n_valid = n_valid;
    r.reserved = 0;
    if (n_valid != (1ull << kc)) {
        const double nan = quiet_nan();
        r.complete = r.corner_hi = r.corner_lo = 0;
        r.mean_dev = r.var = r.m_hi = r.m_lo = nan;
        for (uint32_t c = 0; c < kc; ++c) first[c] = total[c] = nan;
        return r;
    }
    r.complete = 1;
    uint32_t hi = 0, lo = 0;
    for (uint32_t c = 0; c < kc; ++c) {
        if (main[c] > 0.0) hi |= 1u << c;
        if (main[c] < 0.0) lo |= 1u << c;
    }
    double var = 0.0;
    for (uint32_t o = 1; o <= kc; ++o) var = var + ss_order[o];
    for (uint32_t c = 0; c < kc; ++c) {
        const double sq = main[c] * main[c];
        first[c] = var == 0.0 ? 0.0 : sq / var;
        total[c] = var == 0.0 ? 0.0 : ss_total[c] / var;
    }
    r.corner_hi = hi, r.corner_lo = lo;
    r.mean_dev = mean_dev, r.var = var;
    r.m_hi = m[(size_t)hi * n_meas + i], r.m_lo = m[(size_t)lo * n_meas + i];
    return r;
}

// ---- the argument checks shared by the entries of the reduction alone: the pointers are only compared with NULL -------------------------
inline int check(uint32_t n_corner, size_t n_meas, const void* m, const void* nominal_m, const void* info, const void* main,
                 const void* pair, const void* ss_order, const void* ss_total, const void* first, const void* total) {
    if (n_corner == 0 || n_corner > kMaxCorners || n_meas == 0 || n_meas > kMaxMeas) return EZPZ_ERR_INVALID_ARGUMENT;
    if (!m || !nominal_m || !info || !main || !pair || !ss_order || !ss_total || !first || !total) return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

// ---- the host form, whole: ezpz_mc_factorial forwards to it (tools/asan_factorial.cpp drives it) --------------------------------------
inline int factorial_host(const double* m, const uint8_t* flags, const uint8_t* ok, const double* nominal_m, uint32_t n_corner, size_t n_meas,
                          EzpzMcFactorial* info, double* main, double* pair, double* ss_order, double* ss_total, double* first, double* total,
                          double* coef) {
    if (int rc = check(n_corner, n_meas, m, nominal_m, info, main, pair, ss_order, ss_total, first, total)) return rc;
    const uint32_t kc = n_corner, M = (uint32_t)n_meas, K = 2 * kc + 1;
    const size_t N = (size_t)1 << kc;
    const double scale = 1.0 / (double)N, nan = quiet_nan();
    std::vector<double> w(N), leaves(kBlock);
    for (uint32_t i = 0; i < M; ++i) {
        uint64_t n_valid = 0;
        for (size_t b = 0; b < N; ++b) {
            const size_t at = b * M + i;
            const double v = m[at];
            if ((!ok || ok[b]) && (!flags || !(flags[at] & 1u)) && finite_value(v)) ++n_valid;
            w[b] = v - nominal_m[i];
        }
        const bool complete = n_valid == N;
        double* mn = main + (size_t)i * kc;
        double* pr = pair + (size_t)i * kc * kc;
        double* so = ss_order + (size_t)i * (kc + 1);
        double* st = ss_total + (size_t)i * kc;
        if (!complete) {
            for (uint32_t c = 0; c < kc; ++c) mn[c] = st[c] = nan;
            for (uint32_t e = 0; e < kc * kc; ++e) pr[e] = nan;
            for (uint32_t o = 0; o <= kc; ++o) so[o] = nan;
            if (coef)
                for (size_t S = 0; S < N; ++S) coef[(size_t)i * N + S] = nan;
            info[i] = record_of(n_valid, kc, M, i, m, nan, mn, so, st, first + (size_t)i * kc, total + (size_t)i * kc);
            continue;
        }
        for (uint32_t l = 0; l < kc; ++l) {
            const size_t h = (size_t)1 << l;
            for (size_t b = 0; b < N; ++b) {
                if (b & h) continue;
                const double lo = w[b], hi = w[b + h];
                w[b] = lo + hi;
                w[b + h] = hi - lo;
            }
        }
        for (size_t S = 0; S < N; ++S) w[S] = w[S] * scale;
        if (coef)
            for (size_t S = 0; S < N; ++S) coef[(size_t)i * N + S] = w[S];
        for (uint32_t k = 0; k < K; ++k) {
            double sum = 0.0;
            for (size_t first_S = 0; first_S < N; first_S += kBlock) {
                for (uint32_t t = 0; t < kBlock; ++t) {
                    const size_t S = first_S + t;
                    leaves[t] = S < N && in_class((uint32_t)S, k, kc) ? w[S] * w[S] : 0.0;
                }
                sum = sum + mcb::pair_tree_256(leaves.data());
            }
            (k <= kc ? so[k] : st[k - kc - 1]) = sum;
        }
        for (uint32_t c = 0; c < kc; ++c) mn[c] = w[(size_t)1 << c];
        for (uint32_t c = 0; c < kc; ++c)
            for (uint32_t e = 0; e < kc; ++e) pr[c * kc + e] = c == e ? 0.0 : w[((size_t)1 << c) | ((size_t)1 << e)];
        info[i] = record_of(n_valid, kc, M, i, m, w[0], mn, so, st, first + (size_t)i * kc, total + (size_t)i * kc);
    }
    return EZPZ_OK;
}

#if defined(__HIPCC__) && !defined(EZPZ_MCF_HOST_ONLY)

// ---- the tiling (DESIGN.md 3r says why) ------------------------------------------------------------------------------------------
constexpr uint32_t kTa = 7;      // the gather: tiles of 2^kTa rows, levels 0 .. kTa - 1 in LDS
constexpr uint32_t kG = 7;       // a strided launch: up to kG levels
constexpr uint32_t kRun = 32;    // ... on runs of kRun contiguous doubles (256 bytes) per group
constexpr uint32_t kLdsDoubles = kRun * ((1u << kG) + 1);        // 4128: the strided tile, rows padded by one double
// the LDS row of the gather: 2^kTa values and a pad that spreads the transposed store (16-lane groups, 32 banks of 4 bytes) over the banks
inline __host__ __device__ uint32_t gather_pitch(uint32_t n_meas) { return (1u << kTa) + (16 + n_meas - 1) / n_meas; }
static_assert(kTa <= 7 && kG <= 7 && kMaxMeas * ((1u << kTa) + 1) <= kLdsDoubles && 15 * ((1u << kTa) + 16) <= kLdsDoubles,
              "lds_levels has seven levels; the gather's tile fits the strided one's room at every n_meas");

// ---- the kernels' arguments (filled by the host side: mc_factorial.hip) ---------------------------------------------------------------
struct FactorialArgs {
    const double* m;       // [N][n_meas]
    const uint8_t* flags;  // (NULL: every bit clear)
    const uint8_t* ok;     // (NULL: every one set)
    const double* nominal_m;
    uint32_t kc, n_meas;
    uint32_t level0, levels;  // the strided launch: levels level0 .. level0 + levels - 1
    uint32_t blocks;          // ceil(N / 256)
    double scale;             // 2^-kc
    double* w;                // [n_meas][N]: the work array
    uint32_t* cnt;            // [n_meas]: the valid rows; zero before the gather
    double* part;             // [n_meas][2 kc + 1][blocks]: the block sums
    EzpzMcFactorial* info;
    double *main, *pair, *ss_order, *ss_total, *first, *total, *coef;
};

#ifdef EZPZ_MCF_KERNELS  // (mc_factorial.hip alone: the kernels have one home)

// `levels` levels (at most 7) on `rows` arrays of 2^levels contiguous doubles in LDS, row r at s + r * pitch, by the 256 threads of the
// workgroup, between barriers of its own.  Levels below 6: a thread owns an element, its partner sits in the same wavefront and comes
// by a lane exchange; LDS is read and written once, consecutive lanes at consecutive doubles.  Level 6: a thread owns a pair 64
// doubles apart; a wavefront's reads and writes are 64 consecutive doubles each.
__device__ inline void lds_levels(double* s, uint32_t rows, uint32_t pitch, uint32_t levels) {
    const uint32_t t = threadIdx.x, lane = t & 63u, total = rows << levels, low = levels < 6 ? levels : 6;
    __syncthreads();
    for (uint32_t f0 = t - lane; f0 < total; f0 += 256) {  // (wave-uniform: every lane takes part in the exchanges)
        const uint32_t f = f0 + lane, r = f >> levels, q = f & ((1u << levels) - 1);
        const bool live = f < total;
        double x = live ? s[r * pitch + q] : 0.0;
        for (uint32_t l = 0; l < low; ++l) {
            const double p = __shfl_xor(x, 1 << l);
            x = (lane >> l) & 1u ? x - p : x + p;
        }
        if (live) s[r * pitch + q] = x;
    }
    __syncthreads();
    if (levels == 7) {
        for (uint32_t pp = t; pp < rows * 64; pp += 256) {
            const uint32_t r = pp >> 6, b = pp & 63u;
            double* at = s + r * pitch + b;
            const double lo = at[0], hi = at[64];
            at[0] = lo + hi;
            at[64] = hi - lo;
        }
        __syncthreads();
    }
}

// ---- phase 1: gather -------------------------------------------------------------------------------------------------------------
// Workgroups take tiles of 2^ta rows (ta = min(kc, kTa)) and read them as the flat array they are -- thread t the elements t, t + 256,
// .. of the tile: a wavefront reads 64 consecutive doubles, whole rows.  An element that is valid counts for its record (LDS integers,
// one global integer add per record and workgroup); its deviation goes to LDS transposed, the levels below ta run there, and the
// record's 2^ta values go to the work array as one contiguous run.
__global__ __launch_bounds__(256) void mc_factorial_gather_kernel(FactorialArgs a) {
    __shared__ double s_w[kLdsDoubles];
    __shared__ uint32_t s_cnt[kMaxMeas];
    const uint32_t t = threadIdx.x, M = a.n_meas, kc = a.kc, ta = kc < kTa ? kc : kTa, rows = 1u << ta, pitch = gather_pitch(M);
    const uint32_t N = 1u << kc, tiles = N >> ta;
    if (t < kMaxMeas) s_cnt[t] = 0;
    __syncthreads();
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t row0 = tile << ta;
        const double* mp = a.m + (size_t)row0 * M;
        const uint8_t* fp = a.flags ? a.flags + (size_t)row0 * M : nullptr;
        const uint8_t* op = a.ok ? a.ok + row0 : nullptr;
        for (uint32_t e = t; e < rows * M; e += 256) {
            const uint32_t s = e / M, i = e - s * M;
            const double v = mp[e];
            if ((!op || op[s]) && (!fp || !(fp[e] & 1u)) && finite_value(v)) atomicAdd(&s_cnt[i], 1u);
            s_w[i * pitch + s] = v - a.nominal_m[i];
        }
        lds_levels(s_w, M, pitch, ta);
        for (uint32_t f = t; f < rows * M; f += 256) {
            const uint32_t i = f >> ta, q = f & (rows - 1);
            a.w[(size_t)i * N + row0 + q] = s_w[i * pitch + q];
        }
        __syncthreads();  // (the next tile's stores wait for these reads)
    }
    if (t < M && s_cnt[t]) atomicAdd(&a.cnt[t], s_cnt[t]);
}

// ---- phase 2: strided levels -----------------------------------------------------------------------------------------------------
// Levels level0 .. level0 + levels - 1 (level0 >= kTa, so 2^level0 >= kRun).  Index b of a record splits into hi | mid | lo, mid the
// `levels` bits being transformed.  A tile is one record, one hi, one run of kRun consecutive lo and every mid: 2^levels groups of
// kRun contiguous doubles, 2^level0 doubles apart.  In LDS a tile is [lo][mid], rows one double longer than 2^levels: the loads' store
// (consecutive lanes at consecutive lo) and the read back both step through the banks one double a lane.
__global__ __launch_bounds__(256) void mc_factorial_strided_kernel(FactorialArgs a) {
    __shared__ double s_w[kLdsDoubles];
    const uint32_t t = threadIdx.x, kc = a.kc, l0 = a.level0, g = a.levels, mids = 1u << g, pitch = mids + 1;
    const uint32_t N = 1u << kc, runs = 1u << (l0 - 5), his = N >> (l0 + g);  // runs of kRun = 2^5 doubles per 2^level0
    const uint32_t tiles_rec = his * runs, tiles = tiles_rec * a.n_meas;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t i = tile / tiles_rec, rest = tile - i * tiles_rec, hi = rest / runs, run = rest - hi * runs;
        double* base = a.w + (size_t)i * N + ((size_t)hi << (l0 + g)) + (size_t)run * kRun;
        for (uint32_t e = t; e < mids * kRun; e += 256) {
            const uint32_t mid = e >> 5, lo = e & 31u;
            s_w[lo * pitch + mid] = base[((size_t)mid << l0) + lo];
        }
        lds_levels(s_w, kRun, pitch, g);
        for (uint32_t e = t; e < mids * kRun; e += 256) {
            const uint32_t mid = e >> 5, lo = e & 31u;
            base[((size_t)mid << l0) + lo] = s_w[lo * pitch + mid];
        }
        __syncthreads();
    }
}

// ---- phase 3: walk ---------------------------------------------------------------------------------------------------------------
// A wavefront takes one block of the sums, coefficients [256 q, 256 q + 256) of record i (workgroup (x, i): blocks 4 x .. 4 x + 3), a
// lane four consecutive ones: scaled (NaN for an incomplete record), written to coef where asked, squared, and for a complete record
// summed per class -- the 2 kc + 1 masked sums -- by the adjacent-pair tree: two levels in the lane's registers, six lane exchanges
// (both partners form the same rounded sum).  Most classes need no tree of their own.  Inside a block the high bits of S are q's, so
// bit c >= 8 holds every leaf of the block or none -- the tree over all leaves, once, or +0.0 -- and popcount(S) = popcount(q) +
// popcount(S & 255) lies in nine values: at most 1 + 8 + 9 trees, the others are +0.0, the sum of a block of +0.0 leaves.  Lane k
// keeps sum k and stores it in the block sums [record][sum][block], where the close reads a sum's blocks as one run.
__device__ inline double block_tree(const double (&sq)[4], uint32_t S, uint32_t N, uint32_t k, uint32_t kc, bool all) {
    double v[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) v[j] = S + j < N && (all || in_class(S + j, k, kc)) ? sq[j] : 0.0;
    double sum = (v[0] + v[1]) + (v[2] + v[3]);
    for (uint32_t h = 1; h < 64; h *= 2) sum = sum + __shfl_xor(sum, (int)h);
    return sum;
}

__global__ __launch_bounds__(256) void mc_factorial_walk_kernel(FactorialArgs a) {
    const uint32_t lane = threadIdx.x & 63u, q = blockIdx.x * 4 + (threadIdx.x >> 6), i = blockIdx.y, kc = a.kc, K = 2 * kc + 1, N = 1u << kc;
    if (q >= a.blocks) return;  // (a whole wavefront)
    const uint32_t S = q * kBlock + 4 * lane;
    const bool complete = a.cnt[i] == N;
    const double* w = a.w + (size_t)i * N;
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    if (!complete) {
        c[0] = c[1] = c[2] = c[3] = quiet_nan();
    } else if (S + 3 < N) {  // (N >= 4: the four are one aligned 32 bytes)
        const double2 lo = *reinterpret_cast<const double2*>(w + S), hi = *reinterpret_cast<const double2*>(w + S + 2);
        c[0] = lo.x * a.scale, c[1] = lo.y * a.scale, c[2] = hi.x * a.scale, c[3] = hi.y * a.scale;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (S + j < N) c[j] = w[S + j] * a.scale;
    }
    if (a.coef) {
        double* out = a.coef + (size_t)i * N;
        if (S + 3 < N && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {  // (the caller's array: aligned as a double, maybe no further)
            *reinterpret_cast<double2*>(out + S) = double2{c[0], c[1]};
            *reinterpret_cast<double2*>(out + S + 2) = double2{c[2], c[3]};
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (S + j < N) out[S + j] = c[j];
        }
    }
    if (!complete) return;
    const double sq[4] = {c[0] * c[0], c[1] * c[1], c[2] * c[2], c[3] * c[3]};
    const uint32_t pop_q = popcount32(q);
    const double whole = block_tree(sq, S, N, 0, kc, true);
    double mine = 0.0;
    for (uint32_t k = 0; k < K; ++k) {  // (every branch is the wavefront's: q, k and kc decide)
        double v;
        if (k <= kc)
            v = k >= pop_q && k - pop_q <= 8 ? block_tree(sq, S, N, k, kc, false) : 0.0;
        else if (k - kc - 1 < 8)
            v = block_tree(sq, S, N, k, kc, false);
        else
            v = (q >> (k - kc - 1 - 8)) & 1u ? whole : 0.0;
        if (lane == k) mine = v;
    }
    if (lane < K) a.part[((size_t)i * K + lane) * a.blocks + q] = mine;
}

// ---- phase 4: close --------------------------------------------------------------------------------------------------------------
// One workgroup per record: thread k < 2 kc + 1 adds the blocks of sum k left to right from +0.0; main and pair are gathered from the
// work array and scaled; one thread runs the closing body.
__global__ __launch_bounds__(256) void mc_factorial_close_kernel(FactorialArgs a) {
    __shared__ double s_sum[kMaxSums], s_main[kMaxCorners];
    const uint32_t t = threadIdx.x, i = blockIdx.x, kc = a.kc, K = 2 * kc + 1, N = 1u << kc;
    const uint32_t n_valid = a.cnt[i];
    const bool complete = n_valid == N;
    const double* w = a.w + (size_t)i * N;
    const double nan = quiet_nan();
    if (t < K) {
        double sum = complete ? 0.0 : nan;
        if (complete) {
            const double* part = a.part + ((size_t)i * K + t) * a.blocks;  // (the sum's blocks: one contiguous run)
            // (the sums depend on each other, the loads do not: unrolled, several blocks' partials are in flight at once)
#pragma unroll 8
            for (uint32_t b = 0; b < a.blocks; ++b) sum = sum + part[b];
        }
        s_sum[t] = sum;
        if (t <= kc)
            a.ss_order[(size_t)i * (kc + 1) + t] = sum;
        else
            a.ss_total[(size_t)i * kc + (t - kc - 1)] = sum;
    }
    if (t < kc) {
        const double v = complete ? w[1u << t] * a.scale : nan;
        s_main[t] = v;
        a.main[(size_t)i * kc + t] = v;
    }
    for (uint32_t e = t; e < kc * kc; e += 256) {
        const uint32_t c = e / kc, d = e - c * kc;
        a.pair[(size_t)i * kc * kc + e] = !complete ? nan : c == d ? 0.0 : w[(1u << c) | (1u << d)] * a.scale;
    }
    __syncthreads();
    if (t == 0)
        a.info[i] = record_of(n_valid, kc, a.n_meas, i, a.m, complete ? w[0] * a.scale : nan, s_main, s_sum, s_sum + kc + 1,
                              a.first + (size_t)i * kc, a.total + (size_t)i * kc);
}

#endif  // EZPZ_MCF_KERNELS

// ---- the host side (mc_factorial.hip), shared with the run of tolerance_mc.hip -------------------------------------------------------
// The reduction's workspace: whoever owns one orders the launches that use it (a LaunchOrder beside it) and waits for them before it
// grows.
struct FactorialWork {
    DevBuf<double> w, part;
    DevBuf<uint32_t> cnt;
    bool grows(uint32_t n_meas, uint32_t kc) const;
    int ensure(uint32_t n_meas, uint32_t kc);
};
// the outputs of the reduction: device pointers; coef may be NULL
struct FactorialOut {
    EzpzMcFactorial* info = nullptr;
    double *main = nullptr, *pair = nullptr, *ss_order = nullptr, *ss_total = nullptr, *first = nullptr, *total = nullptr, *coef = nullptr;
};
// the whole reduction on rows that stay where they are until it has run: the counts' reset, the gather, the strided launches, the walk
// and the close.  The arguments are checked; `cus`: the device's compute units
int enqueue_factorial(FactorialWork& work, const double* m, const uint8_t* flags, const uint8_t* ok, const double* nominal_m, uint32_t kc,
                      uint32_t n_meas, const FactorialOut& out, uint32_t cus, hipStream_t stream);

#endif  // __HIPCC__ && !EZPZ_MCF_HOST_ONLY

}  // namespace mcf
}  // namespace ezpz
