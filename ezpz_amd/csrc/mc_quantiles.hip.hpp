// Monte-Carlo quantiles (include/ezpz_amd.h: ezpz_mc_quantiles[_device], ezpz_system_tolerance_mc_quantiles[_device]):
// the rule -- the key, the ranks, the band and the interpolated value, ONE __host__ __device__ body behind the host form and the
// device's closing threads -- the host form (plain C++: no device), and the kernels of the device form: a most-significant-digit
// radix select over the keys, eight digits of eight bits, every counter an integer.  The process-wide plan and the entries of the
// selection alone are in mc_quantiles.hip; the run is in tolerance_mc.hip, on its plan.
//
// Built without contraction (build.py: -ffp-contract=off for every unit); the rule is * + - sqrt floor ceil and comparisons alone,
// every record written by one caller: the same bits on both sides.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ezpz_amd.h"
#ifndef EZPZ_QUANTILES_HOST_ONLY  // (a host-only user takes the rule and the host form alone: tools/asan_quantiles.cpp)
#include "system.hpp"
#endif

namespace ezpz {
namespace mcq {

#define EZPZ_MCQ_HD __host__ __device__ inline

constexpr uint32_t kMaxQ = EZPZ_MC_QUANTILE_MAX_PROBS;
constexpr uint32_t kMaxMeas = EZPZ_MC_QUANTILE_MAX_MEAS;
constexpr uint32_t kMaxSel = 4 * kMaxQ;  // the selections of one record: k, k + 1, k_lo, k_hi per probability
constexpr uint64_t kNone = ~0ull;

EZPZ_MCQ_HD uint64_t bits_of(double v) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint64_t)__double_as_longlong(v);
#else
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
#endif
}
EZPZ_MCQ_HD double double_of(uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __longlong_as_double((long long)b);
#else
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
#endif
}
EZPZ_MCQ_HD bool finite_bits(uint64_t b) { return (b & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }
// the total order on finite doubles as an unsigned order, -0.0 before +0.0, and back
EZPZ_MCQ_HD uint64_t key_of_bits(uint64_t b) { return b ^ ((b >> 63) ? ~0ull : 1ull << 63); }
EZPZ_MCQ_HD double value_of_key(uint64_t key) { return double_of(key ^ ((key >> 63) ? 1ull << 63 : ~0ull)); }
EZPZ_MCQ_HD double root_of(double v) {
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(v);
#else
    return std::sqrt(v);
#endif
}

// ---- the rule ----------------------------------------------------------------------------------------------------------------------
struct Ranks {
    double g;
    uint64_t k, k1, k_lo, k_hi;
};

// n >= 1 valid values, 0 <= p <= 1, z >= 0
EZPZ_MCQ_HD Ranks ranks_of(uint64_t n, double p, double z) {
    Ranks r;
    const double top = (double)(n - 1);
    const double h = p * top;
    r.k = (uint64_t)floor(h);
    r.g = h - (double)r.k;
    r.k1 = r.k + 1 < n - 1 ? r.k + 1 : n - 1;
    const double s = root_of(((double)n * p) * (1.0 - p));
    const double zs = z * s;
    const double a = h - zs, b = h + zs;
    r.k_lo = a <= 0.0 ? 0 : (uint64_t)floor(a);
    r.k_hi = b >= top ? n - 1 : (uint64_t)ceil(b);
    return r;
}

// the record from the four order statistics: x_k, x_k1, x_k_lo, x_k_hi
EZPZ_MCQ_HD EzpzMcQuantile record_of(uint64_t n, const Ranks& r, double lo, double hi, double band_lo, double band_hi) {
    EzpzMcQuantile q;
    q.n_valid = n, q.rank = r.k, q.rank_lo = r.k_lo, q.rank_hi = r.k_hi;
    q.frac = r.g, q.lo = lo, q.hi = hi;
    const double step = r.g * (hi - lo);
    q.value = r.g == 0.0 ? lo : lo + step;
    q.band_lo = band_lo, q.band_hi = band_hi;
    return q;
}

EZPZ_MCQ_HD EzpzMcQuantile empty_record() {  // no valid sample
    EzpzMcQuantile q;
    const double nan = double_of(0x7FF8000000000000ull);
    q.n_valid = 0, q.rank = q.rank_lo = q.rank_hi = kNone;
    q.frac = q.lo = q.hi = q.value = q.band_lo = q.band_hi = nan;
    return q;
}

// ---- the argument checks shared by every entry: `out`, `m` are only compared with NULL ------------------------------------------------
inline void default_config(EzpzMcQuantileConfig* c) {
    c->z = 0.0;
    c->reserved = 0;
}

inline int check(uint64_t samples, size_t n_meas, const double* probs, size_t n_q, const EzpzMcQuantileConfig* qc, const void* m,
                 const void* out, double& z) {
    if (n_meas == 0 || n_meas > kMaxMeas || n_q > kMaxQ || samples > 0xFFFFFFFFull) return EZPZ_ERR_INVALID_ARGUMENT;
    if (n_q && (!probs || !out)) return EZPZ_ERR_INVALID_ARGUMENT;
    for (size_t q = 0; q < n_q; ++q)
        if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return EZPZ_ERR_INVALID_ARGUMENT;
    z = qc ? qc->z : 0.0;
    if (!(z >= 0.0) || !std::isfinite(z)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (samples && !m) return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

// ---- the host form, whole: ezpz_mc_quantiles forwards to it (tools/asan_quantiles.cpp drives it) --------------------------------------
inline int quantiles_host(const double* m, const uint8_t* flags, const uint8_t* ok, uint64_t samples, size_t n_meas, const double* probs,
                          size_t n_q, const EzpzMcQuantileConfig* qc, EzpzMcQuantile* out) {
    double z;
    if (int rc = check(samples, n_meas, probs, n_q, qc, m, out, z)) return rc;
    if (samples == 0 || n_q == 0) return EZPZ_OK;
    std::vector<uint64_t> keys;
    keys.reserve(samples);
    for (size_t i = 0; i < n_meas; ++i) {
        keys.clear();
        for (uint64_t b = 0; b < samples; ++b) {
            const uint64_t at = b * n_meas + i, bits = bits_of(m[at]);
            if ((ok && !ok[b]) || (flags && (flags[at] & 1u)) || !finite_bits(bits)) continue;
            keys.push_back(key_of_bits(bits));
        }
        std::sort(keys.begin(), keys.end());
        const uint64_t n = keys.size();
        for (size_t q = 0; q < n_q; ++q) {
            if (n == 0) {
                out[i * n_q + q] = empty_record();
                continue;
            }
            const Ranks r = ranks_of(n, probs[q], z);
            out[i * n_q + q] = record_of(n, r, value_of_key(keys[r.k]), value_of_key(keys[r.k1]), value_of_key(keys[r.k_lo]),
                                         value_of_key(keys[r.k_hi]));
        }
    }
    return EZPZ_OK;
}

#if defined(__HIPCC__) && !defined(EZPZ_QUANTILES_HOST_ONLY)

// ---- the kernels' arguments (filled by the host side: mc_quantiles.hip) ---------------------------------------------------------------
// A SELECTION is one distinct target rank of a record; a record has at most 4 n_q of them, kept in ascending rank, so their keys --
// and the prefixes of their keys -- ascend too.  A SLOT is one distinct prefix among a record's selections: the slots of a record
// are the runs of equal prefixes, in the same order.  The state arrays are [n_meas][kMaxSel].
struct SelectArgs {
    const double* m;       // [samples][n_meas]
    const uint8_t* flags;  // (NULL: every bit clear)
    const uint8_t* ok;     // (NULL: every one set)
    uint64_t samples;
    uint32_t n_meas, n_q;
    uint32_t pass;   // the digit: bits [56 - 8 pass, 64 - 8 pass) of the key
    uint32_t d_cap;  // the count kernel: the slots of a record counted in LDS; the others go to the global counters directly
    double probs[kMaxQ];
    double z;
    uint32_t* cnt;          // [n_meas][4 n_q][256]: a slot's keys by digit; all zero between passes
    uint64_t* sel_prefix;   // a selection's prefix: the top 8 pass bits of its key
    uint32_t* sel_r;        // ... and its rank among the valid keys that share the prefix
    uint64_t* slot_prefix;  // the record's distinct prefixes, ascending
    uint32_t* n_slot;       // [n_meas]
    uint32_t* n_sel;        // [n_meas]
    uint8_t* sel_of;        // the selection of rank c (k, k1, k_lo, k_hi) of probability q, at [4 q + c]
    uint64_t* n_valid;      // [n_meas]
    EzpzMcQuantile* out;    // [n_meas][n_q]
};

constexpr uint32_t kRows = 1024;       // samples per turn of a workgroup of the count kernel
constexpr uint32_t kLdsBytes = 65536;  // what a workgroup of the count kernel may take

// The LDS of the count kernel at a pass: the record's slot prefixes ([n_meas][4 n_q] uint64, pass > 0), the slot counts ([n_meas]) and
// the counters ([n_meas][d_cap][256]).  Pass 0 has one slot per record, the empty prefix.
inline uint32_t d_cap_of(uint32_t n_meas, uint32_t n_q, uint32_t pass) {
    const uint32_t fixed = (pass ? n_meas * 4 * n_q * 8 : 0) + n_meas * 4;
    return std::min<uint32_t>(pass ? 4 * n_q : 1, (kLdsBytes - fixed) / (n_meas * 1024));
}
inline uint32_t lds_bytes_of(uint32_t n_meas, uint32_t n_q, uint32_t pass) {
    return (pass ? n_meas * 4 * n_q * 8 : 0) + n_meas * 4 + n_meas * d_cap_of(n_meas, n_q, pass) * 1024;
}

#ifdef EZPZ_QUANTILES_KERNELS  // (mc_quantiles.hip alone: the kernels have one home)

// ---- a digit pass, first half: count -----------------------------------------------------------------------------------------------
// Workgroups take turns of kRows samples and walk them as the flat array they are -- thread t the elements t, t + 256, .. of the turn:
// a wavefront reads 64 consecutive doubles, whole rows.  A valid element whose key carries one of its record's slot prefixes (a binary
// search in LDS) counts in that slot under its digit: in LDS for the first d_cap slots, which the workgroup adds to the global
// counters when its turns are over, with integer atomics directly for the others.  Pass 0 counts every valid element: the counters
// of a record then sum to its n_valid.
__global__ __launch_bounds__(256) void mc_quantile_count_kernel(SelectArgs a) {
    extern __shared__ uint64_t s_mem[];
    const uint32_t t = threadIdx.x, M = a.n_meas, T = 4 * a.n_q, D = a.d_cap, pass = a.pass;
    uint64_t* s_pref = s_mem;
    uint32_t* s_nd = reinterpret_cast<uint32_t*>(s_mem + (pass ? M * T : 0));
    uint32_t* s_cnt = s_nd + M;
    for (uint32_t e = t; e < M; e += 256) s_nd[e] = pass ? a.n_slot[e] : 1u;
    __syncthreads();
    if (pass)
        for (uint32_t e = t; e < M * T; e += 256) {
            const uint32_t i = e / T, d = e - i * T;
            s_pref[e] = d < s_nd[i] ? a.slot_prefix[i * kMaxSel + d] : 0;
        }
    for (uint32_t e = t; e < M * D * 256; e += 256) s_cnt[e] = 0;
    __syncthreads();
    const uint32_t shift = 64 - 8 * pass;  // the bits below the prefix
    const uint64_t turns = (a.samples + kRows - 1) / kRows;
    for (uint64_t turn = blockIdx.x; turn < turns; turn += gridDim.x) {
        const uint64_t row0 = turn * kRows;
        const uint32_t rows = (uint32_t)(a.samples - row0 < kRows ? a.samples - row0 : kRows);
        const double* mp = a.m + row0 * M;
        const uint8_t* fp = a.flags ? a.flags + row0 * M : nullptr;
        const uint8_t* op = a.ok ? a.ok + row0 : nullptr;
        for (uint32_t e = t; e < rows * M; e += 256) {
            const uint32_t s = e / M, i = e - s * M;
            if (op && !op[s]) continue;
            if (fp && (fp[e] & 1u)) continue;
            const uint64_t bits = bits_of(mp[e]);
            if (!finite_bits(bits)) continue;
            const uint64_t key = key_of_bits(bits);
            uint32_t slot = 0;
            if (pass) {
                const uint64_t prefix = key >> shift;
                const uint64_t* list = s_pref + i * T;
                uint32_t lo = 0, hi = s_nd[i];  // the first slot whose prefix is not below the key's
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) / 2;
                    if (list[mid] < prefix)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (lo == s_nd[i] || list[lo] != prefix) continue;
                slot = lo;
            }
            const uint32_t digit = (uint32_t)(key >> (shift - 8)) & 255u;
            if (slot < D)
                atomicAdd(&s_cnt[(i * D + slot) * 256 + digit], 1u);
            else
                atomicAdd(&a.cnt[((uint64_t)i * T + slot) * 256 + digit], 1u);
        }
    }
    __syncthreads();
    for (uint32_t e = t; e < M * D * 256; e += 256) {
        const uint32_t v = s_cnt[e];
        if (!v) continue;
        const uint32_t i = e / (D * 256), rest = e - i * D * 256;  // rest = slot * 256 + digit
        atomicAdd(&a.cnt[(uint64_t)i * T * 256 + rest], v);
    }
}

// ---- a digit pass, second half: narrow ---------------------------------------------------------------------------------------------
// One workgroup per record, behind the count kernel on the stream.  Before pass 0's digit: n_valid from the counters, the ranks of
// every probability by ranks_of, sorted and made distinct into the record's selections.  Every pass: per slot, the inclusive scan of
// its 256 counters; the thread whose digit's range holds a selection's rank appends its digit to the selection's prefix and takes
// the keys below off the rank; the counters go back to zero; the slots are formed again from the new prefixes.  After the last
// digit a prefix is the key itself: record_of writes the outputs.
__global__ __launch_bounds__(256) void mc_quantile_narrow_kernel(SelectArgs a) {
    __shared__ uint32_t s_scan[2][256];
    __shared__ uint64_t s_pref[kMaxSel], s_new[kMaxSel], s_rank[kMaxSel];
    __shared__ uint32_t s_r[kMaxSel], s_newr[kMaxSel], s_slot[kMaxSel];
    __shared__ uint32_t s_nsel, s_nd;
    const uint32_t t = threadIdx.x, i = blockIdx.x, T = 4 * a.n_q, pass = a.pass;
    uint32_t* cnt = a.cnt + (uint64_t)i * T * 256;
    auto scan = [&](uint32_t c) {  // the inclusive scan of the 256 threads' c
        s_scan[0][t] = c;
        __syncthreads();
        uint32_t cur = 0;
        for (uint32_t off = 1; off < 256; off *= 2) {
            const uint32_t v = s_scan[cur][t] + (t >= off ? s_scan[cur][t - off] : 0u);
            s_scan[cur ^ 1u][t] = v;
            __syncthreads();
            cur ^= 1u;
        }
        const uint32_t incl = s_scan[cur][t];
        __syncthreads();
        return incl;
    };
    uint64_t n;
    if (pass == 0) {
        const uint32_t incl = scan(cnt[t]);
        if (t == 255) s_nsel = incl;  // (n_valid, for a moment)
        __syncthreads();
        n = s_nsel;
        __syncthreads();
        if (n && t < a.n_q) {
            const Ranks r = ranks_of(n, a.probs[t], a.z);
            s_rank[4 * t] = r.k, s_rank[4 * t + 1] = r.k1, s_rank[4 * t + 2] = r.k_lo, s_rank[4 * t + 3] = r.k_hi;
        }
        __syncthreads();
        if (t == 0) {
            a.n_valid[i] = n;
            uint32_t count = 0;  // s_pref, for a moment: the distinct ranks, ascending
            if (n)
                for (uint32_t e = 0; e < T; ++e) {
                    const uint64_t rank = s_rank[e];
                    uint32_t at = 0;
                    while (at < count && s_pref[at] < rank) ++at;
                    if (at < count && s_pref[at] == rank) continue;
                    for (uint32_t j = count; j > at; --j) s_pref[j] = s_pref[j - 1];
                    s_pref[at] = rank;
                    ++count;
                }
            for (uint32_t e = 0; n && e < T; ++e) {
                uint32_t at = 0;
                while (s_pref[at] != s_rank[e]) ++at;
                a.sel_of[i * kMaxSel + e] = (uint8_t)at;
            }
            for (uint32_t j = 0; j < count; ++j) s_r[j] = (uint32_t)s_pref[j], s_pref[j] = 0, s_slot[j] = 0;
            s_nsel = count;
            s_nd = count ? 1u : 0u;
        }
    } else {
        n = a.n_valid[i];
        const uint32_t count = a.n_sel[i];
        if (t < count) s_pref[t] = a.sel_prefix[i * kMaxSel + t], s_r[t] = a.sel_r[i * kMaxSel + t];
        __syncthreads();
        if (t == 0) {
            uint32_t d = 0;
            for (uint32_t j = 0; j < count; ++j) {
                if (j && s_pref[j] != s_pref[j - 1]) ++d;
                s_slot[j] = d;
            }
            s_nsel = count;
            s_nd = count ? d + 1 : 0u;
        }
    }
    __syncthreads();
    const uint32_t n_sel = s_nsel, n_d = s_nd;
    if (t < n_sel) s_new[t] = s_pref[t] << 8, s_newr[t] = 0;  // (every selection finds its digit below: its rank is below its slot's count)
    __syncthreads();
    for (uint32_t d = 0; d < n_d; ++d) {
        const uint32_t c = cnt[d * 256 + t];
        cnt[d * 256 + t] = 0;
        const uint32_t incl = scan(c), excl = incl - c;
        for (uint32_t j = 0; j < n_sel; ++j) {
            if (s_slot[j] != d) continue;
            const uint32_t r = s_r[j];
            if (excl <= r && r < incl) s_new[j] = (s_pref[j] << 8) | t, s_newr[j] = r - excl;
        }
        __syncthreads();
    }
    if (t < n_sel) a.sel_prefix[i * kMaxSel + t] = s_new[t], a.sel_r[i * kMaxSel + t] = s_newr[t];
    if (t == 0) {
        uint32_t d = 0;
        for (uint32_t j = 0; j < n_sel; ++j) {
            if (j && s_new[j] == s_new[j - 1]) continue;
            a.slot_prefix[i * kMaxSel + d++] = s_new[j];
        }
        a.n_slot[i] = d;
        a.n_sel[i] = n_sel;
    }
    if (pass == 7 && t < a.n_q) {
        EzpzMcQuantile q = empty_record();
        if (n) {
            const uint8_t* sel = a.sel_of + i * kMaxSel + 4 * t;
            q = record_of(n, ranks_of(n, a.probs[t], a.z), value_of_key(s_new[sel[0]]), value_of_key(s_new[sel[1]]),
                          value_of_key(s_new[sel[2]]), value_of_key(s_new[sel[3]]));
        }
        a.out[(size_t)i * a.n_q + t] = q;
    }
}

#endif  // EZPZ_QUANTILES_KERNELS

// ---- the host side (mc_quantiles.hip), shared with the run of tolerance_mc.hip -----------------------------------------------------
// The selection's workspace: whoever owns one orders the launches that use it (a LaunchOrder beside it) and waits for them before it
// grows.
struct SelectWork {
    DevBuf<uint32_t> cnt, sel_r, n_slot, n_sel;
    DevBuf<uint64_t> sel_prefix, slot_prefix, n_valid;
    DevBuf<uint8_t> sel_of;
    bool grows(uint32_t n_meas, uint32_t n_q) const { return (size_t)n_meas * 4 * n_q * 256 > cnt.cap || !sel_r.p; }
    int ensure(uint32_t n_meas, uint32_t n_q);
};
// the whole selection on rows that stay where they are until it has run: the counters' reset and eight digit passes of two launches.
// samples > 0, n_q > 0, the arguments checked; `cus`: the device's compute units
int enqueue_select(SelectWork& work, const double* m, const uint8_t* flags, const uint8_t* ok, uint64_t samples, uint32_t n_meas,
                   const double* probs, uint32_t n_q, double z, EzpzMcQuantile* out, uint32_t cus, hipStream_t stream);

#endif  // __HIPCC__ && !EZPZ_QUANTILES_HOST_ONLY

}  // namespace mcq
}  // namespace ezpz
