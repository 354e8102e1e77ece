// Dimension targets (include/ezpz_amd.h: ezpz_seek_step, ezpz_system_seek_targets[_device]): the step of the projected
// Levenberg-Marquardt iteration -- ONE __host__ __device__ body, written for a lane of a team that owns column r of the normal
// matrix, behind the host entry (HostTeam: the lanes' values side by side, an operation at a time) and the kernel (LaneTeam: a
// lane's value in a register, other lanes' values by cross-lane moves) -- and the two kernels of a round: seek_step_kernel (verdict,
// bookkeeping, the next step) and seek_commit_kernel (the accepted rows of x).  The host plan and the entries are in seek.hip.
//
// Built without contraction (build.py: -ffp-contract=off for every unit) and from + - * /, comparisons and fabs alone: the step is
// the same bits on both sides.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ezpz_amd.h"

namespace ezpz {
namespace seek {

#define EZPZ_SEEK_HD __host__ __device__ inline

constexpr uint32_t kActive = 0xFFFFFFFFu;  // EzpzSeekInfo.status of a system that is not finished: never left behind by a run
constexpr double kTiny = 1e-300, kFloor = 1e-2, kMaxFinite = 1.7976931348623157e308;

EZPZ_SEEK_HD bool finite_d(double v) { return fabs(v) <= kMaxFinite; }

// ---- the host's team: T lanes' values side by side -----------------------------------------------------------------------------------
template <int T_>
struct HostTeam {
    static constexpr int T = T_;
    struct V {
        double v[T_];
    };
    using B = uint32_t;  // bit r: lane r
    static V splat(double a) {
        V o;
        for (int r = 0; r < T; ++r) o.v[r] = a;
        return o;
    }
    static V load(const double* row, uint32_t n) {  // lane r: row[r], +0.0 past n
        V o;
        for (int r = 0; r < T; ++r) o.v[r] = (uint32_t)r < n ? row[r] : 0.0;
        return o;
    }
    static double get(const V& a, int k) { return a.v[k]; }
#define EZPZ_SEEK_HOST_OP(name, expr)      \
    static V name(const V& a, const V& b) { \
        V o;                               \
        for (int r = 0; r < T; ++r) o.v[r] = expr; \
        return o;                          \
    }
    EZPZ_SEEK_HOST_OP(add, a.v[r] + b.v[r])
    EZPZ_SEEK_HOST_OP(sub, a.v[r] - b.v[r])
    EZPZ_SEEK_HOST_OP(mul, a.v[r] * b.v[r])
    EZPZ_SEEK_HOST_OP(div, a.v[r] / b.v[r])
#undef EZPZ_SEEK_HOST_OP
    static V abs(const V& a) {
        V o;
        for (int r = 0; r < T; ++r) o.v[r] = fabs(a.v[r]);
        return o;
    }
#define EZPZ_SEEK_HOST_CMP(name, op)       \
    static B name(const V& a, const V& b) { \
        B o = 0;                           \
        for (int r = 0; r < T; ++r) o |= (a.v[r] op b.v[r]) ? 1u << r : 0u; \
        return o;                          \
    }
    EZPZ_SEEK_HOST_CMP(lt, <)
    EZPZ_SEEK_HOST_CMP(gt, >)
    EZPZ_SEEK_HOST_CMP(le, <=)
    EZPZ_SEEK_HOST_CMP(eq, ==)
    EZPZ_SEEK_HOST_CMP(ne, !=)
#undef EZPZ_SEEK_HOST_CMP
    static B not_(B a) { return ~a & ((1u << T) - 1u); }
    static B lane_is(int k) { return 1u << k; }
    static B lane_gt(int k) { return ~((2u << k) - 1u) & ((1u << T) - 1u); }
    static B lane_lt(int k) { return (1u << k) - 1u; }
    static V sel(B c, const V& a, const V& b) {
        V o;
        for (int r = 0; r < T; ++r) o.v[r] = (c >> r) & 1u ? a.v[r] : b.v[r];
        return o;
    }
    static uint32_t mask(B a) { return a; }
    static void store(double* row, uint32_t n, const V& a) {
        for (int r = 0; r < T && (uint32_t)r < n; ++r) row[r] = a.v[r];
    }
};

// What STEP gives: the kind (EZPZ_SEEK_STEP_*) and the held dimensions are the team's; p_trial and delta are a lane's.
template <class TM>
struct StepOut {
    int kind;
    uint32_t held;
    typename TM::V p_trial, delta;
};

// The normal matrix's column and the gradient's entry of every lane: colA[c] = A[c][r] (= A[r][c], bit for bit), g = g[r].
// D [n_meas][n_param] as the response entry writes it; lanes past n_param hold zeros.
template <class TM>
struct Normal {
    typename TM::V colA[TM::T], g;
};

template <class TM>
EZPZ_SEEK_HD void normal(uint32_t n_param, uint32_t n_meas, const double* m, const double* D, const double* targets, const double* weight,
                         const typename TM::V& scale, Normal<TM>& N) {
    using V = typename TM::V;
    for (int c = 0; c < TM::T; ++c) N.colA[c] = TM::splat(0.0);
    N.g = TM::splat(0.0);
    for (uint32_t i = 0; i < n_meas; ++i) {
        const double w = weight[i], e = w * (targets[i] - m[i]);
        const V dp = TM::mul(TM::mul(TM::splat(w), TM::load(D + (size_t)i * n_param, n_param)), scale);
#pragma unroll
        for (int c = 0; c < TM::T; ++c) N.colA[c] = TM::add(N.colA[c], TM::mul(dp, TM::splat(TM::get(dp, c))));
        N.g = TM::add(N.g, TM::mul(dp, TM::splat(e)));
    }
}

// STEP of include/ezpz_amd.h from the normal matrix: lanes past n_param pass lo == hi (held).
template <class TM>
EZPZ_SEEK_HD void step(const Normal<TM>& N, const typename TM::V& p, const typename TM::V& lo, const typename TM::V& hi,
                       const typename TM::V& scale, double mu, double step_tol, StepOut<TM>& out) {
    using V = typename TM::V;
    using B = typename TM::B;
    constexpr int T = TM::T;
    const V zero = TM::splat(0.0);
    const B held = TM::eq(lo, hi) | (TM::eq(p, lo) & TM::lt(N.g, zero)) | (TM::eq(p, hi) & TM::gt(N.g, zero));
    const B fr = TM::not_(held);
    const uint32_t freem = TM::mask(fr);
    out.held = TM::mask(held);
    out.p_trial = p;
    out.delta = zero;
    if (freem == 0) {
        out.kind = EZPZ_SEEK_STEP_MINIMUM;
        return;
    }
    V diag = zero;
#pragma unroll
    for (int c = 0; c < T; ++c) diag = TM::sel(TM::lane_is(c), N.colA[c], diag);
    double amax = 0.0;
#pragma unroll
    for (int k = 0; k < T; ++k) {
        const double a = TM::get(diag, k);
        if (((freem >> k) & 1u) && a > amax) amax = a;
    }
    double f = kFloor * amax;
    if (f < kTiny) f = kTiny;
    const V fv = TM::splat(f);
    const V dd = TM::add(diag, TM::mul(TM::splat(mu), TM::sel(TM::gt(diag, fv), diag, fv)));
    V colM[T];
#pragma unroll
    for (int c = 0; c < T; ++c) colM[c] = TM::sel(TM::lane_is(c), dd, N.colA[c]);
    // M = L diag(d) L^T: lane j keeps M[i][j] for every i, both triangles with the same bits
    bool pivot_ok = true;
#pragma unroll
    for (int k = 0; k < T; ++k) {
        if (!((freem >> k) & 1u) || !pivot_ok) continue;
        const double dk = TM::get(colM[k], k);
        if (!(dk > 0.0) || !finite_d(dk)) {
            pivot_ok = false;
            continue;
        }
        const V dkv = TM::splat(dk);
        const B upd = fr & TM::lane_gt(k);
#pragma unroll
        for (int i = k + 1; i < T; ++i) {
            if (!((freem >> i) & 1u)) continue;
            const double mik = TM::get(colM[i], k);
            colM[i] = TM::sel(upd, TM::sub(colM[i], TM::div(TM::mul(TM::splat(mik), colM[k]), dkv)), colM[i]);
        }
    }
    if (!pivot_ok) {
        out.kind = EZPZ_SEEK_STEP_PIVOT;
        return;
    }
    V dg = TM::splat(1.0);  // (a held lane divides by one)
#pragma unroll
    for (int c = 0; c < T; ++c) dg = TM::sel(TM::lane_is(c) & fr, colM[c], dg);
    V y = TM::sel(fr, N.g, zero);
#pragma unroll
    for (int k = 0; k < T; ++k) {
        if (!((freem >> k) & 1u)) continue;
        const double yk = TM::get(y, k), dk = TM::get(dg, k);
        y = TM::sel(fr & TM::lane_gt(k), TM::sub(y, TM::mul(TM::div(colM[k], TM::splat(dk)), TM::splat(yk))), y);
    }
    V v = TM::sel(fr, TM::div(y, dg), zero);
#pragma unroll
    for (int i = T - 1; i >= 1; --i) {
        if (!((freem >> i) & 1u)) continue;
        const double vi = TM::get(v, i);
        v = TM::sel(fr & TM::lane_lt(i), TM::sub(v, TM::mul(TM::div(colM[i], dg), TM::splat(vi))), v);
    }
    if (TM::mask(fr & TM::not_(TM::le(TM::abs(v), TM::splat(kMaxFinite))))) {
        out.kind = EZPZ_SEEK_STEP_PIVOT;
        return;
    }
    const V delta = TM::sel(fr, TM::mul(scale, v), zero);
    const V q = TM::add(p, delta);
    const V pt = TM::sel(fr, TM::sel(TM::lt(q, lo), lo, TM::sel(TM::gt(q, hi), hi, q)), p);
    out.delta = delta;
    out.p_trial = pt;
    const V bar = TM::mul(TM::splat(step_tol), TM::add(TM::abs(p), TM::splat(step_tol)));
    const bool small = TM::mask(fr & TM::not_(TM::le(TM::abs(delta), bar))) == 0;
    const bool same = TM::mask(TM::ne(pt, p)) == 0;
    out.kind = small || same ? EZPZ_SEEK_STEP_MINIMUM : EZPZ_SEEK_STEP_TRIAL;
}

// ezpz_seek_step behind its argument check (seek.hip; tools/asan_seek_step.cpp drives it under the sanitizers): the arrays of cfg
// are set, n_param in 1 .. 16.
template <int T>
inline int step_host_team(uint32_t n_param, uint32_t n_meas, const double* p, const double* m, const double* D, const double* targets,
                          const double* weight, const double* lo, const double* hi, const double* scale, double mu, double step_tol,
                          double* p_trial_out, double* delta_out, uint32_t* held_out) {
    using TM = HostTeam<T>;
    const typename TM::V sv = TM::sel((1u << n_param) - 1u, TM::load(scale, n_param), TM::splat(1.0));
    Normal<TM> N;
    normal<TM>(n_param, n_meas, m, D, targets, weight, sv, N);
    StepOut<TM> out;
    step<TM>(N, TM::load(p, n_param), TM::load(lo, n_param), TM::load(hi, n_param), sv, mu, step_tol, out);
    TM::store(p_trial_out, n_param, out.p_trial);
    TM::store(delta_out, n_param, out.delta);
    if (held_out) *held_out = out.held & ((1u << n_param) - 1u);
    return out.kind;
}
inline int step_host(uint32_t n_param, uint32_t n_meas, const double* p, const double* m, const double* D, const double* targets,
                     const double* weight, const double* lo, const double* hi, const double* scale, double mu, double step_tol,
                     double* p_trial_out, double* delta_out, uint32_t* held_out) {
    // (the team of the kernel for this n_param: the lanes past n_param are held, so every team gives the same bits)
    if (n_param <= 4) return step_host_team<4>(n_param, n_meas, p, m, D, targets, weight, lo, hi, scale, mu, step_tol, p_trial_out, delta_out, held_out);
    if (n_param <= 8) return step_host_team<8>(n_param, n_meas, p, m, D, targets, weight, lo, hi, scale, mu, step_tol, p_trial_out, delta_out, held_out);
    return step_host_team<16>(n_param, n_meas, p, m, D, targets, weight, lo, hi, scale, mu, step_tol, p_trial_out, delta_out, held_out);
}

// (EZPZ_SEEK_HOST_ONLY: a host program that wants the step alone -- tools/asan_seek_step.cpp -- leaves the kernels out)
#if defined(__HIPCC__) && !defined(EZPZ_SEEK_HOST_ONLY)

// ---- the kernel's team: T consecutive lanes of a wavefront, a lane's value in a register --------------------------------------------
template <int T_>
struct LaneTeam {
    static constexpr int T = T_;
    using V = double;
    using B = bool;
    static __device__ inline int lane() { return (int)(threadIdx.x & (T_ - 1)); }
    static __device__ inline V splat(double a) { return a; }
    static __device__ inline V load(const double* row, uint32_t n) { return (uint32_t)lane() < n ? row[lane()] : 0.0; }
    static __device__ inline double get(V a, int k) { return __shfl(a, k, T_); }  // (lane k of the caller's team)
    static __device__ inline V add(V a, V b) { return a + b; }
    static __device__ inline V sub(V a, V b) { return a - b; }
    static __device__ inline V mul(V a, V b) { return a * b; }
    static __device__ inline V div(V a, V b) { return a / b; }
    static __device__ inline V abs(V a) { return fabs(a); }
    static __device__ inline B lt(V a, V b) { return a < b; }
    static __device__ inline B gt(V a, V b) { return a > b; }
    static __device__ inline B le(V a, V b) { return a <= b; }
    static __device__ inline B eq(V a, V b) { return a == b; }
    static __device__ inline B ne(V a, V b) { return a != b; }
    static __device__ inline B not_(B a) { return !a; }
    static __device__ inline B lane_is(int k) { return lane() == k; }
    static __device__ inline B lane_gt(int k) { return lane() > k; }
    static __device__ inline B lane_lt(int k) { return lane() < k; }
    static __device__ inline V sel(B c, V a, V b) { return c ? a : b; }
    static __device__ inline uint32_t mask(B a) {  // the team's lanes with `a`, lane 0 of the team in bit 0
        const unsigned long long all = __ballot(a);
        return (uint32_t)(all >> ((threadIdx.x & 63u) & ~(uint32_t)(T_ - 1))) & ((1u << T_) - 1u);
    }
};

// ---- verdict, bookkeeping and the next step: one team per system -----------------------------------------------------------------------
struct StepArgs {
    // the round's evaluation: what the four entries wrote
    const EzpzStatus* solve_status;  // [count]
    const uint32_t* sens_status;     // [count]
    const double* m_trial;           // [count][n_meas]
    const uint8_t* flags;            // [count][n_meas]
    const double* D_trial;           // [count][n_meas][n_param]
    // the request
    const double* targets;                         // [count][n_meas]
    const double *weight, *tol, *lo, *hi, *scale;  // the tables
    // the state: the last commit
    double* p;          // [count][n_param]: params_out
    double* m;          // [count][n_meas]: m_out
    double* D;          // [count][n_meas][n_param]
    EzpzSeekInfo* info;  // [count]
    double* trace;      // [count][1 + max_iterations], optional
    // what the next round reads
    double* p_trial;          // [count][n_param]
    uint8_t* verdict;         // [count]: 1 = this round's x is committed
    unsigned int* active;     // [rounds]: the unfinished systems after each round (one integer atomic per workgroup)
    uint32_t count, n_param, n_meas, round, max_iterations;
    double mu0, mu_up, mu_down, mu_min, mu_max, step_tol;
};

__device__ inline double seek_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

template <int T>
__global__ __launch_bounds__(256) void seek_step_kernel(StepArgs a) {
    using TM = LaneTeam<T>;
    __shared__ unsigned int s_active;
    if (threadIdx.x == 0) s_active = 0;
    __syncthreads();
    const uint32_t r = (uint32_t)TM::lane(), n_param = a.n_param, n_meas = a.n_meas;
    const uint64_t b = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / T;
    const bool live = b < a.count;
    const uint64_t bs = live ? b : 0;  // (a team past the batch walks system 0 and writes nothing)
    const bool mine = r < n_param;
    EzpzSeekInfo info = a.info[bs];
    if (a.round == 0) {
        info.status = kActive, info.iterations = info.accepted = info.rejected = 0;
        info.cost0 = info.cost = info.worst = seek_nan();
        info.mu = a.mu0;
    }
    const bool was_active = live && info.status == kActive;
    const double* targets = a.targets + bs * n_meas;
    const double* m_t = a.m_trial + bs * n_meas;
    const double* D_t = a.D_trial + bs * n_meas * n_param;
    double* m_c = a.m + bs * n_meas;
    double* D_c = a.D + bs * n_meas * n_param;
    double* trace = a.trace ? a.trace + bs * (a.max_iterations + 1) : nullptr;
    // ---- the verdict on the round's evaluation ----
    const EzpzStatus st = a.solve_status[bs];
    bool good = st.converged != 0 && st.n_unsatisfied == 0 && a.sens_status[bs] == 0;
    bool bad_d = false, reached = true;
    double cost = 0.0, worst = 0.0;
    for (uint32_t i = 0; i < n_meas; ++i) {
        const double w = a.weight[i], mt = m_t[i], dev = targets[i] - mt, e = w * dev, ad = fabs(dev);
        if ((w > 0.0 && (a.flags[bs * n_meas + i] & 1u)) || !finite_d(mt)) good = false;
        if (mine && !finite_d(D_t[(size_t)i * n_param + r])) bad_d = true;
        cost = cost + e * e;
        if (w > 0.0 && ad > worst) worst = ad;
        if (w > 0.0 && !(ad <= a.tol[i])) reached = false;
    }
    if (TM::mask(bad_d)) good = false;
    const bool accept = was_active && good && (a.round == 0 || cost < info.cost);
    bool stalled = false;
    if (was_active) {
        if (accept) {
            info.cost = cost, info.worst = worst;
            if (a.round == 0) {
                info.cost0 = cost;
            } else {
                info.accepted += 1;
                info.mu = info.mu * a.mu_down;
                if (info.mu < a.mu_min) info.mu = a.mu_min;
            }
            if (reached) info.status = EZPZ_SEEK_REACHED;
            if (mine) a.p[bs * n_param + r] = a.p_trial[bs * n_param + r];
            for (uint32_t i = r; i < n_meas; i += T) m_c[i] = m_t[i];
            if (mine)
                for (uint32_t i = 0; i < n_meas; ++i) D_c[(size_t)i * n_param + r] = D_t[(size_t)i * n_param + r];
        } else if (a.round == 0) {
            info.status = EZPZ_SEEK_START_FAILED;
            for (uint32_t i = r; i < n_meas; i += T) m_c[i] = seek_nan();
        } else {
            info.rejected += 1;
            if (info.mu >= a.mu_max) {
                stalled = true;
            } else {
                info.mu = info.mu * a.mu_up;
                if (info.mu > a.mu_max) info.mu = a.mu_max;
            }
        }
        if (trace) {
            if (a.round == 0)
                for (uint32_t k = r; k <= a.max_iterations; k += T) trace[k] = k == 0 ? info.cost0 : seek_nan();
            else if (r == 0)
                trace[info.iterations] = info.cost;
        }
    }
    // ---- the next step, from the last commit: this round's evaluation where it was accepted, the kept one elsewhere ----
    bool stepping = was_active && info.status == kActive;
    const double* m_s = accept ? m_t : m_c;
    const double* D_s = accept ? D_t : D_c;
    const double scale_r = mine ? a.scale[r] : 1.0;
    const double lo_r = mine ? a.lo[r] : 0.0, hi_r = mine ? a.hi[r] : 0.0;
    const double p_r = mine ? (accept ? a.p_trial[bs * n_param + r] : a.p[bs * n_param + r]) : 0.0;
    Normal<TM> N;
    normal<TM>(n_param, n_meas, m_s, D_s, targets, a.weight, scale_r, N);
    // (a failed pivot is an iteration without a trial: the loop runs while any team of the wavefront has one to repeat)
    while (__any(stepping)) {
        StepOut<TM> out;
        step<TM>(N, p_r, lo_r, hi_r, scale_r, info.mu, a.step_tol, out);
        if (stepping) {
            if (out.kind == EZPZ_SEEK_STEP_MINIMUM) {
                info.status = EZPZ_SEEK_MINIMUM;
            } else if (stalled) {
                info.status = EZPZ_SEEK_STALLED;
            } else if (info.iterations == a.max_iterations) {
                info.status = EZPZ_SEEK_ITERATIONS;
            } else {
                info.iterations += 1;
                if (out.kind == EZPZ_SEEK_STEP_PIVOT) {
                    info.rejected += 1;
                    if (info.mu >= a.mu_max) {
                        stalled = true;
                    } else {
                        info.mu = info.mu * a.mu_up;
                        if (info.mu > a.mu_max) info.mu = a.mu_max;
                    }
                    if (trace && r == 0) trace[info.iterations] = info.cost;
                    continue;
                }
                if (mine) a.p_trial[bs * n_param + r] = out.p_trial;
            }
            stepping = false;
        }
    }
    if (was_active && r == 0) {
        a.info[bs] = info;
        if (info.status == kActive) atomicAdd(&s_active, 1u);
    }
    if (live && r == 0) a.verdict[bs] = accept ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0 && s_active) atomicAdd(a.active + a.round, s_active);
}

// ---- p_trial = p = clamp(params0) before round 0 ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seek_start_kernel(const double* __restrict__ params0, const double* __restrict__ lo,
                                                         const double* __restrict__ hi, uint32_t n_param, uint64_t count,
                                                         double* __restrict__ p, double* __restrict__ p_trial) {
    const uint64_t total = count * n_param, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const uint32_t r = (uint32_t)(idx % n_param);
        const double v = params0[idx], c = v < lo[r] ? lo[r] : v > hi[r] ? hi[r] : v;
        p[idx] = c;
        p_trial[idx] = c;
    }
}

// ---- x_best[b] = x_trial[b] where the round's verdict says so: a wavefront per row, 16 bytes per lane where both rows allow --------
__global__ __launch_bounds__(256) void seek_commit_kernel(const uint8_t* __restrict__ verdict, const double* __restrict__ x_trial,
                                                          double* __restrict__ x_best, uint32_t n_vars, uint64_t count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    const bool wide = (n_vars & 1u) == 0 && (((uintptr_t)x_trial | (uintptr_t)x_best) & 15u) == 0;
    for (uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < count; b += waves) {
        if (!verdict[b]) continue;
        const double* src = x_trial + b * n_vars;
        double* dst = x_best + b * n_vars;
        if (wide) {
            const double2* s2 = reinterpret_cast<const double2*>(src);
            double2* d2 = reinterpret_cast<double2*>(dst);
            for (uint32_t k = lane; k < n_vars / 2; k += 64) d2[k] = s2[k];
        } else {
            for (uint32_t k = lane; k < n_vars; k += 64) dst[k] = src[k];
        }
    }
}

#endif  // __HIPCC__ && !EZPZ_SEEK_HOST_ONLY

}  // namespace seek
}  // namespace ezpz
