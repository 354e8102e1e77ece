// Redundancy analysis on the device: which constraints of a system are redundant, which conflict, and with whom.
//
// The row-space counterpart of FreedomAnalysis (freedom.hip.hpp works on the columns of the same matrix); a project extension,
// the reference has no such analysis.  The definition is above ezpz_system_redundancy in include/ezpz_amd.h: the rows of the
// weighted Jacobian are visited in request order, each one orthogonalised against the rows accepted so far by classical
// Gram-Schmidt applied twice (CGS2), the residual entry carried along as one more column; a row that keeps more than rank_tol of
// its length is INDEPENDENT, the others are REDUNDANT or -- what is left of their residual exceeds conflict_tol -- CONFLICTING.
// J is block diagonal over the components of freedom.hip: build_freedom, and ascending local row index is request order there,
// so the procedure runs per component.
//
// Workspace of one m x n component, doubles (pm = min(m, n), ld = n + 1, made odd where lanes share the matrix):
//   A[m][ld]  row-major; column n is the row's weighted residual.  The p-th accepted row is overwritten into row p (p <= i: that
//             row has been visited) as q_p with its companion s_p in column n, so the basis is the leading P rows
//   norm[m]   ||a_i|| | acc[pm] local row of the p-th accepted | h[pm] this pass's Q v | hs[pm] both passes' sum, then c = L^-T hs
//   Lt[pm][pm] only with conflict groups: the transposed factor of A_accepted = L Q, Lt(p, q) = L(q, p)
// Two layouts, one code body (redundancy_component<Ctx>), as in freedom.hip.hpp:
//   LANE  one lane per (system, component), private workspace interleaved in LDS, no synchronisation
//   TEAM  one workgroup (256 or 1024 lanes) per system, components in sequence, workspace in LDS or global memory.  h = Q v: one basis vector per lane
//         group (8 ... 64 lanes over the columns, folded by shuffles); v -= h^T Q: lanes over columns, basis vectors in sequence.
//         A row costs four sweeps of the basis and eight barriers, whatever the number of accepted rows.
// Every sum has a fixed order that depends on the component alone: the outputs do not depend on the batch or the place in it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch_types.hpp"

namespace ezpz {

constexpr uint32_t kNoFocus = 0xFFFFFFFFu;
constexpr uint8_t kRowIndependent = 0, kRowZero = 1, kRowRedundant = 2, kRowConflicting = 3;

struct RedundancyArgs {
    const double* jv;  // [batch][zj] weighted Jacobian values, internal slot order
    const double* r;   // [batch][n_rows] weighted residuals, internal row order
    const FreedomComp* comps;
    const uint32_t* items;
    const uint32_t* comp_row0;  // [ncomp] start of the component's rows in comp_rows
    const uint32_t* comp_rows;  // per component: the caller's (request-order) row of every local row
    const uint32_t* row_int;    // [n_rows] caller's row -> internal row (where r has it)
    const uint32_t* row_con;    // [n_rows] caller's row -> constraint position
    const uint32_t* con_row0;   // [n_cs + 1] first row of every constraint
    const double* row_w;        // [n_rows] weight of the row's constraint
    const uint32_t* focus_of;   // [n_cs] place in the focus list or kNoFocus; null without groups
    uint8_t* con_status;        // [batch][n_cs] out
    uint8_t* row_status;        // [batch][n_rows] out (the plan's scratch when the caller wants none)
    uint32_t* rank;             // [batch] out, may be null
    uint8_t* group;             // [batch][n_focus][n_cs] out, null without groups
    double* gws;                // TEAM: global workspace [gridDim][ws], null when the workspace is in LDS
    uint64_t batch;
    uint32_t n_rows, n_cs, zj, ncomp, n_focus;
    uint32_t ws;        // workspace doubles of the largest component
    uint32_t group_sz;  // LANE: systems per workgroup
    double rank_tol, conflict_tol, group_tol;
};

__global__ void __launch_bounds__(256) rd_gather_kernel(const double* x, const uint32_t* var_of, double* x_int, uint32_t n,
                                                        uint64_t total) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = i / n;
        const uint32_t k = (uint32_t)(i - b * n);
        x_int[i] = x[b * n + var_of[k]];
    }
}

namespace redundancy {

struct Ws {
    double* p;
    uint32_t stride;
    __device__ __forceinline__ double& operator()(uint32_t e) const { return p[(size_t)e * stride]; }
};

__host__ __device__ inline uint32_t row_stride(uint32_t n, bool shared) { return shared ? ((n + 1) | 1u) : n + 1; }
// (64-bit: the host refuses a component beyond 2^31 words)
__host__ __device__ inline uint64_t component_ws(uint32_t m, uint32_t n, bool shared, bool with_l) {
    const uint64_t pm = m < n ? m : n;
    return (uint64_t)m * row_stride(n, shared) + m + 3 * pm + (with_l ? pm * pm : 0);
}

struct LaneCtx {
    static constexpr bool kShared = false;
    __device__ __forceinline__ uint32_t id() const { return 0; }
    __device__ __forceinline__ uint32_t count() const { return 1; }
    __device__ __forceinline__ uint32_t gid() const { return 0; }
    __device__ __forceinline__ uint32_t groups() const { return 1; }
    __device__ __forceinline__ uint32_t glane() const { return 0; }
    __device__ __forceinline__ uint32_t gwidth() const { return 1; }
    __device__ __forceinline__ void sync() const {}
    __device__ __forceinline__ double sum(double v) const { return v; }
    __device__ __forceinline__ double gsum(double v) const { return v; }
};

struct BlockCtx {
    static constexpr bool kShared = true;
    double* red;  // LDS scratch, 16 doubles
    uint32_t gw;  // lanes per group: a power of two, 8 ... 64
    __device__ __forceinline__ uint32_t id() const { return threadIdx.x; }
    __device__ __forceinline__ uint32_t count() const { return blockDim.x; }
    __device__ __forceinline__ uint32_t gid() const { return threadIdx.x / gw; }
    __device__ __forceinline__ uint32_t groups() const { return blockDim.x / gw; }
    __device__ __forceinline__ uint32_t glane() const { return threadIdx.x & (gw - 1); }
    __device__ __forceinline__ uint32_t gwidth() const { return gw; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // every lane of the group gets the group's sum (the groups of a wavefront fold side by side; all their lanes are active)
    __device__ __forceinline__ double gsum(double v) const {
        for (uint32_t off = gw >> 1; off > 0; off >>= 1) v += __shfl_xor(v, (int)off);
        return v;
    }
    __device__ double sum(double v) const {
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (blockDim.x > 64) {
            const uint32_t nw = blockDim.x >> 6;
            __syncthreads();
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
            __syncthreads();
            v = 0.0;
            for (uint32_t w = 0; w < nw; ++w) v += red[w];
        }
        return v;
    }
};

// `rows`: the component's caller rows; `row_status` / `group`: this system's.  Every lane of the context takes every branch.
template <class C>
__device__ void redundancy_component(const C& ctx, const Ws W, const FreedomComp cd, const RedundancyArgs& a,
                                     const uint32_t* __restrict__ rows, const double* __restrict__ jv, const double* __restrict__ r,
                                     uint8_t* __restrict__ row_status, uint8_t* __restrict__ group) {
    const uint32_t m = cd.m, n = cd.n, ld = row_stride(n, C::kShared), pm = m < n ? m : n;
    const uint32_t oNorm = m * ld, oAcc = oNorm + m, oH = oAcc + pm, oHs = oH + pm, oLt = oHs + pm;
    const uint32_t id = ctx.id(), cnt = ctx.count();
#define A_(i, j) W((i) * ld + (j))
    for (uint32_t e = id; e < m * ld; e += cnt) W(e) = 0.0;
    ctx.sync();
    for (uint32_t it = cd.item0 + id; it < cd.item1; it += cnt) {
        const uint32_t e = a.items[2 * it + 1];  // lcol * m + lrow
        const uint32_t lcol = e / m;
        A_(e - lcol * m, lcol) = jv[a.items[2 * it]];
    }
    for (uint32_t i = id; i < m; i += cnt) A_(i, n) = r[a.row_int[rows[i]]];
    ctx.sync();
    for (uint32_t i = ctx.gid(); i < m; i += ctx.groups()) {  // ||a_i||, a lane group per row
        double s = 0.0;
        for (uint32_t j = ctx.glane(); j < n; j += ctx.gwidth()) {
            const double v = A_(i, j);
            s += v * v;
        }
        s = ctx.gsum(s);
        if (ctx.glane() == 0) W(oNorm + i) = sqrt(s);
    }
    ctx.sync();
    uint32_t P = 0;  // accepted rows = the basis in rows 0 .. P-1
    for (uint32_t i = 0; i < m; ++i) {
        const double na = W(oNorm + i);
        if (na == 0.0) {  // a guard fired, or nothing depends on the row at x
            if (id == 0) row_status[rows[i]] = kRowZero;
            continue;
        }
        double sq = 0.0;
        for (uint32_t pass = 0; pass < 2; ++pass) {
            for (uint32_t p = ctx.gid(); p < P; p += ctx.groups()) {  // h = Q v
                double s = 0.0;
                for (uint32_t j = ctx.glane(); j < n; j += ctx.gwidth()) s += A_(p, j) * A_(i, j);
                s = ctx.gsum(s);
                if (ctx.glane() == 0) {
                    W(oH + p) = s;
                    W(oHs + p) = pass ? W(oHs + p) + s : s;
                }
            }
            ctx.sync();
            for (uint32_t j = id; j <= n; j += cnt) {  // v -= h^T Q, and rho -= h . s in column n
                double v = A_(i, j);
                uint32_t p = 0;
                // (the basis vectors in sequence, eight loads in flight: a lane of a large component waits for global memory here)
                for (; p + 8 <= P; p += 8) {
                    double q[8], h[8];
#pragma unroll
                    for (uint32_t u = 0; u < 8; ++u) q[u] = A_(p + u, j), h[u] = W(oH + p + u);
#pragma unroll
                    for (uint32_t u = 0; u < 8; ++u) v -= h[u] * q[u];
                }
                for (; p < P; ++p) v -= W(oH + p) * A_(p, j);
                A_(i, j) = v;
                if (pass && j < n) sq += v * v;
            }
            ctx.sync();
        }
        const double nv = sqrt(ctx.sum(sq));
        if (nv / na > a.rank_tol && P < pm) {  // (a basis of n rows spans every row: whatever is left then is rounding)
            for (uint32_t j = id; j <= n; j += cnt) A_(P, j) = A_(i, j) / nv;  // (P == i: in place, a lane's own entries)
            if (group) {
                for (uint32_t p = id; p < P; p += cnt) W(oLt + p * pm + P) = W(oHs + p);
                if (id == 0) W(oLt + P * pm + P) = nv;
            }
            if (id == 0) {
                W(oAcc + P) = (double)i;
                row_status[rows[i]] = kRowIndependent;
            }
            ++P;
        } else {
            const uint32_t row = rows[i], con = a.row_con[row];
            const bool conflicting = fabs(A_(i, n)) / a.row_w[row] > a.conflict_tol;
            if (id == 0) row_status[row] = conflicting ? kRowConflicting : kRowRedundant;
            const uint32_t k = group ? a.focus_of[con] : kNoFocus;
            if (k != kNoFocus) {  // a_i = sum_p c_p a_(acc p), c = L^-T hs (in place, last first)
                for (uint32_t p = P; p-- > 0;) {
                    double dot = 0.0;
                    for (uint32_t q = p + 1 + id; q < P; q += cnt) dot += W(oLt + p * pm + q) * W(oHs + q);
                    dot = ctx.sum(dot);
                    if (id == 0) W(oHs + p) = (W(oHs + p) - dot) / W(oLt + p * pm + p);
                    ctx.sync();
                }
                uint8_t* g = group + (size_t)k * a.n_cs;
                for (uint32_t p = id; p < P; p += cnt) {
                    const uint32_t lr = (uint32_t)W(oAcc + p);
                    if (fabs(W(oHs + p)) * W(oNorm + lr) > a.group_tol * na) g[a.row_con[rows[lr]]] = 1;
                }
                if (id == 0) g[con] = 1;
            }
        }
        ctx.sync();
    }
#undef A_
}

}  // namespace redundancy

// TEAM: 256 lanes, or 1024 where a component has more than 64 variables (sixteen basis vectors per sweep of h = Q v instead of four)
template <bool LANE>
__global__ void __launch_bounds__(LANE ? 256 : 1024) redundancy_kernel(const RedundancyArgs a) {
    using namespace redundancy;
    extern __shared__ double rd_lds[];
    const uint32_t G = LANE ? a.group_sz : 1;
    uint32_t* rankc = reinterpret_cast<uint32_t*>(rd_lds);  // [G] independent rows per system (rounded up to doubles)
    double* red = rd_lds + (G + 1) / 2;
    double* wsl = red + 16;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const size_t per_group = (size_t)a.n_focus * a.n_cs;
    for (uint64_t base = (uint64_t)blockIdx.x * G; base < a.batch; base += (uint64_t)gridDim.x * G) {
        const uint32_t nsys = (uint32_t)((a.batch - base) < G ? (a.batch - base) : G);
        // a row in no component has no entries: ZERO
        for (uint32_t idx = tid; idx < nsys * a.n_rows; idx += nthr) a.row_status[base * a.n_rows + idx] = kRowZero;
        if (a.group)
            for (size_t idx = tid; idx < nsys * per_group; idx += nthr) a.group[base * per_group + idx] = 0;
        for (uint32_t g = tid; g < G; g += nthr) rankc[g] = 0;
        __threadfence_block();
        __syncthreads();
        if (LANE) {
            for (uint32_t item = tid; item < nsys * a.ncomp; item += nthr) {
                const uint32_t g = item / a.ncomp, c = item - g * a.ncomp;
                redundancy_component(LaneCtx{}, Ws{wsl + tid, nthr}, a.comps[c], a, a.comp_rows + a.comp_row0[c],
                                     a.jv + (base + g) * a.zj, a.r + (base + g) * a.n_rows, a.row_status + (base + g) * a.n_rows,
                                     a.group ? a.group + (base + g) * per_group : nullptr);
            }
        } else {
            double* w = a.gws ? a.gws + (size_t)blockIdx.x * a.ws : wsl;
            for (uint32_t c = 0; c < a.ncomp; ++c) {
                const FreedomComp cd = a.comps[c];
                const uint32_t gw = cd.n > 32 ? 64 : cd.n > 16 ? 32 : cd.n > 8 ? 16 : 8;
                redundancy_component(BlockCtx{red, gw}, Ws{w, 1}, cd, a, a.comp_rows + a.comp_row0[c], a.jv + base * a.zj,
                                     a.r + base * a.n_rows, a.row_status + base * a.n_rows, a.group ? a.group + base * per_group : nullptr);
            }
        }
        __threadfence_block();
        __syncthreads();
        for (uint32_t idx = tid; idx < nsys * a.n_cs; idx += nthr) {  // a constraint's status: the maximum over its rows
            const uint32_t g = idx / a.n_cs, c = idx - g * a.n_cs;
            const uint8_t* rs = a.row_status + (base + g) * a.n_rows;
            uint8_t st = 0;
            uint32_t indep = 0;
            for (uint32_t row = a.con_row0[c]; row < a.con_row0[c + 1]; ++row) {
                const uint8_t s = rs[row];
                st = s > st ? s : st;
                indep += s == kRowIndependent ? 1u : 0u;
            }
            a.con_status[(base + g) * a.n_cs + c] = st;
            if (indep) atomicAdd(&rankc[g], indep);
        }
        __syncthreads();
        if (a.rank)
            for (uint32_t g = tid; g < nsys; g += nthr) a.rank[base + g] = rankc[g];
        __syncthreads();
    }
}

}  // namespace ezpz
