// Dimension sensitivities (include/ezpz_amd.h: ezpz_system_param_sensitivity*):
//     S_b[j, :] = -(JtJ + lambda I)^-1 Jt g_j      for every system b of a batch and every driven parameter j.
// JtJ + lambda I is block diagonal over the connected components of the variable-constraint graph, and a parameter moves only
// its own component: the host plans per component (sensitivity.hip) and only components that hold a driven constraint are
// evaluated.  S is zeroed before the kernels run (whole lines, by the runtime's fill), so they write component entries only.
//
// Two shapes, both with every sum in a fixed order (same bits whatever the batch and a system's place in it):
//   sens_small_kernel   components of <= kSensSmallVars variables: one LANE per (system, component).  A workgroup is 64
//                       consecutive systems of one component, so the records and every branch are uniform across the
//                       wavefront; a lane's few dozen values (x, the record's partials, the packed factor, one right-hand
//                       side) sit in LDS, lane-interleaved (conflict free; only the record's small index arrays go to scratch).
//   sens_block_kernel   larger components: one WORKGROUP per (system, component), persistent over the work items.  Lanes gather x
//                       and the parameter row, evaluate J (con_jacobian, one record per lane) and g (con_dparam), build the
//                       ROW ENVELOPE of JtJ + lambda I from per-entry product lists the host made (the order of a list is the
//                       caller's constraint order), factorise it column by column (left-looking Cholesky: a lane per row of the
//                       column, two barriers a column), then take one right-hand side per lane through the forward and
//                       backward substitutions, in place in that parameter's row of S.  The envelope is of the better of the
//                       caller's variable order and reverse Cuthill-McKee: a chain-like sketch of 300 variables keeps ~4
//                       entries a row (the dense triangle, 361 KB, would not fit LDS; its envelope is ~10 KB).
//                       <false>: partials and factor in LDS.  <true>: in a global-memory workspace per resident workgroup
//                       (the idea of lm_kernel.hip.hpp's WsRef: same code, another base), for envelopes beyond the LDS budget,
//                       up to the dense triangle of EZPZ_SENSITIVITY_MAX_COMPONENT_VARS variables.
//   sens_finish_kernel  a system with a failed pivot (status 1) gets its whole S filled with NaN.
#pragma once
#include <hip/hip_runtime.h>

#include "constraint_dparam.hip.hpp"
#include "constraint_eval.hip.hpp"

namespace ezpz {

constexpr uint32_t kSensSmallVars = 8;
constexpr uint32_t kSensSmallLane = 16 + kSensSmallVars * 2 + kSensSmallVars * (kSensSmallVars + 1) / 2;  // partials | x | rhs | factor
constexpr uint32_t kSensNone = 0xFFFFFFFFu;
constexpr size_t kSensLdsBudget = 64 * 1024;  // per workgroup of the LDS shape: two of them to a CU

// One constraint of a component.  c.ids number the component's variables (in its elimination order), c.jbase is the first of
// the record's partials among the component's (0 in the small shape, whose lanes keep one record's partials at a time) (c.jloc[e] = e: every emitted partial keeps a slot of its own, duplicates of a
// column are summed where the products are formed), c.param is the system's own value.
struct alignas(16) SensRec {
    DevCon c;
    uint16_t ecol[16];  // variable (component numbering) of each emitted partial: row 0's, then row 1's
    uint8_t ne0, ne1, pad0[2];
    uint32_t drv;   // place in the caller's `positions`, or kSensNone
    uint32_t slot;  // ... and among the component's driven records
    uint32_t pad1;
};
static_assert(sizeof(SensRec) == 128, "SensRec layout");

struct SensComp {
    uint32_t n, n_rec, n_drv, env;  // variables, records, driven records, entries of the envelope
    uint32_t rec0, n_jv;            // first record; partials of all records
    uint32_t o_vars, o_drv;         // in the u32 lists: caller's variable per local one; (place in `positions`, local record) per driven
    uint32_t o_rowptr, o_colend, o_aptr, o_apairs;  // block shapes: envelope rows (n + 1), last row of each column, product lists
    uint32_t width, pad[3];         // entries of the widest row
};
static_assert(sizeof(SensComp) == 64, "SensComp layout");

struct SensArgs {
    const SensComp* comps;
    const SensRec* recs;
    const uint32_t* u32;
    const uint32_t *list_small, *list_lds, *list_ws;  // components of each shape
    uint32_t n_small, n_lds, n_ws;
    uint32_t n_vars, n_param;
    uint64_t batch;
    const double* x;       // [batch][n_vars]
    const double* params;  // [batch][n_param] or null
    double lambda;
    double* S;             // [batch][n_param][n_vars]
    uint32_t* status;      // [batch]
    uint32_t* deg;         // [batch] or null
    double* ws;            // workspace shape: ws_stride doubles per workgroup of the grid
    uint64_t ws_stride;
};

namespace dev {

struct LaneArr {  // a lane's array in LDS, interleaved with the 63 other lanes'
    double* p;
    __device__ __forceinline__ double& operator[](uint32_t i) const { return p[i * 64u]; }
};

template <class JP>
__device__ __forceinline__ JacWriter<JP> sens_writer(JP jv, const DevCon& c) {
    JacWriter<JP> w;
    w.jv = jv;
    w.jbase = c.jbase;
    const uint32_t* l = reinterpret_cast<const uint32_t*>(c.jloc);
    w.loc[0] = l[0];
    w.loc[1] = l[1];
    w.loc[2] = l[2];
    w.loc[3] = l[3];
    w.weight = c.weight;
    return w;
}

__device__ __forceinline__ bool pivot_ok(double d) { return d > 0.0 && d <= 1.7976931348623157e308; }

}  // namespace dev

static __global__ void __launch_bounds__(64) sens_small_kernel(const SensArgs a) {
    using namespace dev;
    __shared__ double lane_mem[kSensSmallLane * 64];
    const uint64_t b = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (b >= a.batch) return;  // (no barrier below)
    const LaneArr jv{lane_mem + threadIdx.x};
    const LaneArr X{lane_mem + 16 * 64 + threadIdx.x};
    const LaneArr y{lane_mem + (16 + kSensSmallVars) * 64 + threadIdx.x};
    const LaneArr L{lane_mem + (16 + 2 * kSensSmallVars) * 64 + threadIdx.x};
    const double* xb = a.x + b * a.n_vars;
    const double* pb = a.params ? a.params + b * a.n_param : nullptr;
    for (uint32_t ci = blockIdx.y; ci < a.n_small; ci += gridDim.y) {
        const SensComp c = a.comps[a.list_small[ci]];
        const uint32_t* vars = a.u32 + c.o_vars;
        const uint32_t n = c.n;
        for (uint32_t i = 0; i < n; ++i) X[i] = xb[vars[i]];
        for (uint32_t e = 0; e < n * (n + 1) / 2; ++e) L[e] = 0.0;
        uint32_t n_deg = 0;
        for (uint32_t r = 0; r < c.n_rec; ++r) {
            SensRec rec = a.recs[c.rec0 + r];
            if (rec.drv != kSensNone && pb) rec.c.param = pb[rec.drv];
            bool deg = con_jacobian<false>(rec.c, X, sens_writer(jv, rec.c));
            if (rec.drv != kSensNone) {
                double g0, g1;
                deg = dparam::con_dparam(rec.c.kind, rec.c.tag, rec.c.ids, rec.c.param, X, g0, g1) || deg;
            }
            n_deg += deg ? 1u : 0u;
            // JtJ: every ordered pair of partials of one row, into the lower triangle
            uint32_t e0 = 0;
            for (uint32_t row = 0; row < 2; ++row) {
                const uint32_t ne = row ? rec.ne1 : rec.ne0;
                for (uint32_t ea = e0; ea < e0 + ne; ++ea) {
                    const uint32_t ia = rec.ecol[ea];
                    const double va = jv[ea];
                    for (uint32_t eb = e0; eb < e0 + ne; ++eb) {
                        const uint32_t ib = rec.ecol[eb];
                        if (ia >= ib) {
                            const uint32_t at = ia * (ia + 1) / 2 + ib;
                            L[at] = L[at] + va * jv[eb];
                        }
                    }
                }
                e0 += ne;
            }
        }
        if (a.deg && n_deg) atomicAdd(a.deg + b, n_deg);
        // Cholesky of the packed lower triangle, in place
        bool ok = true;
        for (uint32_t j = 0; j < n && ok; ++j) {
            const uint32_t rj = j * (j + 1) / 2;
            double d = L[rj + j] + a.lambda;
            for (uint32_t k = 0; k < j; ++k) d = d - L[rj + k] * L[rj + k];
            ok = pivot_ok(d);
            const double ljj = sqrt(d);
            L[rj + j] = ljj;
            for (uint32_t i = j + 1; i < n; ++i) {
                const uint32_t ri = i * (i + 1) / 2;
                double s = L[ri + j];
                for (uint32_t k = 0; k < j; ++k) s = s - L[ri + k] * L[rj + k];
                L[ri + j] = s / ljj;
            }
        }
        if (!ok) {
            a.status[b] = 1u;
            continue;
        }
        const uint32_t* drv = a.u32 + c.o_drv;
        for (uint32_t d = 0; d < c.n_drv; ++d) {
            const uint32_t pj = drv[2 * d];
            SensRec rec = a.recs[c.rec0 + drv[2 * d + 1]];
            if (pb) rec.c.param = pb[pj];
            (void)con_jacobian<false>(rec.c, X, sens_writer(jv, rec.c));
            double g0, g1;
            (void)dparam::con_dparam(rec.c.kind, rec.c.tag, rec.c.ids, rec.c.param, X, g0, g1);
            g0 = rec.c.weight * g0;
            g1 = rec.c.weight * g1;
            for (uint32_t i = 0; i < n; ++i) y[i] = 0.0;
            for (uint32_t e = 0; e < (uint32_t)rec.ne0 + rec.ne1; ++e) {
                const uint32_t i = rec.ecol[e];
                y[i] = y[i] - jv[e] * (e < rec.ne0 ? g0 : g1);
            }
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t ri = i * (i + 1) / 2;
                double s = y[i];
                for (uint32_t k = 0; k < i; ++k) s = s - L[ri + k] * y[k];
                y[i] = s / L[ri + i];
            }
            for (uint32_t i = n; i-- > 0;) {
                const uint32_t ri = i * (i + 1) / 2;
                const double s = y[i] / L[ri + i];
                y[i] = s;
                for (uint32_t k = 0; k < i; ++k) y[k] = y[k] - L[ri + k] * s;
            }
            double* out = a.S + (b * a.n_param + pj) * a.n_vars;
            for (uint32_t i = 0; i < n; ++i) out[vars[i]] = y[i];
        }
    }
}

// LDS of a work item, in doubles: x[n] | g[2 n_drv] | (LDS shape: partials[n_jv] | envelope[env]) | as u32: vars[n] |
// rowptr[n + 1] | colend[n]
template <bool WS>
static __global__ void __launch_bounds__(256) sens_block_kernel(const SensArgs a) {
    using namespace dev;
    extern __shared__ double lds[];
    __shared__ uint32_t s_fail, s_deg;
    const uint32_t t = threadIdx.x, T = blockDim.x;
    const uint32_t n_list = WS ? a.n_ws : a.n_lds;
    const uint32_t* list = WS ? a.list_ws : a.list_lds;
    const uint64_t total = a.batch * n_list;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const uint64_t b = w / n_list;
        const SensComp c = a.comps[list[w - b * n_list]];
        const uint32_t n = c.n;
        double* xs = lds;
        double* g = xs + n;
        double* jv = WS ? a.ws + (uint64_t)blockIdx.x * a.ws_stride : g + 2 * c.n_drv;
        double* A = jv + c.n_jv;
        uint32_t* vars = reinterpret_cast<uint32_t*>(WS ? g + 2 * c.n_drv : A + c.env);
        uint32_t* rowptr = vars + n;
        uint32_t* colend = rowptr + n + 1;
        const double* xb = a.x + b * a.n_vars;
        const double* pb = a.params ? a.params + b * a.n_param : nullptr;
        if (t == 0) s_fail = s_deg = 0u;
        for (uint32_t i = t; i < n; i += T) {
            const uint32_t v = a.u32[c.o_vars + i];
            vars[i] = v;
            xs[i] = xb[v];
            colend[i] = a.u32[c.o_colend + i];
        }
        for (uint32_t i = t; i < n + 1; i += T) rowptr[i] = a.u32[c.o_rowptr + i];
        __syncthreads();
        // J and g: a record per lane
        for (uint32_t r = t; r < c.n_rec; r += T) {
            SensRec rec = a.recs[c.rec0 + r];
            if (rec.drv != kSensNone && pb) rec.c.param = pb[rec.drv];
            bool deg = con_jacobian<false>(rec.c, (const double*)xs, sens_writer(jv, rec.c));
            if (rec.drv != kSensNone) {
                double g0, g1;
                deg = dparam::con_dparam(rec.c.kind, rec.c.tag, rec.c.ids, rec.c.param, (const double*)xs, g0, g1) || deg;
                g[2 * rec.slot] = rec.c.weight * g0;
                g[2 * rec.slot + 1] = rec.c.weight * g1;
            }
            if (deg) atomicAdd(&s_deg, 1u);
        }
        __syncthreads();
        // the envelope of JtJ: an entry per lane, its products in the host's order
        {
            const uint32_t* aptr = a.u32 + c.o_aptr;
            const uint32_t* apairs = a.u32 + c.o_apairs;
            for (uint32_t e = t; e < c.env; e += T) {
                double s = 0.0;
                for (uint32_t p = aptr[e], p1 = aptr[e + 1]; p < p1; ++p) s = s + jv[apairs[2 * p]] * jv[apairs[2 * p + 1]];
                A[e] = s;
            }
        }
        __syncthreads();
        for (uint32_t i = t; i < n; i += T) A[rowptr[i + 1] - 1] = A[rowptr[i + 1] - 1] + a.lambda;
        __syncthreads();
        // left-looking Cholesky, column by column: row i of column j takes A[i][j] - sum_k L[i][k] L[j][k], k ascending
        // inside both envelopes; the row of the diagonal takes the root, then the others divide
        bool failed = false;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t rj = rowptr[j], wj = rowptr[j + 1] - rj - 1, fj = j - wj, last = colend[j];
            for (uint32_t i = j + t; i <= last; i += T) {
                const uint32_t ri = rowptr[i], fi = i - (rowptr[i + 1] - ri - 1);
                if (fi > j) continue;
                const uint32_t k0 = fi > fj ? fi : fj;
                const double* li = A + ri + (k0 - fi);
                const double* lj = A + rj + (k0 - fj);
                double s = A[ri + (j - fi)];
                for (uint32_t k = 0; k < j - k0; ++k) s = s - li[k] * lj[k];
                if (i == j) {
                    if (!pivot_ok(s)) s_fail = 1u;
                    s = sqrt(s);
                }
                A[ri + (j - fi)] = s;
            }
            __syncthreads();
            failed = s_fail != 0u;
            if (failed) break;
            const double ljj = A[rj + wj];
            for (uint32_t i = j + 1 + t; i <= last; i += T) {
                const uint32_t ri = rowptr[i], fi = i - (rowptr[i + 1] - ri - 1);
                if (fi <= j) A[ri + (j - fi)] = A[ri + (j - fi)] / ljj;
            }
            __syncthreads();
        }
        if (t == 0) {
            if (failed) a.status[b] = 1u;
            if (a.deg && s_deg) atomicAdd(a.deg + b, s_deg);
        }
        if (!failed) {
            // a right-hand side per lane, in place in its row of S (zero so far)
            for (uint32_t d = t; d < c.n_drv; d += T) {
                const uint32_t pj = a.u32[c.o_drv + 2 * d];
                const SensRec& rec = a.recs[c.rec0 + a.u32[c.o_drv + 2 * d + 1]];
                double* out = a.S + (b * a.n_param + pj) * a.n_vars;
                const uint32_t ne0 = rec.ne0, ne = ne0 + rec.ne1, jb = rec.c.jbase;
                uint32_t first = n;
                for (uint32_t e = 0; e < ne; ++e) {
                    const uint32_t i = rec.ecol[e];
                    first = i < first ? i : first;
                    out[vars[i]] = out[vars[i]] - jv[jb + e] * g[2 * d + (e < ne0 ? 0 : 1)];
                }
                for (uint32_t i = first; i < n; ++i) {
                    const uint32_t ri = rowptr[i], wi = rowptr[i + 1] - ri - 1, fi = i - wi;
                    double s = out[vars[i]];
                    for (uint32_t k = fi > first ? fi : first; k < i; ++k) s = s - A[ri + (k - fi)] * out[vars[k]];
                    out[vars[i]] = s / A[ri + wi];
                }
                for (uint32_t i = n; i-- > 0;) {
                    const uint32_t ri = rowptr[i], wi = rowptr[i + 1] - ri - 1, fi = i - wi;
                    const double s = out[vars[i]] / A[ri + wi];
                    out[vars[i]] = s;
                    for (uint32_t k = fi; k < i; ++k) out[vars[k]] = out[vars[k]] - A[ri + (k - fi)] * s;
                }
            }
        }
        __syncthreads();
    }
}

static __global__ void __launch_bounds__(256) sens_finish_kernel(const SensArgs a) {
    const uint64_t row = (uint64_t)a.n_param * a.n_vars;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (uint64_t b = blockIdx.y; b < a.batch; b += gridDim.y) {
        if (a.status[b] == 0u) continue;
        double* out = a.S + b * row;
        for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < row; i += (uint64_t)gridDim.x * 256u) out[i] = nan;
    }
}

}  // namespace ezpz
