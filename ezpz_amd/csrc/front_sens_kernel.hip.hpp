// Dimension sensitivities on the FRONTAL shape: S_b[j, :] = -(JtJ + lambda I)^-1 Jt g_j, g_j = d r / d p_j, with the
// machinery of front_kernel.hip.hpp -- its assembly, its factorisation of the fronts, its backward substitution, its chunks
// between the workgroups of a system -- and ONE factorisation for many right-hand sides.
//
// In the solve the forward substitution rides along inside the factorisation (the right-hand side is row S of every front), so
// another right-hand side costs another factorisation there.  Here a work item (system b, chunk c of the listed constraints)
//   1. gathers x_b, evaluates the Jacobian once (driven parameters overlaid by caller position, as the PAR build does), counts
//      degenerate constraints;
//   2. assembles JtJ + lambda I with an all-zero right-hand side and factorises: the factor stays in the panels;
//   3. for every right-hand side j of its chunk: zeroes the fronts' rhs rows, lets the constraint's home workgroup put g_j into
//      a residual-space vector that is zero elsewhere, runs the RHS-ONLY assembly stream (front_sens_types.hpp), then
//      front_fwd_rhs over the forward schedule -- the children's rhs rows (rhs-only extend-add; remote children's last rows as
//      chunks), the K entries of row S against the panel, the rows below into the last row of the update matrix -- and
//      front_bwd as it is; the own variables of d go to S[b, j, :].
// Every right-hand side, the first included, takes the same rhs-only pass: S[b, j, :] does not depend on the rest of the list,
// its order or the chunking.  front_fwd_rhs keeps the operation order of front_pivots (ascending fma per column) and of
// front_schur (acc0 / acc1), so the bits are those a ride-along substitution gives.
//
// Between workgroups: `epoch` tags the chunks of one pass (the factorisation, then one per right-hand side), `fact_no` counts
// the passes for the `arrived` / `bdone` counters; both advance per pass.  Why no chunk is overwritten before it is consumed:
// DESIGN.md 3g ("hazards").
#pragma once
#include "constraint_dparam.hip.hpp"
#include "front_kernel.hip.hpp"
#include "front_sens_types.hpp"

namespace ezpz {
namespace frontal {

// The rhs rows of front k: row S of its panel, the last row of its update matrix.
__device__ __forceinline__ void front_zero_rhs(const Ctx& cx, uint32_t k, int lane) {
    const DescRegs d = load_desc(cx.descs + k);
    const uint32_t K = d.K, S = d.S, S1 = S + 1, R = S - K;
    if ((uint32_t)lane < K) cx.ws[d.panel + lane * S1 + S] = 0.0;
    if (R && (uint32_t)lane <= R) cx.ws[d.upd + R * (R + 1) / 2 + lane] = 0.0;
}

// -Jt r into the fronts' rhs rows, all wavefronts: the FASM_RHS entries of the assembly stream alone (trips in global memory).
__device__ __forceinline__ void assemble_rhs(const Ctx& cx, const FrontWg& W, const uint32_t* tabs, uint32_t w_offs, uint32_t n_trips,
                                             uint32_t l_r) {
    double* const ws = cx.ws;
    const int lane = threadIdx.x & 63;
    const uint32_t nwaves = blockDim.x >> 6, o_j = cx.l_jv, o_pan = W.l_panels;
    for (uint32_t t = uni(threadIdx.x >> 6); t < n_trips; t += nwaves) {
        const uint32_t* st = tabs + uni(tabs[w_offs + t]);
        const uint32_t hdr = st[lane];
        const uint32_t w = uni(hdr >> 24);
        switch (w) {
        case 0: asm_trip<0>(ws, st, lane, hdr, o_j, l_r, o_pan, 0.0); break;
        case 1: asm_trip<1>(ws, st, lane, hdr, o_j, l_r, o_pan, 0.0); break;
        case 2: asm_trip<2>(ws, st, lane, hdr, o_j, l_r, o_pan, 0.0); break;
        case 3: asm_trip<3>(ws, st, lane, hdr, o_j, l_r, o_pan, 0.0); break;
        case 4: asm_trip<4>(ws, st, lane, hdr, o_j, l_r, o_pan, 0.0); break;
        case 5: asm_trip<5>(ws, st, lane, hdr, o_j, l_r, o_pan, 0.0); break;
        case 6: asm_trip<6>(ws, st, lane, hdr, o_j, l_r, o_pan, 0.0); break;
        default: {
            double acc = 0.0;
            for (uint32_t q = 0; q < w; ++q) {
                const uint32_t op = st[64 * (1 + q) + lane];
                acc = __builtin_fma(ws[o_j + (op & 0xFFFFu)], ws[l_r + (op >> 16)], acc);
            }
            if (!(hdr & FASM_NOP)) ws[o_pan + (hdr & 0xFFFFu)] = -acc;
        }
        }
    }
    __syncthreads();
}

// The forward substitution of front k for a right-hand side that is in the rhs rows, against the factor in its panel.
__device__ __forceinline__ void front_fwd_rhs(const Ctx& cx, uint32_t k, int lane, uint32_t o_pan, unsigned int epoch, const uint32_t* tabs,
                                              uint32_t w_ext) {
    const DescRegs d = load_desc(cx.descs + k);
    const uint32_t K = d.K, S = d.S, S1 = S + 1, R = S - K;
    double* const ws = cx.ws;
    const uint32_t o_p = d.panel, o_u = d.upd;
    // ---- the rhs rows of this workgroup's own children, gathered by destination ----------------------------------------------------
    {
        const uint32_t* st = tabs + uni(tabs[w_ext + 2 * k]);
        for (uint32_t t = 0, nt = uni(tabs[w_ext + 2 * k + 1]); t < nt; ++t) {
            const uint32_t hdr = st[lane];
            const uint32_t v = uni(hdr >> 24);
            const uint32_t dst = o_pan + (hdr & 0xFFFFu);
            double acc = ws[dst];
            for (uint32_t q = 0; q < v; ++q) {
                const uint32_t x = st[64 * (1 + q) + lane];
                acc += ws[o_pan + (x & 0xFFFFu)] + ws[o_pan + (x >> 16)];
            }
            if (!(hdr & FASM_NOP)) ws[dst] = acc;
            st += 64 * (1 + v);
        }
    }
    wave_sync();
    // ---- children in other workgroups: the last row of their update matrices arrives as chunks ------------------------------------
    for (uint32_t c = 0; c < d.n_child; ++c) {
        const uint4 q = *reinterpret_cast<const uint4*>(cx.children + d.child0 + c);
        const uint32_t upd = uni(q.x), last = (uni(q.y) & 0xFFFFu) - 1;
        const uint8_t* const map = cx.maps + uni(q.z);
        if ((uint32_t)lane < last) {
            const uint32_t i = map[last], j = map[lane];
            const double val = grid_wait(cx.chunks + upd + tri_index(last, lane), epoch, cx.dead);
            const uint32_t dst = j < K ? o_p + j * S1 + i : o_u + tri_index(i - K, j - K);
            ws[dst] += val;
        }
        wave_sync();
    }
    // ---- y_c = (b_c - sum_{j < c} L[c][j] y_j) / d_c: lane = row, the panel column-major, its diagonal holds 1 / d --------------------
    const uint32_t r = (uint32_t)lane;
    const uint32_t kc = r < K ? r : K - 1;
    double t = ws[o_p + kc * S1 + S];
    const double rinv = ws[o_p + kc * S1 + kc];
    double yown = 0.0;
    for (uint32_t j = 0; j < K; ++j) {
        const double yj = readlane_f64(t * rinv, j);
        if (r > j && r < K) t = __builtin_fma(-yj, ws[o_p + j * S1 + r], t);
        if (r == j) yown = yj;
    }
    if (r < K) ws[o_p + r * S1 + S] = yown;
    // ---- the rows below: U[R][b] -= sum_c L[K + b][c] y_c, into the update matrix's last row or the remote parent's chunks ------------
    if (R) {
        const uint32_t rb = o_p + K + (r < R ? r : 0);
        double acc0 = 0.0, acc1 = 0.0;
        for (uint32_t c = 0; c < K; c += 2) {
            acc0 = __builtin_fma(readlane_f64(yown, c), ws[rb + c * S1], acc0);
            if (c + 1 < K) acc1 = __builtin_fma(readlane_f64(yown, c + 1), ws[rb + (c + 1) * S1], acc1);
        }
        if (r < R) {
            const uint32_t e = tri_index(R, r);
            const double v = ws[o_u + e] - (acc0 + acc1);
            if (d.flags & FRONT_REMOTE_PARENT)
                grid_store(cx.chunks + d.up_chunk + e, v, epoch);
            else
                ws[o_u + e] = v;
        }
    }
}

}  // namespace frontal

// A constraint's record with the call's value of its parameter; ps: its place in the list, or kNoParamSlot.
__device__ __forceinline__ DevCon front_sens_load_con(const DevCon* p, const FrontSensArgs& a, const double* par, uint32_t& ps) {
    DevCon c = load_con(p);
    ps = a.par_slot[c.pos];
    if (ps != kNoParamSlot && par) c.param = par[ps];
    return c;
}

template <bool LIN>
__global__ void __launch_bounds__(512, 1) front_sens_kernel(const FrontSensArgs a) {
    using namespace frontal;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = (uint32_t)tid >> 6, nwaves = blockDim.x >> 6;
    const uint32_t G = a.n_wgs, wg = blockIdx.x % G, slot = blockIdx.x / G, n_slots = gridDim.x / G;
    const FrontWg& W = reinterpret_cast<const FrontWg*>(a.plan)[wg];
    // ---- LDS: front_solve_kernel's carve-up ([staged tables][workspace][128 doubles][triangle table][ints][arrived | bdone]) --------
    unsigned char* const tab = reinterpret_cast<unsigned char*>(smem);
    double* const ws = smem + a.tab_lds_bytes / 8;
    uint16_t* const tri = reinterpret_cast<uint16_t*>(ws + a.ws_doubles + 128);
    int* const ints = reinterpret_cast<int*>(tri + 2080);  // [1] a pivot failed
    unsigned int* const arrived = reinterpret_cast<unsigned int*>(ints + 16);
    unsigned int* const bdone = arrived + W.n_fronts;
    for (uint32_t i = tid; i < 2 * W.n_fronts; i += blockDim.x) arrived[i] = 0;
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.plan + W.o_tables);
        uint4* dst = reinterpret_cast<uint4*>(tab);
        for (uint32_t i = tid; i < W.tab_bytes / 16; i += blockDim.x) dst[i] = src[i];
        for (uint32_t ra = tid; ra < 64; ra += blockDim.x)
            for (uint32_t rb = 0; rb <= ra; ++rb) tri[tri_index(ra, rb)] = (uint16_t)(ra | (rb << 8));
    }
    Ctx cx;
    cx.ws = ws;
    cx.descs = reinterpret_cast<const FrontDesc*>(tab);
    cx.children = reinterpret_cast<const FrontChild*>(tab + W.t_children);
    cx.rows = reinterpret_cast<const uint16_t*>(tab + W.t_rows);
    cx.exports = reinterpret_cast<const uint32_t*>(tab + W.t_exports);
    cx.maps = reinterpret_cast<const uint8_t*>(tab + W.t_maps);
    cx.tri = tri;
    cx.stream = reinterpret_cast<const uint32_t*>(tab + W.t_stream);
    unsigned char* const scratch = G > 1 ? a.scratch + (size_t)slot * a.scratch_stride : nullptr;
    FrontScratchHead* const head = reinterpret_cast<FrontScratchHead*>(scratch);
    cx.chunks = G > 1 ? reinterpret_cast<gridchunk_t*>(scratch + sizeof(FrontScratchHead) + 2 * kFrontScratchRedBytes) : nullptr;
    cx.dead = G > 1 ? &head->dead : nullptr;
    cx.l_jv = W.l_jv;
    cx.l_d = W.l_d;
    cx.l_upool = W.l_upool;
#ifdef EZPZ_STAMPS
    cx.stamps = nullptr;
    cx.stamp_n = nullptr;
#endif
    const uint16_t* const sched = reinterpret_cast<const uint16_t*>(tab + W.t_sched);
    unsigned int fact_no = 0;  // passes of this launch so far (a factorisation, or one right-hand side's substitutions)
    unsigned int epoch = 0;    // tag of the chunks of one pass
    if (G > 1) epoch = __hip_atomic_load(&head->hop[wg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t n_loc = W.n_loc, n_own = W.n_own, n_cons = W.n_cons, m = W.n_rows, zj = W.zj;
    const uint32_t* const var_glob = reinterpret_cast<const uint32_t*>(a.plan + W.o_var_glob);
    const DevCon* const cons = W.t_cons != 0xFFFFFFFFu ? reinterpret_cast<const DevCon*>(tab + W.t_cons) : reinterpret_cast<const DevCon*>(a.plan + W.o_cons);
    const FrontGhost* const ghosts = reinterpret_cast<const FrontGhost*>(a.plan + W.o_ghosts);
    double* const xs = ws + W.l_x;
    double* const dv = ws + W.l_d;
    double* const jvp = ws + W.l_jv;
    const uint32_t l_rn = W.l_rn;
    if (tid == 0) {  // the operands of padding pairs
        ws[W.l_r + m] = 0.0;
        jvp[zj] = 0.0;
        ws[W.l_panels] = 0.0;
    }
    const bool unit_w = a.unit_weights != 0;
    const uint32_t* const tabs = a.tabs;
    const uint32_t w_asm_offs = uni(tabs[4 + 4 * wg]), asm_trips = uni(tabs[5 + 4 * wg]), w_ext = uni(tabs[6 + 4 * wg]);
    const uint32_t* const homes = tabs + uni(tabs[2]);
    const uint64_t n_items = a.batch * a.items_per_system;
    for (uint64_t item = slot; item < n_items; item += n_slots) {
        const uint64_t sys = item / a.items_per_system;
        const uint32_t j0 = (uint32_t)(item - sys * a.items_per_system) * a.rhs_per_item;
        const uint32_t j1 = j0 + a.rhs_per_item < a.n_param ? j0 + a.rhs_per_item : a.n_param;
        // (the previous item's readers of x, of the Jacobian and of d are behind its last barrier)
        const double* const x0 = a.x0 + sys * a.n_vars;
        for (uint32_t i = tid; i < n_loc; i += blockDim.x) xs[i] = x0[var_glob[i]];
        for (uint32_t i = tid; i <= m; i += blockDim.x) ws[l_rn + i] = 0.0;  // the residual-space vector of the right-hand sides
        const double* const par = a.params ? a.params + sys * a.n_param : nullptr;
        if (tid == 0) ints[1] = 0;
        __syncthreads();
        // ---- the Jacobian at x, once; degenerate constraints (3d: the Jacobian's guard, or a listed constraint's residual guard) -----
        {
            uint32_t n_deg = 0;
            for (uint32_t ci = tid; ci < n_cons; ci += blockDim.x) {
                uint32_t ps;
                const DevCon c = front_sens_load_con(cons + ci, a, par, ps);
                JacWriter<double*> w;
                w.jv = jvp;
                w.jbase = c.jbase;
                const uint32_t* loc = reinterpret_cast<const uint32_t*>(c.jloc);
                w.loc[0] = loc[0], w.loc[1] = loc[1], w.loc[2] = loc[2], w.loc[3] = loc[3];
                w.weight = unit_w ? 1.0 : c.weight;
                bool deg = con_jacobian<LIN>(c, (const double*)xs, w);
                if (ps != kNoParamSlot) {
                    double g0, g1;
                    deg = dparam::con_dparam(c.kind, c.tag, c.ids, c.param, (const double*)xs, g0, g1) || deg;
                }
                n_deg += deg ? 1u : 0u;
            }
            if (a.deg && n_deg && j0 == 0) atomicAdd(a.deg + sys, n_deg);  // (a system's first chunk counts for all of them)
        }
        __syncthreads();
        // ---- JtJ + lambda I with an all-zero right-hand side, factorised: the item's one factorisation ----------------------------------
        ++epoch;
        assemble(cx, W, a.lambda, l_rn);
        bool bad_here = false;
        ++fact_no;
        for (uint32_t i = uni(sched[wave]), i1 = uni(sched[wave + 1]); i < i1; ++i) {
            const uint32_t k = uni(sched[i]);
            const uint32_t kids = uni(cx.descs[k].n_kids_local), parent = uni(cx.descs[k].parent_local);
            if (kids) {
                const unsigned int want = kids * fact_no;
                while (uni(__hip_atomic_load(&arrived[k], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) != want) __builtin_amdgcn_s_sleep(1);
            }
            bad_here |= front_factor(cx, k, lane, W.l_panels, epoch);
            if (parent != 0xFFFFFFFFu) {
                wave_sync();
                if (lane == 0) __hip_atomic_fetch_add(&arrived[parent], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        if (bad_here && lane == 0) ints[1] = 1;
        if (G > 1) {
            // a pivot failed somewhere?  every workgroup tells workgroup 0, whose verdict comes back -- and orders the first
            // right-hand side's chunks behind the consumption of the factorisation's
            __syncthreads();
            if (wg != 0) {
                if (tid == 0) grid_store(cx.chunks + a.bad_chunk0 + wg, ints[1] ? 1.0 : 0.0, epoch);
            } else {
                if (tid > 0 && (uint32_t)tid < G && grid_wait(cx.chunks + a.bad_chunk0 + tid, epoch, cx.dead) != 0.0) ints[1] = 1;
                __syncthreads();
                if (tid == 0) grid_store(cx.chunks + a.verdict_chunk, ints[1] ? 1.0 : 0.0, epoch);
            }
            if (wg != 0) {
                if (tid == 0 && grid_wait(cx.chunks + a.verdict_chunk, epoch, cx.dead) != 0.0) ints[1] = 1;
            }
        }
        __syncthreads();
        const bool bad = ints[1] != 0;
        __syncthreads();  // (ints[1] is reset at the top of the next item)
        for (uint32_t j = bad ? j1 : j0; j < j1; ++j) {
            ++epoch;
            ++fact_no;
            // ---- the right-hand side: rhs rows zeroed, g_j where its constraint lives, -Jt g_j by the rhs-only assembly stream -----------
            for (uint32_t k = wave; k < W.n_fronts; k += nwaves) front_zero_rhs(cx, k, lane);
            const bool home = uni(homes[2 * j]) == wg && tid == 0;
            uint32_t g_row = 0, g_rows = 0;
            if (home) {
                uint32_t ps;
                const DevCon c = front_sens_load_con(cons + homes[2 * j + 1], a, par, ps);
                double g0, g1;
                (void)dparam::con_dparam(c.kind, c.tag, c.ids, c.param, (const double*)xs, g0, g1);
                const double wgt = unit_w ? 1.0 : c.weight;
                g_row = l_rn + c.row0;
                g_rows = c.nrows;
                ws[g_row] = wgt * g0;
                if (g_rows > 1) ws[g_row + 1] = wgt * g1;
            }
            __syncthreads();
            assemble_rhs(cx, W, tabs, w_asm_offs, asm_trips, l_rn);
            if (home) {
                ws[g_row] = 0.0;
                if (g_rows > 1) ws[g_row + 1] = 0.0;
            }
            // ---- forward, every wavefront its list of fronts ----------------------------------------------------------------------------
            for (uint32_t i = uni(sched[wave]), i1 = uni(sched[wave + 1]); i < i1; ++i) {
                const uint32_t k = uni(sched[i]);
                const uint32_t kids = uni(cx.descs[k].n_kids_local), parent = uni(cx.descs[k].parent_local);
                if (kids) {
                    const unsigned int want = kids * fact_no;
                    while (uni(__hip_atomic_load(&arrived[k], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) != want) __builtin_amdgcn_s_sleep(1);
                }
                front_fwd_rhs(cx, k, lane, W.l_panels, epoch, tabs, w_ext);
                if (parent != 0xFFFFFFFFu) {
                    wave_sync();
                    if (lane == 0) __hip_atomic_fetch_add(&arrived[parent], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            __syncthreads();
            // ---- backward, top down; the entries of variables other workgroups eliminate arrive as chunks --------------------------------
            if (G > 1 && wg != 0) {
                for (uint32_t i = tid; i < W.n_ghost; i += blockDim.x) dv[ghosts[i].local] = grid_wait(cx.chunks + ghosts[i].chunk, epoch, cx.dead);
                __syncthreads();
            }
            double dmax = __builtin_nan("");
            for (uint32_t i = uni(sched[nwaves + 1 + wave]), i1 = uni(sched[nwaves + 2 + wave]); i < i1; ++i) {
                const uint32_t k = uni(sched[i]);
                const uint32_t parent = uni(cx.descs[k].parent_local);
                if (parent != 0xFFFFFFFFu)
                    while (uni(__hip_atomic_load(&bdone[parent], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) != fact_no) __builtin_amdgcn_s_sleep(1);
                dmax = front_bwd(cx, k, lane, epoch, dmax);
                wave_sync();
                if (lane == 0) __hip_atomic_store(&bdone[k], fact_no, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            __syncthreads();
            // (an entry that is exactly zero keeps the +0.0 of the fill: the variables of a component without the listed constraint)
            double* const out = a.S + (sys * a.n_param + j) * a.n_vars;
            for (uint32_t i = tid; i < n_own; i += blockDim.x) {
                const double v = dv[i];
                if (v != 0.0) out[var_glob[i]] = v;
            }
            __syncthreads();
        }
        if (tid == 0 && wg == 0) {
            if (bad) atomicMax(a.sens_status + sys, 1u);
            if (G > 1 && __hip_atomic_load(cx.dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.sens_status + sys, 2u);
        }
        __syncthreads();
    }
    if (G > 1 && tid == 0) __hip_atomic_store(&head->hop[wg], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A system whose status is not zero gets its whole S filled with NaN.
static __global__ void __launch_bounds__(256) front_sens_finish_kernel(double* S, const uint32_t* status, uint64_t row, uint64_t batch) {
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (uint64_t b = blockIdx.y; b < batch; b += gridDim.y) {
        if (status[b] == 0u) continue;
        double* out = S + b * row;
        for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < row; i += (uint64_t)gridDim.x * 256u) out[i] = nan;
    }
}

}  // namespace ezpz
