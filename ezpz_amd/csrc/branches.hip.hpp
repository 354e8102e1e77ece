// Solution branches (include/ezpz_amd.h: ezpz_branch_cluster, ezpz_system_solve_branches and their _device forms):
// the rule two answers are compared by -- one __host__ __device__ body -- and the three kernels of a round: branch_start_kernel
// (the round's starts), branch_assign_kernel (every sample against the leaders known when the round begins, grid-wide) and
// branch_elect_kernel (one workgroup per base: the sequential leader pass over what is left).  The host plan and the entries are
// in branches.hip.
//
// The rule uses comparisons only.  Its one product and one sum are built without contraction (build.py: -ffp-contract=off for every
// unit), so `same` is the expression include/ezpz_amd.h writes down, on either side.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ezpz_amd.h"
#include "mc_sampler.hip.hpp"

namespace ezpz {
namespace branch {

// |a - c| <= eps_abs + eps_rel * max(|a|, |c|), as written (a and c finite: a sample with a non-finite compared value is not ok)
EZPZ_MC_HD bool same(double a, double c, double eps_abs, double eps_rel) {
    const double fa = fabs(a), fc = fabs(c);
    return fabs(a - c) <= eps_abs + eps_rel * (fa > fc ? fa : fc);
}

#ifdef __HIPCC__

// a label: the slot, or one of these (kPending never leaves a round)
constexpr int32_t kNotOk = -1, kOverflow = -2, kPending = -3;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kTileDoubles = 4096;  // the assign kernel's LDS tile: 32 KiB of compared leader values, five workgroups to a CU's 160 KiB
constexpr uint32_t kSamplesPerGroup = 16;  // samples a lane group of the assign kernel takes per staged tile

// ---- the round's starts: x[b][s][v] for the samples first + s, s < count, of every base ------------------------------------------
// mc_sample_kernel with a nominal per base -- x0[b][v] -- and sample 0 = x0[b] itself.
__global__ __launch_bounds__(256) void branch_start_kernel(const mc::Dist* __restrict__ dist, const double* __restrict__ x0, uint64_t seed,
                                                           uint64_t first, uint32_t count, uint64_t batch, uint32_t n_vars,
                                                           double* __restrict__ x) {
    const uint64_t total = batch * count * n_vars, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const uint64_t r = idx / n_vars, b = r / count;
        const uint32_t v = (uint32_t)(idx - r * n_vars);
        const uint64_t sample = first + (r - b * count);
        const double nominal = x0[b * n_vars + v];
        mc::Dist d = dist[v];
        d.nominal = nominal;
        x[idx] = sample == 0 ? nominal : mc::draw(seed, sample, v, d);
    }
}

// What the two clustering kernels of a round read and write.  A round is the samples first .. first + count - 1 of every base.
struct Round {
    const double* x;           // the answers: row (b, s) at x + (b * x_stride + s) * n_vars
    const uint8_t* ok;         // [b * x_stride + s] bytes (NULL: every one set) ...
    const EzpzStatus* status;  // ... and / or the solves' records (NULL: none)
    uint64_t x_stride;
    const double* origin;      // dist_inf is measured from the row origin + b * origin_stride
    uint64_t origin_stride;
    const uint32_t* cmp;       // [n_cmp]: the compared variables, ascending
    uint32_t n_cmp, n_vars;
    uint64_t batch, first, samples;
    uint32_t count, max_branches;
    double eps_abs, eps_rel;
    int32_t* label;            // label (b, s) at label[b * label_stride + s]
    uint64_t label_stride;
    uint32_t* pend;            // [batch][count]: the elect kernel's list of unmatched samples
    EzpzBranchInfo* info;      // [batch]
    EzpzBranch* branches;      // [batch][max_branches]
    double* x_branch;          // [batch][max_branches][n_vars]
    uint32_t fresh;            // the elect kernel classifies the samples itself: no assign launch went before it
};

__device__ inline bool flagged_ok(const Round& a, uint64_t at) {
    bool ok = !a.ok || a.ok[at] != 0;
    if (a.status) {
        const EzpzStatus st = a.status[at];
        ok = ok && st.converged != 0 && st.n_unsatisfied == 0;
    }
    return ok;
}

// ---- every sample of the round against the leaders known at its start ---------------------------------------------------------------
// A group of G lanes (8 / 16 / 32 / 64: the smallest that holds the compared variables, 64 with a loop beyond) takes one sample at a
// time, lane k the compared variable k; several samples share a wavefront when the sketch is small.  The group's verdict on a leader
// is a ballot.  A workgroup item is a span of 256 / G * 16 samples of one base; the base's leaders are staged in LDS, compared
// values only, in tiles of kTileDoubles (a row that does not fit a tile by itself is read from global memory instead).  Between
// tiles a sample's state is its label.  Every loop but the early exit is uniform over the workgroup, and that exit over the
// wavefront: a ballot always sees whole groups.
template <int G>
__global__ __launch_bounds__(256) void branch_assign_kernel(Round a, uint32_t tile_leaders, uint32_t spans_per_base) {
    extern __shared__ double s_tab[];
    constexpr uint32_t kGroups = 256 / G, kSpan = kGroups * kSamplesPerGroup;
    const uint32_t t = threadIdx.x, gid = t / G, gl = t % G, lane = t & 63u, n_cmp = a.n_cmp;
    const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull)) << (lane & ~(uint32_t)(G - 1));
    const bool single = n_cmp <= (uint32_t)G;  // one compared variable per lane: the sample's value stays in a register
    const uint32_t my_var = single && gl < n_cmp ? a.cmp[gl] : 0;
    const uint64_t items = a.batch * spans_per_base;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const uint64_t b = w / spans_per_base;
        const uint32_t s0 = (uint32_t)(w - b * spans_per_base) * kSpan;
        const uint32_t nb = (uint32_t)a.info[b].n_branches;
        const uint32_t per_tile = tile_leaders ? tile_leaders : (nb ? nb : 1);
        const uint32_t n_tiles = nb ? (nb + per_tile - 1) / per_tile : 1;  // (no leaders yet: one pass that classifies)
        const double* lead = a.x_branch + b * a.max_branches * a.n_vars;
        for (uint32_t tile = 0; tile < n_tiles; ++tile) {
            const uint32_t l0 = tile * per_tile, ln = nb > l0 ? (nb - l0 < per_tile ? nb - l0 : per_tile) : 0;
            __syncthreads();  // (the last tile's readers are through, and the labels they wrote are the workgroup's to read)
            if (tile_leaders) {
                for (uint32_t i = t; i < ln * n_cmp; i += 256) {
                    const uint32_t l = i / n_cmp, k = i - l * n_cmp;
                    s_tab[i] = lead[(uint64_t)(l0 + l) * a.n_vars + a.cmp[k]];
                }
                __syncthreads();
            }
            for (uint32_t i = 0; i < kSamplesPerGroup; ++i) {
                const uint32_t s = s0 + i * kGroups + gid;
                const bool live = s < a.count;
                const uint64_t at = b * a.x_stride + (live ? s : 0);
                const double* row = a.x + at * a.n_vars;
                int32_t* label = a.label + b * a.label_stride + (live ? s : 0);
                double mine = 0.0;
                if (single && live && gl < n_cmp) mine = row[my_var];
                bool fin = true;
                if (live && tile == 0) {
                    if (single)
                        fin = isfinite(mine);
                    else
                        for (uint32_t k = gl; k < n_cmp; k += G) fin = fin && isfinite(row[a.cmp[k]]);
                }
                const bool all_fin = (__ballot(fin) & gmask) == gmask;
                int32_t state = kNotOk;
                if (live) state = tile == 0 ? (flagged_ok(a, at) && all_fin ? kPending : kNotOk) : *label;
                const int32_t before = state;
                bool open = live && state == kPending;
                for (uint32_t l = 0; l < ln; ++l) {
                    if (__ballot(open) == 0) break;
                    bool m = true;
                    if (open) {
                        if (single) {
                            if (gl < n_cmp)
                                m = same(mine, tile_leaders ? s_tab[l * n_cmp + gl] : lead[(uint64_t)(l0 + l) * a.n_vars + my_var], a.eps_abs,
                                         a.eps_rel);
                        } else {
                            for (uint32_t k = gl; k < n_cmp; k += G) {
                                const uint32_t v = a.cmp[k];
                                m = m && same(row[v], tile_leaders ? s_tab[l * n_cmp + k] : lead[(uint64_t)(l0 + l) * a.n_vars + v], a.eps_abs,
                                              a.eps_rel);
                            }
                        }
                    }
                    const bool hit = (__ballot(m) & gmask) == gmask;
                    if (open && hit) state = (int32_t)(l0 + l), open = false;
                }
                if (live && gl == 0 && (tile == 0 || state != before)) *label = state;
            }
        }
    }
}

// ---- the round's election: one workgroup per base ---------------------------------------------------------------------------------
// What the assign kernel left unmatched (everything, in a fresh round) goes through the sequential leader pass: the lowest unmatched
// sample index -- a minimum over integers -- becomes the next leader, its row goes to x_branch, and the unmatched samples are compared
// against that leader only: they have failed the older ones already.  It ends when nothing is unmatched or the table is full; the
// rest is then overflow.  Bounded by max_branches, no word to another workgroup.  Counts are integer adds; dist_inf is a maximum of
// non-negative doubles taken on their bit patterns, which order as the values do.
__global__ __launch_bounds__(256) void branch_elect_kernel(Round a) {
    __shared__ uint32_t s_count[EZPZ_BRANCH_MAX];
    __shared__ uint32_t s_min, s_npend, s_nok, s_nover;
    __shared__ unsigned long long s_dist;
    const uint32_t t = threadIdx.x, n_cmp = a.n_cmp;
    for (uint64_t b = blockIdx.x; b < a.batch; b += gridDim.x) {
        __syncthreads();
        s_count[t] = 0;
        if (t == 0) s_min = kNone, s_npend = 0, s_nok = 0, s_nover = 0;
        __syncthreads();
        uint32_t nb = (uint32_t)a.info[b].n_branches;
        int32_t* label = a.label + b * a.label_stride;
        uint32_t* pend = a.pend + b * a.count;
        const double* org = a.origin + b * a.origin_stride;
        uint32_t lowest = kNone, n_ok = 0;
        for (uint32_t s = t; s < a.count; s += 256) {
            int32_t lab;
            if (a.fresh) {
                const uint64_t at = b * a.x_stride + s;
                const double* row = a.x + at * a.n_vars;
                bool ok = flagged_ok(a, at);
                for (uint32_t k = 0; ok && k < n_cmp; ++k) ok = isfinite(row[a.cmp[k]]);
                lab = ok ? kPending : kNotOk;
                label[s] = lab;
            } else {
                lab = label[s];
            }
            if (lab != kNotOk) ++n_ok;
            if (lab >= 0) atomicAdd(&s_count[lab], 1u);
            if (lab == kPending) {
                pend[atomicAdd(&s_npend, 1u)] = s;
                lowest = s < lowest ? s : lowest;
            }
        }
        if (n_ok) atomicAdd(&s_nok, n_ok);
        if (lowest != kNone) atomicMin(&s_min, lowest);
        __syncthreads();
        const uint32_t n_pend = s_npend;
        uint32_t leader = s_min;
        while (leader != kNone && nb < a.max_branches) {
            const uint32_t slot = nb++;
            const uint64_t at = b * a.x_stride + leader;
            const double* lrow = a.x + at * a.n_vars;
            double* out = a.x_branch + (b * a.max_branches + slot) * a.n_vars;
            __syncthreads();  // (everybody has read s_min)
            if (t == 0) s_min = kNone, s_dist = 0;
            __syncthreads();
            for (uint32_t k = t; k < a.n_vars; k += 256) out[k] = lrow[k];
            double d = 0.0;
            for (uint32_t k = t; k < n_cmp; k += 256) {
                const uint32_t v = a.cmp[k];
                const double e = fabs(lrow[v] - org[v]);
                if (e > d) d = e;  // (a NaN never wins)
            }
            if (d > 0.0) atomicMax(&s_dist, (unsigned long long)__double_as_longlong(d));
            uint32_t joined = 0;
            lowest = kNone;
            for (uint32_t e = t; e < n_pend; e += 256) {
                const uint32_t s = pend[e];
                if (label[s] != kPending) continue;
                const double* row = a.x + (b * a.x_stride + s) * a.n_vars;
                bool m = true;
                for (uint32_t k = 0; m && k < n_cmp; ++k) {
                    const uint32_t v = a.cmp[k];
                    m = same(row[v], lrow[v], a.eps_abs, a.eps_rel);
                }
                if (m)
                    label[s] = (int32_t)slot, ++joined;
                else
                    lowest = s < lowest ? s : lowest;
            }
            if (joined) atomicAdd(&s_count[slot], joined);
            if (lowest != kNone) atomicMin(&s_min, lowest);
            __syncthreads();
            if (t == 0) {
                EzpzBranch br;
                br.first = a.first + leader;
                br.count = 0;  // (added below, with the older slots')
                br.dist_inf = __longlong_as_double((long long)s_dist);
                if (a.status) {
                    br.status = a.status[at];
                } else {
                    br.status.iterations = br.status.converged = br.status.n_unsatisfied = br.status.n_warnings = 0;
                    br.status.final_residual_inf = br.status.final_lambda = 0.0;
                }
                a.branches[b * a.max_branches + slot] = br;
            }
            leader = s_min;
        }
        if (leader != kNone) {  // the table is full
            uint32_t over = 0;
            for (uint32_t e = t; e < n_pend; e += 256) {
                const uint32_t s = pend[e];
                if (label[s] == kPending) label[s] = kOverflow, ++over;
            }
            if (over) atomicAdd(&s_nover, over);
        }
        __syncthreads();
        if (t < nb && s_count[t]) a.branches[b * a.max_branches + t].count += s_count[t];
        if (t == 0) {
            EzpzBranchInfo in = a.info[b];
            in.samples = a.samples;
            in.n_ok += s_nok;
            in.n_branches = nb;
            in.n_overflow += s_nover;
            a.info[b] = in;
        }
    }
}

#endif  // __HIPCC__

}  // namespace branch
}  // namespace ezpz
