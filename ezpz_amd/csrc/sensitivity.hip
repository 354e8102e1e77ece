// Dimension sensitivities: ezpz_system_param_sensitivity, its device form, ezpz_system_param_sensitivity_plan and
// ezpz_constraint_param_derivative (include/ezpz_amd.h).  The kernels are in sensitivity.hip.hpp and are
// instantiated here only; this file is the host side: the plan of a `positions` list -- connected components by union-find,
// the shape of every component that holds a listed constraint, its records, elimination order, envelope and product lists --
// kept on the system (a KeptList, like the params overlay's) with its device tables, workspace and the host entry's staging.
// The check of a list is the one every driven entry shares (driven_params.hpp: driven_slot_map).
#include "driven_params.hpp"
#include "host_stage.hpp"
#include "sensitivity.hip.hpp"

#include <numeric>

using namespace ezpz;

namespace {

static_assert(kSensNone == kNoParamSlot, "SensRec::drv takes the list check's map (driven_slot_map) as it is");

struct SensPlan {
    KeptList list;  // (its event: the last launch that read the tables and used the workspace)
    EzpzSensitivityPlan info{};
    std::vector<uint32_t> list_small, list_lds, list_ws;
    size_t lds_bytes = 0;       // dynamic LDS of the LDS shape's launch, and of the workspace shape's
    size_t ws_lds_bytes = 0;
    uint32_t lds_threads = 64;  // a single wavefront where no row of the envelope is wider
    uint64_t ws_stride = 0;     // doubles per workgroup
    uint32_t ws_grid = 0;
    uint32_t o_lists = 0;       // where the three lists start in the u32 table
    DevBuf<SensComp> comps;
    DevBuf<SensRec> recs;
    DevBuf<uint32_t> u32;
    DevBuf<double> ws;
    DevBuf<unsigned char> host_stage;  // the host entry's staging (host_stage.hpp)
};

struct Ids {
    const double* x;
    double operator[](uint32_t id) const { return x[id]; }
};

uint32_t find(std::vector<uint32_t>& parent, uint32_t v) {
    while (parent[v] != v) {
        parent[v] = parent[parent[v]];
        v = parent[v];
    }
    return v;
}

// entries of the row envelope of a component under `order` (local variable -> place): first[i] = the leftmost place that shares
// a row of J with place i
uint64_t envelope(const std::vector<std::vector<uint32_t>>& rows, const std::vector<uint32_t>& place, std::vector<uint32_t>& first) {
    const uint32_t n = (uint32_t)place.size();
    first.resize(n);
    std::iota(first.begin(), first.end(), 0u);
    for (const auto& row : rows) {
        uint32_t lo = n;
        for (uint32_t v : row) lo = std::min(lo, place[v]);
        for (uint32_t v : row) first[place[v]] = std::min(first[place[v]], lo);
    }
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += i - first[i] + 1;
    return total;
}

// reverse Cuthill-McKee over the graph whose edges are the pairs of variables that share a row
std::vector<uint32_t> rcm_places(const std::vector<std::vector<uint32_t>>& rows, uint32_t n) {
    std::vector<std::vector<uint32_t>> adj(n);
    for (const auto& row : rows)
        for (uint32_t a : row)
            for (uint32_t b : row)
                if (a != b) adj[a].push_back(b);
    for (auto& l : adj) {
        std::sort(l.begin(), l.end());
        l.erase(std::unique(l.begin(), l.end()), l.end());
    }
    auto by_degree = [&](uint32_t a, uint32_t b) { return adj[a].size() != adj[b].size() ? adj[a].size() < adj[b].size() : a < b; };
    std::vector<uint32_t> order;
    std::vector<uint8_t> seen(n, 0);
    std::vector<uint32_t> all(n);
    std::iota(all.begin(), all.end(), 0u);
    std::sort(all.begin(), all.end(), by_degree);
    for (uint32_t start : all) {
        if (seen[start]) continue;
        seen[start] = 1;
        order.push_back(start);
        for (size_t head = order.size() - 1; head < order.size(); ++head) {
            std::vector<uint32_t> next;
            for (uint32_t v : adj[order[head]])
                if (!seen[v]) {
                    seen[v] = 1;
                    next.push_back(v);
                }
            std::sort(next.begin(), next.end(), by_degree);
            order.insert(order.end(), next.begin(), next.end());
        }
    }
    std::vector<uint32_t> place(n);
    for (uint32_t k = 0; k < n; ++k) place[order[n - 1 - k]] = k;
    return place;
}

size_t block_lds_bytes(const SensComp& c, bool ws) {
    return ((size_t)c.n + 2 * (size_t)c.n_drv + (ws ? 0 : (size_t)c.n_jv + c.env)) * sizeof(double) + (3 * (size_t)c.n + 1) * sizeof(uint32_t);
}

// (no device is touched: the tables are left in the vectors)
int make_plan(const EzpzSystem& s, const uint32_t* positions, size_t n_param, const std::vector<uint32_t>& slot_of_pos, SensPlan& P,
              std::vector<SensComp>& comps, std::vector<SensRec>& recs, std::vector<uint32_t>& u32) {
    const size_t n_cs = s.host_cs.size(), n_vars = s.counts.n_vars;
    std::vector<uint32_t> parent(std::max<size_t>(n_vars, 1));
    std::iota(parent.begin(), parent.end(), 0u);
    for (size_t i = 0; i < n_cs; ++i) {
        const EzpzConstraint& c = s.host_cs[i];
        for (uint32_t k = 1; k < kKinds[c.kind].n_ids; ++k) {
            const uint32_t a = find(parent, c.ids[0]), b = find(parent, c.ids[k]);
            if (a != b) parent[std::max(a, b)] = std::min(a, b);
        }
    }
    // components in the order of their first variable; which are active
    std::vector<uint32_t> comp_of_root(std::max<size_t>(n_vars, 1), kSensNone);
    uint32_t n_comp = 0;
    for (uint32_t v = 0; v < n_vars; ++v)
        if (find(parent, v) == v) comp_of_root[v] = n_comp++;
    std::vector<uint8_t> active(std::max<uint32_t>(n_comp, 1), 0);
    for (size_t j = 0; j < n_param; ++j) active[comp_of_root[find(parent, s.host_cs[positions[j]].ids[0])]] = 1;
    std::vector<std::vector<uint32_t>> comp_vars(n_comp), comp_cons(n_comp);
    for (uint32_t v = 0; v < n_vars; ++v) {
        const uint32_t c = comp_of_root[find(parent, v)];
        if (active[c]) comp_vars[c].push_back(v);
    }
    for (size_t i = 0; i < n_cs; ++i) {
        if (kKinds[s.host_cs[i].kind].n_ids == 0) continue;
        const uint32_t c = comp_of_root[find(parent, s.host_cs[i].ids[0])];
        if (active[c]) comp_cons[c].push_back((uint32_t)i);
    }
    P.info = EzpzSensitivityPlan{};
    P.info.n_components = n_comp;
    comps.clear();
    recs.clear();
    u32.clear();
    P.list_small.clear();
    P.list_lds.clear();
    P.list_ws.clear();
    P.lds_bytes = P.ws_lds_bytes = 0;
    P.ws_stride = 0;
    uint32_t widest_lds = 0;
    std::vector<uint32_t> local(std::max<size_t>(n_vars, 1), 0);
    for (uint32_t ci = 0; ci < n_comp; ++ci) {
        if (!active[ci]) continue;
        const std::vector<uint32_t>& vars = comp_vars[ci];
        const uint32_t n = (uint32_t)vars.size();
        if (n > EZPZ_SENSITIVITY_MAX_COMPONENT_VARS) return EZPZ_ERR_INVALID_ARGUMENT;
        for (uint32_t k = 0; k < n; ++k) local[vars[k]] = k;
        // rows of J as lists of local variables (the caller's order), for the ordering and the envelope
        std::vector<std::vector<uint32_t>> rows;
        for (uint32_t pos : comp_cons[ci]) {
            const EzpzConstraint& c = s.host_cs[pos];
            const KindInfo& K = kKinds[c.kind];
            for (uint32_t r = 0; r < K.n_rows; ++r) {
                rows.emplace_back();
                for (uint32_t e = 0; e < K.n_emit[r]; ++e) rows.back().push_back(local[c.ids[K.emit[r][e]]]);
            }
        }
        const bool small = n <= kSensSmallVars;
        std::vector<uint32_t> place(n), first;
        std::iota(place.begin(), place.end(), 0u);
        uint64_t env = envelope(rows, place, first);
        if (!small) {
            std::vector<uint32_t> alt = rcm_places(rows, n), alt_first;
            const uint64_t alt_env = envelope(rows, alt, alt_first);
            if (alt_env < env) {
                place.swap(alt);
                first.swap(alt_first);
                env = alt_env;
            }
        }
        SensComp C{};
        C.n = n;
        C.n_rec = (uint32_t)comp_cons[ci].size();
        C.env = (uint32_t)env;
        C.rec0 = (uint32_t)recs.size();
        C.o_vars = (uint32_t)u32.size();
        u32.resize(u32.size() + n);
        for (uint32_t k = 0; k < n; ++k) u32[C.o_vars + place[k]] = vars[k];
        // records, in the caller's constraint order (the reference's row order)
        std::vector<std::pair<uint32_t, uint32_t>> driven;
        uint32_t n_jv = 0;
        for (uint32_t r = 0; r < C.n_rec; ++r) {
            const uint32_t pos = comp_cons[ci][r];
            const EzpzConstraint& c = s.host_cs[pos];
            const KindInfo& K = kKinds[c.kind];
            SensRec R{};
            for (uint32_t k = 0; k < K.n_ids; ++k) R.c.ids[k] = place[local[c.ids[k]]];
            R.c.param = c.param;
            R.c.weight = c.weight;
            R.c.jbase = small ? 0u : n_jv;  // (a lane of the small shape keeps one record's partials at a time)
            R.c.pos = pos;
            R.c.kind = (uint8_t)c.kind;
            R.c.tag = c.tag;
            R.c.nrows = K.n_rows;
            R.ne0 = K.n_emit[0];
            R.ne1 = K.n_rows > 1 ? K.n_emit[1] : 0;
            R.c.nslots = R.ne0 + R.ne1;
            uint32_t e = 0;
            for (uint32_t row = 0; row < K.n_rows; ++row)
                for (uint32_t k = 0; k < K.n_emit[row]; ++k, ++e) {
                    R.c.jloc[e] = (uint8_t)e;
                    R.ecol[e] = (uint16_t)place[local[c.ids[K.emit[row][k]]]];
                }
            n_jv += e;
            R.drv = slot_of_pos[pos];
            R.slot = 0;
            if (R.drv != kSensNone) {
                R.slot = (uint32_t)driven.size();
                driven.emplace_back(R.drv, r);
            }
            recs.push_back(R);
        }
        C.n_jv = n_jv;
        C.n_drv = (uint32_t)driven.size();
        C.o_drv = (uint32_t)u32.size();
        for (const auto& d : driven) {
            u32.push_back(d.first);
            u32.push_back(d.second);
        }
        P.info.n_active++;
        P.info.max_component_vars = std::max(P.info.max_component_vars, n);
        const uint32_t comp_index = (uint32_t)comps.size();
        if (small) {
            P.list_small.push_back(comp_index);
            comps.push_back(C);
            continue;
        }
        P.info.max_envelope = std::max<uint32_t>(P.info.max_envelope, C.env);
        // envelope rows, the last row of every column, and per entry the products that sum to it: every ordered pair of
        // partials of one row of J whose columns are (i, j), i >= j, in the caller's constraint order
        C.o_rowptr = (uint32_t)u32.size();
        u32.resize(u32.size() + n + 1);
        uint32_t at = 0;
        for (uint32_t i = 0; i < n; ++i) {
            u32[C.o_rowptr + i] = at;
            at += i - first[i] + 1;
            C.width = std::max(C.width, i - first[i] + 1);
        }
        u32[C.o_rowptr + n] = at;
        C.o_colend = (uint32_t)u32.size();
        u32.resize(u32.size() + n);
        for (uint32_t j = 0; j < n; ++j) u32[C.o_colend + j] = j;
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = first[i]; j <= i; ++j) u32[C.o_colend + j] = std::max(u32[C.o_colend + j], i);
        std::vector<uint32_t> count(C.env + 1, 0);
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<uint32_t> fill;
            if (pass == 1) {
                C.o_aptr = (uint32_t)u32.size();
                uint32_t run = 0;
                for (uint32_t e = 0; e <= C.env; ++e) {
                    const uint32_t k = e < C.env ? count[e] : 0;
                    u32.push_back(run);
                    run += k;
                }
                C.o_apairs = (uint32_t)u32.size();
                u32.resize(u32.size() + 2 * (size_t)run);
                fill.assign(u32.begin() + C.o_aptr, u32.begin() + C.o_aptr + C.env);
            }
            for (uint32_t r = 0; r < C.n_rec; ++r) {
                const SensRec& R = recs[C.rec0 + r];
                uint32_t e0 = 0;
                for (uint32_t row = 0; row < 2; ++row) {
                    const uint32_t ne = row ? R.ne1 : R.ne0;
                    for (uint32_t ea = e0; ea < e0 + ne; ++ea)
                        for (uint32_t eb = e0; eb < e0 + ne; ++eb) {
                            const uint32_t i = R.ecol[ea], j = R.ecol[eb];
                            if (i < j) continue;
                            const uint32_t entry = u32[C.o_rowptr + i] + (j - first[i]);
                            if (pass == 0) {
                                count[entry]++;
                            } else {
                                const uint32_t p = fill[entry]++;
                                u32[C.o_apairs + 2 * p] = R.c.jbase + ea;
                                u32[C.o_apairs + 2 * p + 1] = R.c.jbase + eb;
                            }
                        }
                    e0 += ne;
                }
            }
        }
        // (the kernel's two static words come on top of the dynamic LDS)
        const bool in_lds = block_lds_bytes(C, false) + 64 <= std::min(kSensLdsBudget, s.lim.lds_bytes);
        if (in_lds) {
            P.list_lds.push_back(comp_index);
            P.lds_bytes = std::max(P.lds_bytes, block_lds_bytes(C, false));
            widest_lds = std::max(widest_lds, C.width);
        } else {
            P.list_ws.push_back(comp_index);
            P.ws_lds_bytes = std::max(P.ws_lds_bytes, block_lds_bytes(C, true));
            P.ws_stride = std::max<uint64_t>(P.ws_stride, (uint64_t)C.n_jv + C.env);
        }
        comps.push_back(C);
    }
    P.lds_threads = widest_lds <= 64 ? 64 : 256;
    P.info.n_small = (uint32_t)P.list_small.size();
    P.info.n_lds = (uint32_t)P.list_lds.size();
    P.info.n_workspace = (uint32_t)P.list_ws.size();
    P.info.lds_bytes = (uint32_t)P.lds_bytes;
    P.info.workspace_bytes = P.ws_stride * sizeof(double);
    // resident workgroups of the workspace shape: the device's CUs, fewer where that would take more than 512 MiB
    P.ws_grid = 0;
    if (P.ws_stride) {
        // what a workgroup of the workspace shape keeps in LDS grows with the driven constraints of its component (g: two doubles
        // each): beyond the LDS budget the request is declined here, before anything is enqueued -- like one whose single
        // workspace would not fit the 512 MiB
        const uint64_t fit = (512ull << 20) / (P.ws_stride * sizeof(double));
        if (P.ws_lds_bytes + 64 > std::min(kSensLdsBudget, s.lim.lds_bytes) || fit == 0) return EZPZ_ERR_INVALID_ARGUMENT;
        P.ws_grid = (uint32_t)std::min<uint64_t>((uint64_t)std::max(s.lim.cus, 1), fit);
    }
    return EZPZ_OK;
}

// The system's plan for `positions` with its device tables (launch_mu is held; the system's device is current).
int plan_for(EzpzSystem* sys, const uint32_t* positions, size_t n_param, const std::vector<uint32_t>& slot_of_pos, SensPlan*& out) {
    if (!sys->sens) sys->sens = std::make_shared<SensPlan>();
    SensPlan& P = *static_cast<SensPlan*>(sys->sens.get());
    out = &P;
    if (P.list.same(positions, n_param)) return EZPZ_OK;
    std::vector<SensComp> comps;
    std::vector<SensRec> recs;
    std::vector<uint32_t> u32;
    SensPlan fresh;
    if (int rc = make_plan(*sys, positions, n_param, slot_of_pos, fresh, comps, recs, u32)) return rc;
    if (int rc = P.list.before_overwrite()) return rc;
    P.list.valid = false;
    std::vector<uint32_t> lists = fresh.list_small;
    lists.insert(lists.end(), fresh.list_lds.begin(), fresh.list_lds.end());
    lists.insert(lists.end(), fresh.list_ws.begin(), fresh.list_ws.end());
    const size_t o_lists = u32.size();
    u32.insert(u32.end(), lists.begin(), lists.end());
    int rc;
    if ((rc = P.comps.ensure(std::max<size_t>(comps.size(), 1))) != EZPZ_OK) return rc;
    if ((rc = P.recs.ensure(std::max<size_t>(recs.size(), 1))) != EZPZ_OK) return rc;
    if ((rc = P.u32.ensure(std::max<size_t>(u32.size(), 1))) != EZPZ_OK) return rc;
    if (fresh.ws_stride && (rc = P.ws.ensure(fresh.ws_stride * fresh.ws_grid)) != EZPZ_OK) return rc;
    if (!comps.empty()) HIP_TRY(hipMemcpy(P.comps.p, comps.data(), comps.size() * sizeof(SensComp), hipMemcpyHostToDevice));
    if (!recs.empty()) HIP_TRY(hipMemcpy(P.recs.p, recs.data(), recs.size() * sizeof(SensRec), hipMemcpyHostToDevice));
    if (!u32.empty()) HIP_TRY(hipMemcpy(P.u32.p, u32.data(), u32.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    P.info = fresh.info;
    P.o_lists = (uint32_t)o_lists;
    P.lds_bytes = fresh.lds_bytes;
    P.ws_lds_bytes = fresh.ws_lds_bytes;
    P.lds_threads = fresh.lds_threads;
    P.ws_stride = fresh.ws_stride;
    P.ws_grid = fresh.ws_grid;
    P.list.keep(positions, n_param);
    return EZPZ_OK;
}

}  // namespace

extern "C" {

int ezpz_constraint_param_derivative(const EzpzConstraint* c, const double* x, double g_out[2], int* degenerate) {
    if (degenerate) *degenerate = 0;
    if (!c || !x || !g_out || c->kind >= 25 || !kind_has_param(c->kind, c->tag)) return 0;
    double g0, g1;
    const bool deg = dparam::con_dparam(c->kind, c->tag, c->ids, c->param, Ids{x}, g0, g1);
    g_out[0] = c->weight * g0;
    g_out[1] = c->weight * g1;
    if (degenerate) *degenerate = deg ? 1 : 0;
    return kKinds[c->kind].n_rows;
}

int ezpz_system_param_sensitivity_plan(EzpzSystem* sys, const uint32_t* positions, size_t n_param, EzpzSensitivityPlan* out) {
    if (!sys || !out) return EZPZ_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> slot_of_pos;
    if (int rc = driven_slot_map(*sys, positions, n_param, slot_of_pos)) return rc;
    {
        // the fronts as this entry's route (ezpz_system_set_sensitivity_route; front_sens.hip): no component limit there
        std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
        if (sys->sens_route == EZPZ_SENSITIVITY_ROUTE_FRONTS) {
            EZPZ_ON_DEVICE(sys->device);
            return front_sens_plan_info(*sys, n_param, *out);
        }
    }
    SensPlan P;
    std::vector<SensComp> comps;
    std::vector<SensRec> recs;
    std::vector<uint32_t> u32;
    if (int rc = make_plan(*sys, positions, n_param, slot_of_pos, P, comps, recs, u32)) return rc;
    *out = P.info;
    return EZPZ_OK;
}

int ezpz_system_param_sensitivity_device(EzpzSystem* sys, const double* x_dev, const uint32_t* positions, size_t n_param,
                                         const double* params_dev, size_t batch, double lambda, double* S_out_dev, uint32_t* status_dev,
                                         uint32_t* degenerate_count_dev, void* stream) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> slot_of_pos;
    if (int rc = driven_slot_map(*sys, positions, n_param, slot_of_pos)) return rc;
    if (batch && (!status_dev || (n_param && (!S_out_dev || (sys->counts.n_vars && !x_dev))))) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch > 0xFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    release_thread_kernel(sys->device);
    EZPZ_ON_DEVICE(sys->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
    if (sys->sens_route == EZPZ_SENSITIVITY_ROUTE_FRONTS) {
        // (fronts on several workgroups allocate their scratch on first use and chain their launches on an event: never inside a capture)
        if (sys->fronts->n_wgs > 1 && stream_capturing(st)) return EZPZ_ERR_INVALID_ARGUMENT;
        if (batch == 0) return EZPZ_OK;
        if (n_param == 0) {
            HIP_TRY(hipMemsetAsync(status_dev, 0, batch * sizeof(uint32_t), st));
            return EZPZ_OK;
        }
        return front_sens_launch(*sys, x_dev, positions, n_param, slot_of_pos, params_dev, batch, lambda, S_out_dev, status_dev,
                                 degenerate_count_dev, st);
    }
    SensPlan* plan = nullptr;
    if (n_param)
        if (int rc = plan_for(sys, positions, n_param, slot_of_pos, plan)) return rc;
    if (batch == 0) return EZPZ_OK;
    HIP_TRY(hipMemsetAsync(status_dev, 0, batch * sizeof(uint32_t), st));
    if (n_param == 0) return EZPZ_OK;
    SensPlan& P = *plan;
    const size_t n_vars = sys->counts.n_vars;
    // (the launches of this entry on one system run one behind the other, whatever their streams: they share the workspace too)
    if (int rc = P.list.order_behind(st)) return rc;
    HIP_TRY(hipMemsetAsync(S_out_dev, 0, batch * n_param * n_vars * sizeof(double), st));
    if (degenerate_count_dev) HIP_TRY(hipMemsetAsync(degenerate_count_dev, 0, batch * sizeof(uint32_t), st));
    SensArgs a{};
    a.comps = P.comps.p;
    a.recs = P.recs.p;
    a.u32 = P.u32.p;
    a.n_small = P.info.n_small;
    a.n_lds = P.info.n_lds;
    a.n_ws = P.info.n_workspace;
    a.list_small = P.u32.p + P.o_lists;
    a.list_lds = a.list_small + a.n_small;
    a.list_ws = a.list_lds + a.n_lds;
    a.n_vars = (uint32_t)n_vars;
    a.n_param = (uint32_t)n_param;
    a.batch = batch;
    a.x = x_dev;
    a.params = params_dev;
    a.lambda = lambda;
    a.S = S_out_dev;
    a.status = status_dev;
    a.deg = degenerate_count_dev;
    a.ws = P.ws.p;
    a.ws_stride = P.ws_stride;
    if (a.n_small) {
        const dim3 grid((uint32_t)((batch + 63) / 64), std::min<uint32_t>(a.n_small, 65535u));
        hipLaunchKernelGGL(sens_small_kernel, grid, dim3(64), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    if (a.n_lds) {
        const uint64_t work = (uint64_t)batch * a.n_lds;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(work, (uint64_t)sys->lim.cus * 8);
        hipLaunchKernelGGL(sens_block_kernel<false>, dim3(grid), dim3(P.lds_threads), P.lds_bytes, st, a);
        HIP_TRY(hipGetLastError());
    }
    if (a.n_ws) {
        const uint64_t work = (uint64_t)batch * a.n_ws;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(work, P.ws_grid);
        hipLaunchKernelGGL(sens_block_kernel<true>, dim3(grid), dim3(256), P.ws_lds_bytes, st, a);
        HIP_TRY(hipGetLastError());
    }
    {
        const uint64_t row = (uint64_t)n_param * n_vars;
        const dim3 grid((uint32_t)std::min<uint64_t>((row + 255) / 256, 64), (uint32_t)std::min<uint64_t>(batch, 65535));
        hipLaunchKernelGGL(sens_finish_kernel, grid, dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return P.list.record(st);
}

int ezpz_system_param_sensitivity(EzpzSystem* sys, const double* x, const uint32_t* positions, size_t n_param, const double* params,
                                  size_t batch, double lambda, double* S_out, uint32_t* status_out, uint32_t* degenerate_count_out) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> slot_of_pos;
    if (int rc = driven_slot_map(*sys, positions, n_param, slot_of_pos)) return rc;
    if (batch && (!status_out || (n_param && (!S_out || (sys->counts.n_vars && !x))))) return EZPZ_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    if (!sys->sens) {
        std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
        if (!sys->sens) sys->sens = std::make_shared<SensPlan>();
    }
    SensPlan& P = *static_cast<SensPlan*>(sys->sens.get());
    const size_t n = sys->counts.n_vars;
    const double *x_dev, *par_dev;
    double* S_dev;
    uint32_t *st_dev, *deg_dev;
    Staged io;
    io.in(x, n_param ? batch * n : 0, x_dev);  // (without dimensions x is not read, and may be absent)
    io.in(params, batch * n_param, par_dev);
    io.out(S_out, batch * n_param * n, S_dev, Staged::kPlaced);  // (the device form wants S wherever there are dimensions, whatever n is)
    io.out(status_out, batch, st_dev);
    io.out(degenerate_count_out, n_param ? batch : 0, deg_dev);
    int rc;
    if ((rc = io.reserve(P.host_stage)) != EZPZ_OK || (rc = io.upload(P.host_stage)) != EZPZ_OK) return rc;
    // (errors of the request are the device form's: nothing has been enqueued then, and no output written)
    rc = ezpz_system_param_sensitivity_device(sys, x_dev, positions, n_param, par_dev, batch, lambda, S_dev, st_dev, deg_dev, hipStreamPerThread);
    if (rc != EZPZ_OK || batch == 0) return rc;
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    if ((rc = io.copy_back(P.host_stage)) != EZPZ_OK) return rc;
    if (degenerate_count_out && !n_param) std::memset(degenerate_count_out, 0, batch * sizeof(uint32_t));
    return EZPZ_OK;
}

}  // extern "C"
