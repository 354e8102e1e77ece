// The one path behind ezpz_system_solve_batch_params and ezpz_system_sweep_params (driven_params.hpp): the
// check of a `positions` list, the request that resolves a list into its routes, the device table a list becomes (kept on the
// system), the enqueue and the host form.  Host code only: the kernels are launched by the route launchers of params.hip,
// sweep.hip, guarded_sweep.hip (a sweep with a GuardLaunch: DESIGN.md 3j), front_params.hip and comp.hip, which instantiate them.
#include "driven_params.hpp"
#include "host_stage.hpp"

namespace ezpz {

int driven_slot_map(const EzpzSystem& s, const uint32_t* positions, size_t n_param, std::vector<uint32_t>& slot_of_pos) {
    if ((n_param && !positions) || n_param > 0xFFFFFFFEull) return EZPZ_ERR_INVALID_ARGUMENT;
    const size_t n_cs = s.host_has_param.size();
    slot_of_pos.assign(std::max<size_t>(n_cs, 1), kNoParamSlot);
    for (size_t j = 0; j < n_param; ++j) {
        const uint32_t pos = positions[j];
        if (pos >= n_cs || slot_of_pos[pos] != kNoParamSlot || !s.host_has_param[pos]) return EZPZ_ERR_INVALID_ARGUMENT;
        slot_of_pos[pos] = (uint32_t)j;
    }
    return EZPZ_OK;
}

int driven_request(EzpzSystem* sys, const uint32_t* positions, size_t n_param, DrivenRequest& r) {
    if (int rc = driven_slot_map(*sys, positions, n_param, r.slot_of_pos)) return rc;
    r.for_comp = sys->comp && sys->comp->interpretable;
    {
        std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
        r.params_route = sys->params_route;
    }
    if (r.params_route == EZPZ_PARAMS_ROUTE_FRONTS) {
        r.sweep_route = EZPZ_SWEEP_FRONTS;
    } else if (r.for_comp) {
        r.sweep_route = EZPZ_SWEEP_INTERPRETER;
    } else {
        if (int rc = ensure_program(sys)) return rc;
        if (sys->mode != MODE_SUB && sys->grid_wgs > 1) return EZPZ_ERR_INVALID_ARGUMENT;
        r.sweep_route = sys->mode == MODE_SUB    ? EZPZ_SWEEP_SUB_WAVEFRONT_TEAMS
                        : sys->mode == MODE_PART ? EZPZ_SWEEP_PARTITIONED_WORKGROUP
                        : sys->rec               ? EZPZ_SWEEP_RECORD_WALK
                                                 : EZPZ_SWEEP_BARRIER_WORKGROUP;
    }
    return EZPZ_OK;
}

namespace {

// What the request's list becomes on the device -- the list-walk teams' side array (per constraint of the table: its place in the
// list, or none), the interpreter's overlay, the fronts' map by caller position -- unless the system keeps it from its last call.
// `uploaded`: whether it had to be made.  (launch_mu is held.)
int driven_table(EzpzSystem& s, const DrivenRequest& r, const uint32_t* positions, size_t n_param, bool& uploaded) {
    EzpzSystem::DrivenParams& d = s.driven;
    uploaded = !(d.list.same(positions, n_param) && d.for_comp == r.for_comp && d.route == r.params_route);
    if (!uploaded) return EZPZ_OK;
    d.list.valid = false;
    std::vector<uint32_t> table;
    if (r.params_route == EZPZ_PARAMS_ROUTE_FRONTS) {
        table = r.slot_of_pos;  // (the fronts' records carry the caller's position: the map itself)
    } else if (r.for_comp) {
        comp_param_overlay(*s.comp, r.slot_of_pos.data(), table);
    } else {
        table.resize(std::max<size_t>(s.host_con_pos.size(), 1), kNoParamSlot);
        for (size_t ci = 0; ci < s.host_con_pos.size(); ++ci) table[ci] = r.slot_of_pos[s.host_con_pos[ci]];
    }
    if (int rc = d.list.before_overwrite()) return rc;
    if (int rc = d.slots.ensure(table.size())) return rc;
    HIP_TRY(hipMemcpy(d.slots.p, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    d.list.keep(positions, n_param);
    d.for_comp = r.for_comp;
    d.route = r.params_route;
    return EZPZ_OK;
}

}  // namespace

int driven_enqueue(EzpzSystem* sys, const DrivenRequest& r, const double* x0_dev, const uint32_t* positions, size_t n_param,
                   const double* params_dev, size_t steps, size_t batch, const EzpzConfig* cfg, double* x_out_dev, EzpzStatus* status_dev,
                   uint8_t* unsat_mask_dev, uint64_t* warn_log_dev, uint32_t warn_cap, hipStream_t st, const GuardLaunch* guard) {
    const bool fronts = r.params_route == EZPZ_PARAMS_ROUTE_FRONTS;
    // fronts on several workgroups allocate their scratch on first use and chain their launches on an event: never inside a capture.
    // (A params call is told so before anything else, even one of no systems; a sweep once the thread's resident kernel is released.)
    auto refused = [&] { return fronts && sys->fronts->n_wgs > 1 && stream_capturing(st); };
    if (!steps && refused()) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch == 0) return EZPZ_OK;
    release_thread_kernel(sys->device);
    EZPZ_ON_DEVICE(sys->device);
    if (steps && refused()) return EZPZ_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
    if (sys->params_route != r.params_route) return EZPZ_ERR_INVALID_ARGUMENT;  // (a setter ran between the request and the lock)
    // (one table, lock and event for both entries: their launches on one system run one behind the other, and a list that either of
    // them used last uploads nothing)
    bool uploaded = false;
    if (int rc = driven_table(*sys, r, positions, n_param, uploaded)) return rc;
    if (steps && uploaded) call_stamp(SWEEP_TABLE_UPLOADED);
    SolveArgs a = solve_args_for(sys, x0_dev, batch, cfg, x_out_dev, status_dev, unsat_mask_dev, warn_log_dev, warn_cap);
    a.params = params_dev;
    a.par_slot = sys->driven.slots.p;
    a.n_param = (uint32_t)n_param;
    a.steps = (uint32_t)steps;
    // (the SWP builds take neither a list of systems nor resumed states nor a completion word: solve_args_for sets none)
    if (steps && (a.sys_list || a.sys_count || a.resume || a.done.flag || a.done.request)) return EZPZ_ERR_INVALID_ARGUMENT;
    KeptList& list = sys->driven.list;
    if (int rc = list.order_behind(st)) return rc;
    int rc;
    if (guard) {
        if (fronts || r.for_comp || !steps) return EZPZ_ERR_INVALID_ARGUMENT;
        GuardedSolveArgs ga{};
        static_cast<SolveArgs&>(ga) = a;
        ga.params0 = guard->params0;
        ga.params_reached = guard->params_reached;
        ga.guard = guard->guard;
        ga.max_move = guard->max_move;
        ga.h_min = guard->h_min;
        ga.max_attempts = guard->max_attempts;
        rc = list_walk_guarded_launch(*sys, ga, r.sweep_route, st);
    } else if (fronts)
        rc = front_params_launch(*sys, a, steps != 0, st);
    else if (r.for_comp)
        rc = steps ? comp_sweep_launch(*sys, a, st)
                   : comp_launch(*sys->comp, sys->dev_comp, comp_driven_launch_args(a), sys->device, sys->lim.cus, sys->lim.lds_bytes, st);
    else
        rc = steps ? list_walk_sweep_launch(*sys, a, r.sweep_route, st) : list_walk_params_launch(*sys, a, st);
    if (rc != EZPZ_OK) return rc;
    if (int rc2 = list.record(st)) return rc2;
    if (steps) call_stamp(SWEEP_LAUNCHED);
    return EZPZ_OK;
}

int driven_host_form(EzpzSystem* sys, const double* x0, size_t n_param, const double* params, size_t steps, size_t batch, double* x_out,
                     EzpzStatus* status, uint8_t* unsat_mask, uint64_t* warn_log, uint32_t warn_cap, const DrivenDeviceForm& device_form) {
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    const size_t n = sys->counts.n_vars, C = sys->counts.n_cons;
    const bool want_log = warn_log && warn_cap;
    const size_t all = std::max<size_t>(steps, 1) * batch, rows = std::max<size_t>(all, 1);
    int rc;
    if ((rc = sys->x_dev.ensure(rows * std::max<size_t>(n, 1))) != EZPZ_OK) return rc;
    if ((rc = sys->st_dev.ensure(rows)) != EZPZ_OK) return rc;
    if ((rc = sys->par_dev.ensure(rows * std::max<size_t>(n_param, 1))) != EZPZ_OK) return rc;
    if (unsat_mask && (rc = sys->mask_dev.ensure(rows * std::max<size_t>(C, 1))) != EZPZ_OK) return rc;
    if (want_log && (rc = sys->log_dev.ensure(rows * warn_cap)) != EZPZ_OK) return rc;
    // (a sweep starts in step 0's block of the results: the one overlap of x0 and x_out its device form allows)
    if (all && n) HIP_TRY(hipMemcpy(sys->x_dev.p, x0, batch * n * sizeof(double), hipMemcpyHostToDevice));
    if (all && n_param) HIP_TRY(hipMemcpy(sys->par_dev.p, params, all * n_param * sizeof(double), hipMemcpyHostToDevice));
    // (errors of the request are the device form's: nothing has been enqueued then, and no output written)
    rc = device_form(sys->x_dev.p, sys->par_dev.p, sys->st_dev.p, unsat_mask ? sys->mask_dev.p : nullptr, want_log ? sys->log_dev.p : nullptr);
    if (rc != EZPZ_OK || all == 0) return rc;
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    HIP_TRY(hipMemcpy(status, sys->st_dev.p, all * sizeof(EzpzStatus), hipMemcpyDeviceToHost));
    if (sys->params_route == EZPZ_PARAMS_ROUTE_FRONTS && sys->fronts->n_wgs > 1)  // (like every host entry of such a system: system.hpp)
        for (size_t b = 0; b < all; ++b)
            if (status[b].iterations == EZPZ_ITERATIONS_TEAM_TIMEOUT) return EZPZ_ERR_HIP;
    if (n) HIP_TRY(hipMemcpy(x_out, sys->x_dev.p, all * n * sizeof(double), hipMemcpyDeviceToHost));
    if (unsat_mask && C) HIP_TRY(hipMemcpy(unsat_mask, sys->mask_dev.p, all * C, hipMemcpyDeviceToHost));
    return want_log ? copy_back_warn_log(warn_log, sys->log_dev.p, status, all, warn_cap) : EZPZ_OK;
}

void debug_params_line(const EzpzSystem& s, uint32_t n_param, bool in_lds, size_t copies, size_t lds_from, size_t lds_to) {
    static const bool say = debug_topic("params");
    if (!say) return;
    const char* form = in_lds ? "staged in LDS" : "read from global memory";
    if (copies)
        std::fprintf(stderr, "[ezpz params] %u values per system %s (team mode %d, %zu copies, LDS %zu -> %zu of %zu bytes)\n", n_param, form,
                     s.rec ? 4 : s.mode, copies, lds_from, lds_to, s.lim.lds_bytes);
    else
        std::fprintf(stderr, "[ezpz params] fronts: %u values per system %s (%u workgroups per system, LDS %zu -> %zu of %zu bytes)\n", n_param,
                     form, s.fronts->n_wgs, lds_from, lds_to, s.lim.lds_bytes);
}

}  // namespace ezpz
