// Dimension sweeps: ezpz_system_sweep_params and its device form.  `batch` sweeps of `steps` driven solves each on
// one topology; step k of sweep b takes params[k][b][:] and starts from step k - 1's answer (step 0 from x0[b]).  By definition
// the sweep is the chain
//     step 0:  ezpz_system_solve_batch_params_device(x0,           params[0]) -> x_out[0], status[0], ...
//     step k:  ezpz_system_solve_batch_params_device(x_out[k - 1], params[k]) -> x_out[k], status[k], ...
// and every layout is step-major so that the chain can be issued literally -- which is what a route with in_kernel == 0 does.
// The routes are the params entry's (params.hip): the component interpreter for a block system, else the list-walk teams on one
// workgroup per system or less; in one launch they run the SWP builds of those kernels, instantiated here and nowhere else,
// whose teams keep a sweep's values in their workspace from one step to the next.  A system whose params route is the fronts
// (ezpz_system_set_params_route) sweeps on them: the SWP build of front_solve_kernel, instantiated in front_params.hip.
#include "call_trace.hpp"
#include "comp_launch.hip.hpp"
#include "driven_params.hpp"
#include "list_walk_launch.hip.hpp"

using namespace ezpz;

namespace {

// Which routes run a sweep in one launch.  profiles/sweep_rate.txt decides (tools/sweep_rate.py): a route whose one sweep of
// 240 steps is not faster in one launch than as the chain of launches, beyond the spread of the measurement, is listed here and
// stays on the chain (one bit per EZPZ_SWEEP_* route).  As measured, none is.  The fronts are measured apart for systems on one
// workgroup and on several (profiles/front_params_rate.txt, tools/front_params_rate.py), by the same rule: 1.01 to 1.02 x, beyond
// the spread in every case, so neither goes on the chain.
constexpr uint32_t kRoutesOnTheChain = 0;
constexpr bool kFrontsOneWgOnTheChain = false, kFrontsSeveralWgsOnTheChain = false;
bool route_in_kernel(const EzpzSystem& s, uint32_t route) {
    if (route == EZPZ_SWEEP_FRONTS) return !(s.fronts->n_wgs > 1 ? kFrontsSeveralWgsOnTheChain : kFrontsOneWgOnTheChain);
    return !(kRoutesOnTheChain >> route & 1u);
}

// (the program exists: ensure_program has run for a list-walk route)
uint32_t route_of(const EzpzSystem& s, bool for_comp) {
    if (for_comp) return EZPZ_SWEEP_INTERPRETER;
    if (s.mode == MODE_SUB) return EZPZ_SWEEP_SUB_WAVEFRONT_TEAMS;
    if (s.mode == MODE_PART) return EZPZ_SWEEP_PARTITIONED_WORKGROUP;
    return s.rec ? EZPZ_SWEEP_RECORD_WALK : EZPZ_SWEEP_BARRIER_WORKGROUP;
}

// What the device form, the host form and the plan check alike before anything else happens: the list, and the route it takes.
struct Request {
    std::vector<uint32_t> slot_of_pos;
    bool for_comp = false, fronts = false;
    uint32_t route = 0;
};
int check_request(EzpzSystem* sys, const uint32_t* positions, size_t n_param, Request& r) {
    if (n_param && (!positions || n_param > 0xFFFFFFFEull)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (int rc = driven_slot_map(*sys, positions, n_param, r.slot_of_pos)) return rc;
    r.for_comp = sys->comp && sys->comp->interpretable;
    {
        std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
        r.fronts = sys->params_route == EZPZ_PARAMS_ROUTE_FRONTS;
    }
    if (r.fronts) {
        r.route = EZPZ_SWEEP_FRONTS;
        return EZPZ_OK;
    }
    if (!r.for_comp) {
        if (int rc = ensure_program(sys)) return rc;
        // one system on several workgroups: declined, like the params entry declines it
        if (sys->mode != MODE_SUB && sys->grid_wgs > 1) return EZPZ_ERR_INVALID_ARGUMENT;
    }
    r.route = route_of(*sys, r.for_comp);
    return EZPZ_OK;
}

}  // namespace

extern "C" {

int ezpz_system_sweep_params_plan(EzpzSystem* sys, const uint32_t* positions, size_t n_param, EzpzSweepPlan* out) {
    if (!sys || !out) return EZPZ_ERR_INVALID_ARGUMENT;
    Request r;
    if (int rc = check_request(sys, positions, n_param, r)) return rc;
    EzpzSweepPlan p{};
    p.route = r.route;
    p.in_kernel = n_param && route_in_kernel(*sys, r.route) ? 1u : 0u;
    if (r.fronts) {
        p.lds_bytes = (uint32_t)sys->fronts->lds_bytes;
        if (n_param) {  // (the occupancy of the build: the one question of this entry that the device answers)
            EZPZ_ON_DEVICE(sys->device);
            std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
            FrontParLds L;
            if (int rc = front_params_lds_plan(*sys, n_param, p.in_kernel != 0, L)) return rc;
            p.params_in_lds = L.in_lds ? 1u : 0u;
            p.lds_bytes = L.bytes;
        }
    } else if (r.for_comp) {
        p.lds_bytes = sys->comp->lds_bytes;
    } else {
        const ParLds L = par_lds_plan(*sys, n_param);
        p.params_in_lds = n_param && L.in_lds ? 1u : 0u;
        p.lds_bytes = (uint32_t)(n_param ? L.bytes : sys->lds_bytes);
    }
    *out = p;
    return EZPZ_OK;
}

int ezpz_system_sweep_params_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                    const double* params_dev, size_t steps, size_t batch, const EzpzConfig* cfg, double* x_out_dev,
                                    EzpzStatus* status_dev, uint8_t* unsat_mask_dev, uint64_t* warn_log_dev, uint32_t warn_cap,
                                    void* stream) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    const bool work = steps && batch;
    if (n_param && !params_dev) return EZPZ_ERR_INVALID_ARGUMENT;
    if (steps > 0xFFFFFFFFull) return EZPZ_ERR_INVALID_ARGUMENT;
    if (work && (!x_out_dev || !status_dev)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (work && sys->counts.n_vars && !x0_dev) return EZPZ_ERR_INVALID_ARGUMENT;
    Request r;
    if (int rc = check_request(sys, positions, n_param, r)) return rc;
    if (!work) return EZPZ_OK;
    const size_t n = sys->counts.n_vars, C = sys->counts.n_cons;
    if (n_param == 0 || !route_in_kernel(*sys, r.route)) {
        // the chain itself, enqueued on the stream: step k's block of every array is a batch in the params entry's layout
        // (n_param == 0: the plain entry's re-solves with the system's own values, on whatever route it takes)
        for (size_t k = 0; k < steps; ++k) {
            const double* from = k ? x_out_dev + (k - 1) * batch * n : x0_dev;
            const int rc = ezpz_system_solve_batch_params_device(
                sys, from, positions, n_param, n_param ? params_dev + k * batch * n_param : nullptr, batch, cfg, x_out_dev + k * batch * n,
                status_dev + k * batch, unsat_mask_dev ? unsat_mask_dev + k * batch * C : nullptr,
                warn_log_dev && warn_cap ? warn_log_dev + k * batch * (size_t)warn_cap : nullptr, warn_cap, stream);
            if (rc != EZPZ_OK) return rc;
        }
        return EZPZ_OK;
    }
    release_thread_kernel(sys->device);
    EZPZ_ON_DEVICE(sys->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (fronts on several workgroups: never inside a capture, like the params entry)
    if (r.fronts && sys->fronts->n_wgs > 1 && stream_capturing(st)) return EZPZ_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
    const uint32_t proute = r.fronts ? EZPZ_PARAMS_ROUTE_FRONTS : EZPZ_PARAMS_ROUTE_DEFAULT;
    if (sys->params_route != proute) return EZPZ_ERR_INVALID_ARGUMENT;  // (a setter ran between the check and the lock)
    // (the params entry's table, lock and event: sweeps and params calls on one system run one behind the other, and a list
    // that either of them used last uploads nothing)
    EzpzSystem::DrivenParams& d = sys->driven;
    const bool repeated = driven_slots_cached(*sys, positions, n_param, r.for_comp, proute);
    if (int rc = driven_slots(*sys, positions, n_param, r.slot_of_pos, r.for_comp, proute)) return rc;
    if (!repeated) call_stamp(SWEEP_TABLE_UPLOADED);
    SolveArgs a = solve_args_for(sys, x0_dev, batch, cfg, x_out_dev, status_dev, unsat_mask_dev, warn_log_dev, warn_cap);
    a.params = params_dev;
    a.par_slot = d.slots.p;
    a.n_param = (uint32_t)n_param;
    a.steps = (uint32_t)steps;
    // (the SWP builds take neither a list of systems nor resumed states nor a completion word: solve_args_for sets none)
    if (a.sys_list || a.sys_count || a.resume || a.done.flag || a.done.request) return EZPZ_ERR_INVALID_ARGUMENT;
    HIP_TRY(d.uploaded ? hipStreamWaitEvent(st, d.uploaded, 0) : hipEventCreateWithFlags(&d.uploaded, hipEventDisableTiming));
    int rc;
    if (r.fronts) {
        rc = front_params_launch(*sys, a, true, st);
    } else if (r.for_comp) {
        CompArgs ca = comp_args_for(*sys->comp, sys->dev_comp, comp_launch_args(a));
        ca.params = a.params;
        ca.par_overlay = a.par_slot;
        ca.n_param = a.n_param;
        ca.steps = a.steps;
        rc = sys->comp->linear ? comp_launch_build<true, true, true>(*sys->comp, ca, sys->device, sys->lim.cus, sys->lim.lds_bytes, st)
                               : comp_launch_build<false, true, true>(*sys->comp, ca, sys->device, sys->lim.cus, sys->lim.lds_bytes, st);
    } else {
        const ParLds L = par_lds_plan(*sys, n_param);
        a.par_lds_off = L.off;
        static const bool say = debug_topic("params");
        if (say)
            std::fprintf(stderr, "[ezpz sweep] %zu sweeps of %zu steps, %u values per step %s (route %u, LDS %zu of %zu bytes)\n", batch,
                         steps, a.n_param, L.in_lds ? "staged in LDS" : "read from global memory", r.route, L.bytes, sys->lim.lds_bytes);
        rc = list_walk_one_workgroup<true, true>(*sys, a, L.bytes, st);
    }
    if (rc != EZPZ_OK) return rc;
    HIP_TRY(hipEventRecord(d.uploaded, st));
    call_stamp(SWEEP_LAUNCHED);
    return EZPZ_OK;
}

int ezpz_system_sweep_params(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params,
                             size_t steps, size_t batch, const EzpzConfig* cfg, double* x_out, EzpzStatus* status, uint8_t* unsat_mask,
                             uint64_t* warn_log, uint32_t warn_cap) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    const bool work = steps && batch;
    if (n_param && (!positions || !params)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (work && (!x_out || !status || (sys->counts.n_vars && !x0))) return EZPZ_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    const size_t n = sys->counts.n_vars, C = sys->counts.n_cons;
    const bool want_log = warn_log && warn_cap;
    const size_t rows = std::max<size_t>(work ? steps * batch : 0, 1);
    int rc;
    if ((rc = sys->x_dev.ensure(rows * std::max<size_t>(n, 1))) != EZPZ_OK) return rc;
    if ((rc = sys->st_dev.ensure(rows)) != EZPZ_OK) return rc;
    if ((rc = sys->par_dev.ensure(rows * std::max<size_t>(n_param, 1))) != EZPZ_OK) return rc;
    if (unsat_mask && (rc = sys->mask_dev.ensure(rows * std::max<size_t>(C, 1))) != EZPZ_OK) return rc;
    if (want_log && (rc = sys->log_dev.ensure(rows * warn_cap)) != EZPZ_OK) return rc;
    // (the sweeps start in step 0's block of the results: the one overlap of x0 and x_out the device form allows)
    if (work && n) HIP_TRY(hipMemcpy(sys->x_dev.p, x0, batch * n * sizeof(double), hipMemcpyHostToDevice));
    if (work && n_param) HIP_TRY(hipMemcpy(sys->par_dev.p, params, steps * batch * n_param * sizeof(double), hipMemcpyHostToDevice));
    // (errors of the request are the device form's: nothing has been enqueued then, and no output written)
    rc = ezpz_system_sweep_params_device(sys, sys->x_dev.p, positions, n_param, sys->par_dev.p, steps, batch, cfg, sys->x_dev.p, sys->st_dev.p,
                                         unsat_mask ? sys->mask_dev.p : nullptr, want_log ? sys->log_dev.p : nullptr, warn_cap,
                                         hipStreamPerThread);
    if (rc != EZPZ_OK || !work) return rc;
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    const size_t all = steps * batch;
    HIP_TRY(hipMemcpy(status, sys->st_dev.p, all * sizeof(EzpzStatus), hipMemcpyDeviceToHost));
    if (sys->params_route == EZPZ_PARAMS_ROUTE_FRONTS && sys->fronts->n_wgs > 1)  // (like every host entry of such a system: system.hpp)
        for (size_t b = 0; b < all; ++b)
            if (status[b].iterations == EZPZ_ITERATIONS_TEAM_TIMEOUT) return EZPZ_ERR_HIP;
    if (n) HIP_TRY(hipMemcpy(x_out, sys->x_dev.p, all * n * sizeof(double), hipMemcpyDeviceToHost));
    if (unsat_mask && C) HIP_TRY(hipMemcpy(unsat_mask, sys->mask_dev.p, all * C, hipMemcpyDeviceToHost));
    if (want_log) {
        // only the entries the kernel wrote are meaningful: n_warnings per (step, system), capped
        std::vector<uint64_t> log(all * (size_t)warn_cap);
        HIP_TRY(hipMemcpy(log.data(), sys->log_dev.p, log.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < all; ++b)
            std::memcpy(warn_log + b * warn_cap, log.data() + b * warn_cap, std::min<size_t>(status[b].n_warnings, warn_cap) * sizeof(uint64_t));
    }
    return EZPZ_OK;
}

}  // extern "C"
