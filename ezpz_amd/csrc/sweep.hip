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
// A sweep in one launch is the params entry's call with `steps` (driven.cpp: driven_request, driven_enqueue, driven_host_form);
// this file keeps the entries' argument checks, the chain, the plan entry and the launchers of the SWP builds.
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

}  // namespace

// (the interpreter's launcher first: the kernels are emitted in the order of their first use, and the object keeps the layout it had)
int ezpz::comp_sweep_launch(EzpzSystem& s, const SolveArgs& a, hipStream_t stream) {
    CompArgs ca = comp_args_for(*s.comp, s.dev_comp, comp_driven_launch_args(a));
    ca.steps = a.steps;
    return s.comp->linear ? comp_launch_build<true, true, true>(*s.comp, ca, s.device, s.lim.cus, s.lim.lds_bytes, stream)
                          : comp_launch_build<false, true, true>(*s.comp, ca, s.device, s.lim.cus, s.lim.lds_bytes, stream);
}

int ezpz::list_walk_sweep_launch(EzpzSystem& s, SolveArgs& a, uint32_t route, hipStream_t stream) {
    const ParLds L = par_lds_plan(s, a.n_param);
    a.par_lds_off = L.off;
    static const bool say = debug_topic("params");
    if (say)
        std::fprintf(stderr, "[ezpz sweep] %zu sweeps of %zu steps, %u values per step %s (route %u, LDS %zu of %zu bytes)\n", (size_t)a.batch,
                     (size_t)a.steps, a.n_param, L.in_lds ? "staged in LDS" : "read from global memory", route, L.bytes, s.lim.lds_bytes);
    return list_walk_one_workgroup<true, true>(s, a, L.bytes, stream);
}

extern "C" {

int ezpz_system_sweep_params_plan(EzpzSystem* sys, const uint32_t* positions, size_t n_param, EzpzSweepPlan* out) {
    if (!sys || !out) return EZPZ_ERR_INVALID_ARGUMENT;
    DrivenRequest r;
    if (int rc = driven_request(sys, positions, n_param, r)) return rc;
    EzpzSweepPlan p{};
    p.route = r.sweep_route;
    p.in_kernel = n_param && route_in_kernel(*sys, r.sweep_route) ? 1u : 0u;
    if (r.sweep_route == EZPZ_SWEEP_FRONTS) {
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
    DrivenRequest r;
    if (int rc = driven_request(sys, positions, n_param, r)) return rc;
    if (!work) return EZPZ_OK;
    if (n_param && route_in_kernel(*sys, r.sweep_route))
        return driven_enqueue(sys, r, x0_dev, positions, n_param, params_dev, steps, batch, cfg, x_out_dev, status_dev, unsat_mask_dev,
                              warn_log_dev, warn_cap, static_cast<hipStream_t>(stream));
    // the chain itself, enqueued on the stream: step k's block of every array is a batch in the params entry's layout
    // (n_param == 0: the plain entry's re-solves with the system's own values, on whatever route it takes)
    const size_t n = sys->counts.n_vars, C = sys->counts.n_cons;
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

int ezpz_system_sweep_params(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params,
                             size_t steps, size_t batch, const EzpzConfig* cfg, double* x_out, EzpzStatus* status, uint8_t* unsat_mask,
                             uint64_t* warn_log, uint32_t warn_cap) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    const bool work = steps && batch;
    if (n_param && (!positions || !params)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (work && (!x_out || !status || (sys->counts.n_vars && !x0))) return EZPZ_ERR_INVALID_ARGUMENT;
    return driven_host_form(sys, x0, n_param, params, steps, work ? batch : 0, x_out, status, unsat_mask, warn_log, warn_cap,
                            [&](double* x_dev, const double* par_dev, EzpzStatus* st_dev, uint8_t* mask_dev, uint64_t* log_dev) {
                                return ezpz_system_sweep_params_device(sys, x_dev, positions, n_param, par_dev, steps, batch, cfg, x_dev, st_dev,
                                                                       mask_dev, log_dev, warn_cap, hipStreamPerThread);
                            });
}

}  // extern "C"
