// Batch solves whose systems bring their own constraint parameters (driven dimensions): ezpz_system_solve_batch_params and its
// device form.  One topology, `batch` dimension sets: params[b][j] replaces cs[positions[j]].param for system b.
//
// The route of this entry is its own: the component interpreter for a block system whose plan it can run
// (comp_kernel.hip.hpp, the PAR builds: a per-call overlay beside the chunks' parameter tables), else the list-walk teams on
// one workgroup per system or less (lm_kernel.hip.hpp, the PAR builds: instantiated here, beside launch.hip's).  Never the
// run-time compiled kernels -- lane, wavefront, block classes hold parameters as literals or stage them once per launch -- and
// never the lanes across the batch, whose programs carry the parameters in their records: a system that has been
// specialised, or whose plain calls take those shapes, is still served from here.  The fronts serve it where the caller asked
// for them (ezpz_system_set_params_route; front_params.hip): an overlay by caller position beside their records.
#include "driven_params.hpp"
#include "list_walk_launch.hip.hpp"

using namespace ezpz;

namespace {

int launch_params(EzpzSystem& s, SolveArgs& a, bool for_comp, hipStream_t stream) {
    if (s.params_route == EZPZ_PARAMS_ROUTE_FRONTS) return front_params_launch(s, a, false, stream);
    if (for_comp) {
        CompLaunch L = comp_launch_args(a);
        L.params = a.params;
        L.par_overlay = a.par_slot;
        L.n_param = a.n_param;
        return comp_launch(*s.comp, s.dev_comp, L, s.device, s.lim.cus, s.lim.lds_bytes, stream);
    }
    const ParLds L = par_lds_plan(s, a.n_param);  // (driven_params.hpp)
    const size_t copies = L.copies;
    const bool in_lds = L.in_lds;
    const size_t with = L.bytes;
    a.par_lds_off = L.off;
    static const bool say = debug_topic("params");
    if (say)
        std::fprintf(stderr, "[ezpz params] %u values per system %s (team mode %d, %zu copies, LDS %zu -> %zu of %zu bytes)\n", a.n_param,
                     in_lds ? "staged in LDS" : "read from global memory", s.rec ? 4 : s.mode, copies, s.lds_bytes, in_lds ? with : s.lds_bytes,
                     s.lim.lds_bytes);
    return list_walk_one_workgroup<true>(s, a, in_lds ? with : s.lds_bytes, stream);
}

}  // namespace

extern "C" {

int ezpz_system_solve_batch_params_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                          const double* params_dev, size_t batch, const EzpzConfig* cfg, double* x_out_dev,
                                          EzpzStatus* status_dev, uint8_t* unsat_mask_dev, uint64_t* warn_log_dev, uint32_t warn_cap,
                                          void* stream) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    if (n_param == 0)
        return ezpz_system_solve_batch_device(sys, x0_dev, batch, cfg, x_out_dev, status_dev, unsat_mask_dev, warn_log_dev, warn_cap, stream);
    if (!positions || !params_dev || n_param > 0xFFFFFFFEull) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch && (!x_out_dev || !status_dev)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch && sys->counts.n_vars && !x0_dev) return EZPZ_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> slot_of_pos;
    if (int rc = driven_slot_map(*sys, positions, n_param, slot_of_pos)) return rc;
    const bool for_comp = sys->comp && sys->comp->interpretable;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (the route is read again under the lock: a setter that runs between the two turns this call into an argument error)
    const uint32_t route = [&] {
        std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
        return sys->params_route;
    }();
    if (route == EZPZ_PARAMS_ROUTE_FRONTS) {
        // fronts on several workgroups allocate their scratch on first use and chain their launches on an event: never inside a capture
        if (sys->fronts->n_wgs > 1 && stream_capturing(st)) return EZPZ_ERR_INVALID_ARGUMENT;
    } else if (!for_comp) {
        if (int rc = ensure_program(sys)) return rc;
        // one system on several workgroups: declined (the workgroups' sub-programs would each need their slice of the side array)
        if (sys->mode != MODE_SUB && sys->grid_wgs > 1) return EZPZ_ERR_INVALID_ARGUMENT;
    }
    if (batch == 0) return EZPZ_OK;
    release_thread_kernel(sys->device);
    EZPZ_ON_DEVICE(sys->device);
    std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
    if (sys->params_route != route) return EZPZ_ERR_INVALID_ARGUMENT;
    if (int rc = driven_slots(*sys, positions, n_param, slot_of_pos, for_comp, route)) return rc;
    SolveArgs a = solve_args_for(sys, x0_dev, batch, cfg, x_out_dev, status_dev, unsat_mask_dev, warn_log_dev, warn_cap);
    a.params = params_dev;
    a.par_slot = sys->driven.slots.p;
    a.n_param = (uint32_t)n_param;
    // (the launches of this entry on one system run one behind the other, whatever their streams: the completion of the last one
    // is then the completion of all that read the table -- what a call with another list waits for before it overwrites it)
    EzpzSystem::DrivenParams& d = sys->driven;
    HIP_TRY(d.uploaded ? hipStreamWaitEvent(st, d.uploaded, 0) : hipEventCreateWithFlags(&d.uploaded, hipEventDisableTiming));
    const int rc = launch_params(*sys, a, for_comp, st);
    if (rc != EZPZ_OK) return rc;
    HIP_TRY(hipEventRecord(d.uploaded, st));
    return EZPZ_OK;
}

int ezpz_system_solve_batch_params(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params,
                                   size_t batch, const EzpzConfig* cfg, double* x_out, EzpzStatus* status, uint8_t* unsat_mask,
                                   uint64_t* warn_log, uint32_t warn_cap) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    if (n_param == 0) return ezpz_system_solve_batch(sys, x0, batch, cfg, x_out, status, unsat_mask, warn_log, warn_cap);
    if (!positions || !params) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch && (!x_out || !status || (sys->counts.n_vars && !x0))) return EZPZ_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    const size_t n = sys->counts.n_vars, C = sys->counts.n_cons;
    const bool want_log = warn_log && warn_cap;
    const size_t nb = std::max<size_t>(batch, 1);
    DevBuf<double>& par_dev = sys->par_dev;
    int rc;
    if ((rc = sys->x_dev.ensure(nb * std::max<size_t>(n, 1))) != EZPZ_OK) return rc;
    if ((rc = sys->st_dev.ensure(nb)) != EZPZ_OK) return rc;
    if ((rc = par_dev.ensure(nb * n_param)) != EZPZ_OK) return rc;
    if (unsat_mask && (rc = sys->mask_dev.ensure(nb * std::max<size_t>(C, 1))) != EZPZ_OK) return rc;
    if (want_log && (rc = sys->log_dev.ensure(nb * warn_cap)) != EZPZ_OK) return rc;
    if (batch && n) HIP_TRY(hipMemcpy(sys->x_dev.p, x0, batch * n * sizeof(double), hipMemcpyHostToDevice));
    if (batch) HIP_TRY(hipMemcpy(par_dev.p, params, batch * n_param * sizeof(double), hipMemcpyHostToDevice));
    // (errors of the request are the device form's: nothing has been enqueued then, and no output written)
    rc = ezpz_system_solve_batch_params_device(sys, sys->x_dev.p, positions, n_param, par_dev.p, batch, cfg, sys->x_dev.p, sys->st_dev.p,
                                               unsat_mask ? sys->mask_dev.p : nullptr, want_log ? sys->log_dev.p : nullptr, warn_cap,
                                               hipStreamPerThread);
    if (rc != EZPZ_OK || batch == 0) return rc;
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    HIP_TRY(hipMemcpy(status, sys->st_dev.p, batch * sizeof(EzpzStatus), hipMemcpyDeviceToHost));
    if (sys->params_route == EZPZ_PARAMS_ROUTE_FRONTS && sys->fronts->n_wgs > 1)  // (like every host entry of such a system: system.hpp)
        for (size_t b = 0; b < batch; ++b)
            if (status[b].iterations == EZPZ_ITERATIONS_TEAM_TIMEOUT) return EZPZ_ERR_HIP;
    if (n) HIP_TRY(hipMemcpy(x_out, sys->x_dev.p, batch * n * sizeof(double), hipMemcpyDeviceToHost));
    if (unsat_mask && C) HIP_TRY(hipMemcpy(unsat_mask, sys->mask_dev.p, batch * C, hipMemcpyDeviceToHost));
    if (want_log) {
        // only the entries the kernel wrote are meaningful: n_warnings per system, capped
        std::vector<uint64_t> log(batch * (size_t)warn_cap);
        HIP_TRY(hipMemcpy(log.data(), sys->log_dev.p, log.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < batch; ++b)
            std::memcpy(warn_log + b * warn_cap, log.data() + b * warn_cap, std::min<size_t>(status[b].n_warnings, warn_cap) * sizeof(uint64_t));
    }
    return EZPZ_OK;
}

}  // extern "C"
