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
// The entries are their argument checks; the call itself is the sweep's too (driven.cpp: driven_request, driven_enqueue,
// driven_host_form), and this file's part of it the launch of the list-walk PAR builds.
#include "driven_params.hpp"
#include "list_walk_launch.hip.hpp"

using namespace ezpz;

int ezpz::list_walk_params_launch(EzpzSystem& s, SolveArgs& a, hipStream_t stream) {
    const ParLds L = par_lds_plan(s, a.n_param);
    a.par_lds_off = L.off;
    debug_params_line(s, a.n_param, L.in_lds, L.copies, s.lds_bytes, L.bytes);
    return list_walk_one_workgroup<true>(s, a, L.bytes, stream);
}

extern "C" {

int ezpz_system_solve_batch_params_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                          const double* params_dev, size_t batch, const EzpzConfig* cfg, double* x_out_dev,
                                          EzpzStatus* status_dev, uint8_t* unsat_mask_dev, uint64_t* warn_log_dev, uint32_t warn_cap,
                                          void* stream) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    if (n_param == 0)
        return ezpz_system_solve_batch_device(sys, x0_dev, batch, cfg, x_out_dev, status_dev, unsat_mask_dev, warn_log_dev, warn_cap, stream);
    if (!params_dev) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch && (!x_out_dev || !status_dev || (sys->counts.n_vars && !x0_dev))) return EZPZ_ERR_INVALID_ARGUMENT;
    DrivenRequest r;
    if (int rc = driven_request(sys, positions, n_param, r)) return rc;
    return driven_enqueue(sys, r, x0_dev, positions, n_param, params_dev, 0, batch, cfg, x_out_dev, status_dev, unsat_mask_dev, warn_log_dev,
                          warn_cap, static_cast<hipStream_t>(stream));
}

int ezpz_system_solve_batch_params(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params,
                                   size_t batch, const EzpzConfig* cfg, double* x_out, EzpzStatus* status, uint8_t* unsat_mask,
                                   uint64_t* warn_log, uint32_t warn_cap) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    if (n_param == 0) return ezpz_system_solve_batch(sys, x0, batch, cfg, x_out, status, unsat_mask, warn_log, warn_cap);
    if (!positions || !params) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch && (!x_out || !status || (sys->counts.n_vars && !x0))) return EZPZ_ERR_INVALID_ARGUMENT;
    return driven_host_form(sys, x0, n_param, params, 0, batch, x_out, status, unsat_mask, warn_log, warn_cap,
                            [&](double* x_dev, const double* par_dev, EzpzStatus* st_dev, uint8_t* mask_dev, uint64_t* log_dev) {
                                return ezpz_system_solve_batch_params_device(sys, x_dev, positions, n_param, par_dev, batch, cfg, x_dev, st_dev,
                                                                             mask_dev, log_dev, warn_cap, hipStreamPerThread);
                            });
}

}  // extern "C"
