// What the entries that take a `positions` list of driven constraints share on the host: the check of a list,
// and for ezpz_system_solve_batch_params and ezpz_system_sweep_params the one path behind both -- the request, the enqueue, the
// host form (driven.cpp) -- with the route launchers it calls, each in the translation unit that instantiates its kernels.
#pragma once
#include "system.hpp"

namespace ezpz {

// The check of a `positions` list for every entry that takes one, and the map from caller position to place in the list
// (kNoParamSlot: not driven).
int driven_slot_map(const EzpzSystem& s, const uint32_t* positions, size_t n_param, std::vector<uint32_t>& slot_of_pos);

// A list resolved once for the params entry, the sweep and ezpz_system_sweep_params_plan: the map, and the routes it takes.
struct DrivenRequest {
    std::vector<uint32_t> slot_of_pos;
    bool for_comp = false;      // the component interpreter (else the list-walk teams, or the fronts)
    uint32_t params_route = 0;  // EZPZ_PARAMS_ROUTE_* as read under launch_mu: checked again when the call takes the lock
    uint32_t sweep_route = 0;   // EZPZ_SWEEP_*
};
// (a list-walk route: the program is built, and a system on a grid team is declined -- its workgroups' sub-programs would each
// need their slice of the side array)
int driven_request(EzpzSystem* sys, const uint32_t* positions, size_t n_param, DrivenRequest& r);
// The device form of both entries behind their argument checks: steps == 0 a params call of `batch` systems, steps >= 1 `batch`
// sweeps of `steps` solves in one launch (n_param, and for a sweep batch, not zero).
// `guard`: the sweep is a guarded one (guarded_sweep.hip; a list-walk route that has a GRD build, steps >= 1) -- the guard's part of
// GuardedSolveArgs, whose SolveArgs part the enqueue fills as for every sweep.
struct GuardLaunch {
    const double* params0;
    double* params_reached;
    EzpzGuardStep* guard;
    double max_move, h_min;
    uint32_t max_attempts;
};
int driven_enqueue(EzpzSystem* sys, const DrivenRequest& r, const double* x0_dev, const uint32_t* positions, size_t n_param,
                   const double* params_dev, size_t steps, size_t batch, const EzpzConfig* cfg, double* x_out_dev, EzpzStatus* status_dev,
                   uint8_t* unsat_mask_dev, uint64_t* warn_log_dev, uint32_t warn_cap, hipStream_t stream,
                   const GuardLaunch* guard = nullptr);
// The host form of both: stages max(steps, 1) * batch rows in the system's scratch, runs `device_form` on them (values in place) on
// hipStreamPerThread, waits and reads back -- statuses first (a team timeout: EZPZ_ERR_HIP), the log cut to n_warnings per row.
using DrivenDeviceForm = std::function<int(double* x_dev, const double* params_dev, EzpzStatus* status_dev, uint8_t* mask_dev, uint64_t* log_dev)>;
int driven_host_form(EzpzSystem* sys, const double* x0, size_t n_param, const double* params, size_t steps, size_t batch, double* x_out,
                     EzpzStatus* status, uint8_t* unsat_mask, uint64_t* warn_log, uint32_t warn_cap, const DrivenDeviceForm& device_form);

// ---- the route launchers (launch_mu is held, the device current; a.params / par_slot / n_param set, a.steps for a sweep) -------
int list_walk_params_launch(EzpzSystem& s, SolveArgs& a, hipStream_t stream);                  // params.hip: the PAR builds
int list_walk_sweep_launch(EzpzSystem& s, SolveArgs& a, uint32_t route, hipStream_t stream);   // sweep.hip: the SWP builds
int list_walk_guarded_launch(EzpzSystem& s, GuardedSolveArgs& a, uint32_t route, hipStream_t stream);  // guarded_sweep.hip: the GRD builds
int comp_sweep_launch(EzpzSystem& s, const SolveArgs& a, hipStream_t stream);                  // sweep.hip: the interpreter's SWP builds
int front_params_launch(EzpzSystem& s, SolveArgs& a, bool sweep, hipStream_t stream);          // front_params.hip: PAR, or SWP
// (the interpreter's PAR builds: comp_launch of comp.hip with these arguments -- the one place that hands it the driven ones)
inline CompLaunch comp_driven_launch_args(const SolveArgs& a) {
    CompLaunch L = comp_launch_args(a);
    L.params = a.params;
    L.par_overlay = a.par_slot;
    L.n_param = a.n_param;
    return L;
}

// EZPZ_PARAMS_LDS=0: the teams read the driven values where the caller left them, whatever room their LDS has (A/B runs;
// tests/test_gpu_params.py runs that form in a child process).  EZPZ_DEBUG=params: which form a launch took, on stderr.
inline bool params_lds_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("EZPZ_PARAMS_LDS");
        return !(e && e[0] == '0');
    }();
    return on;
}
// (the params launches' line: the list-walk teams' -- `copies` of the values per workgroup -- or, copies == 0, the fronts')
void debug_params_line(const EzpzSystem& s, uint32_t n_param, bool in_lds, size_t copies, size_t lds_from, size_t lds_to);

// The teams' copies of their system's values: one per team of a workgroup of sub-wavefront teams, two for a wavefront-
// partitioned workgroup (its wavefronts may be a system apart), one for a barrier workgroup -- behind everything else in
// the LDS, when that costs the CU no workgroup it would otherwise hold; else the values stay where the caller left them
struct ParLds {
    bool in_lds;
    size_t copies, bytes;  // the launch's dynamic LDS
    uint32_t off;          // SolveArgs::par_lds_off
};
inline ParLds par_lds_plan(const EzpzSystem& s, size_t n_param) {
    const size_t copies = s.mode == MODE_SUB ? s.block_threads / s.team_size : s.mode == MODE_PART ? 2 : 1;
    const size_t base = (s.lds_bytes + 15) & ~size_t(15), with = base + copies * n_param * sizeof(double);
    auto per_cu = [&](size_t bytes) {
        const size_t cap = s.mode == MODE_SUB ? 4 : 8;  // (what the kernels' registers and launch_list_walk's grid ask of a CU at most)
        return std::min<size_t>(cap, s.lim.lds_bytes / std::max<size_t>(bytes, 1));
    };
    const bool in_lds = params_lds_enabled() && with <= s.lim.lds_bytes && per_cu(with) == per_cu(s.lds_bytes);
    return {in_lds, copies, in_lds ? with : s.lds_bytes, in_lds ? (uint32_t)(base / 8) : 0u};
}

// ---- the fronts as the route of both entries (front_params.hip; ezpz_system_set_params_route) ---------------------------------
// A workgroup's copy of its system's driven values: behind everything else in the LDS when that costs the CU no workgroup of the
// build (the occupancy the launch itself asks the runtime for), else -- and with EZPZ_PARAMS_LDS=0 -- the rows are read through L2.
struct FrontParLds {
    bool in_lds;
    uint32_t bytes;  // the launch's dynamic LDS
    uint32_t off;    // FrontArgs::par_lds_off
};
int front_params_lds_plan(EzpzSystem& s, size_t n_param, bool sweep, FrontParLds& out);  // (launch_mu is held, the device current)

}  // namespace ezpz
