// Batch solves whose systems bring their own constraint parameters (driven dimensions): ezpz_system_solve_batch_params and its
// device form.  One topology, `batch` dimension sets: params[b][j] replaces cs[positions[j]].param for system b.
//
// The route of this entry is its own: the component interpreter for a block system whose plan it can run
// (comp_kernel.hip.hpp, the PAR builds: a per-call overlay beside the chunks' parameter tables), else the list-walk teams on
// one workgroup per system or less (lm_kernel.hip.hpp, the PAR builds: instantiated here, beside launch.hip's).  Never the
// run-time compiled kernels -- lane, wavefront, block classes hold parameters as literals or stage them once per launch -- and
// never the lanes across the batch or the fronts, whose programs carry the parameters in their records: a system that has been
// specialised, or whose plain calls take those shapes, is still served from here.
#include "list_walk_launch.hip.hpp"

using namespace ezpz;

namespace {

// EZPZ_PARAMS_LDS=0: the teams read the driven values where the caller left them, whatever room their LDS has (A/B runs;
// tests/test_gpu_params.py runs that form in a child process).  EZPZ_DEBUG=params: which form a launch took, on stderr.
bool params_lds_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("EZPZ_PARAMS_LDS");
        return !(e && e[0] == '0');
    }();
    return on;
}

// What a `positions` list becomes on the device -- the list-walk teams' side array (per constraint of the table: its place in the
// list, or none) or the interpreter's overlay -- kept on the system for a caller that repeats its list.  (launch_mu is held.)
int driven_slots(EzpzSystem& s, const uint32_t* positions, size_t n_param, const std::vector<uint32_t>& slot_of_pos, bool for_comp) {
    EzpzSystem::DrivenParams& d = s.driven;
    if (d.valid && d.for_comp == for_comp && d.positions.size() == n_param && std::equal(positions, positions + n_param, d.positions.begin()))
        return EZPZ_OK;
    d.valid = false;
    std::vector<uint32_t> table;
    if (for_comp) {
        comp_param_overlay(*s.comp, slot_of_pos.data(), table);
    } else {
        table.resize(std::max<size_t>(s.host_con_pos.size(), 1), kNoParamSlot);
        for (size_t ci = 0; ci < s.host_con_pos.size(); ++ci) table[ci] = slot_of_pos[s.host_con_pos[ci]];
    }
    // (the launches that read the previous list's table have to be through with it: each waited for the one before it, so the
    // last one's completion is everybody's)
    if (d.uploaded) HIP_TRY(hipEventSynchronize(d.uploaded));
    int rc = d.slots.ensure(table.size());
    if (rc != EZPZ_OK) return rc;
    HIP_TRY(hipMemcpy(d.slots.p, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    d.positions.assign(positions, positions + n_param);
    d.for_comp = for_comp;
    d.valid = true;
    return EZPZ_OK;
}

int launch_params(EzpzSystem& s, SolveArgs& a, bool for_comp, hipStream_t stream) {
    if (for_comp) {
        CompLaunch L = comp_launch_args(a);
        L.params = a.params;
        L.par_overlay = a.par_slot;
        L.n_param = a.n_param;
        return comp_launch(*s.comp, s.dev_comp, L, s.device, s.lim.cus, s.lim.lds_bytes, stream);
    }
    // The teams' copies of their system's values: one per team of a workgroup of sub-wavefront teams, two for a wavefront-
    // partitioned workgroup (its wavefronts may be a system apart), one for a barrier workgroup -- behind everything else in
    // the LDS, when that costs the CU no workgroup it would otherwise hold; else the values stay where the caller left them
    const size_t copies = s.mode == MODE_SUB ? s.block_threads / s.team_size : s.mode == MODE_PART ? 2 : 1;
    const size_t base = (s.lds_bytes + 15) & ~size_t(15), with = base + copies * (size_t)a.n_param * sizeof(double);
    auto per_cu = [&](size_t bytes) {
        const size_t cap = s.mode == MODE_SUB ? 4 : 8;  // (what the kernels' registers and launch_list_walk's grid ask of a CU at most)
        return std::min<size_t>(cap, s.lim.lds_bytes / std::max<size_t>(bytes, 1));
    };
    const bool in_lds = params_lds_enabled() && with <= s.lim.lds_bytes && per_cu(with) == per_cu(s.lds_bytes);
    a.par_lds_off = in_lds ? (uint32_t)(base / 8) : 0u;
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
    const size_t n_cs = sys->host_has_param.size();
    std::vector<uint32_t> slot_of_pos(std::max<size_t>(n_cs, 1), kNoParamSlot);
    for (size_t j = 0; j < n_param; ++j) {
        const uint32_t pos = positions[j];
        if (pos >= n_cs || slot_of_pos[pos] != kNoParamSlot || !sys->host_has_param[pos]) return EZPZ_ERR_INVALID_ARGUMENT;
        slot_of_pos[pos] = (uint32_t)j;
    }
    const bool for_comp = sys->comp && sys->comp->interpretable;
    if (!for_comp) {
        if (int rc = ensure_program(sys)) return rc;
        // one system on several workgroups: declined (the workgroups' sub-programs would each need their slice of the side array)
        if (sys->mode != MODE_SUB && sys->grid_wgs > 1) return EZPZ_ERR_INVALID_ARGUMENT;
    }
    if (batch == 0) return EZPZ_OK;
    release_thread_kernel(sys->device);
    EZPZ_ON_DEVICE(sys->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
    if (int rc = driven_slots(*sys, positions, n_param, slot_of_pos, for_comp)) return rc;
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
