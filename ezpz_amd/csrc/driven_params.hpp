// What ezpz_system_solve_batch_params (params.hip) and ezpz_system_sweep_params (sweep.hip) share on the host: the device table a
// `positions` list becomes, kept on the system, and where the list-walk teams keep their system's driven values.
#pragma once
#include "system.hpp"

namespace ezpz {

// EZPZ_PARAMS_LDS=0: the teams read the driven values where the caller left them, whatever room their LDS has (A/B runs;
// tests/test_gpu_params.py runs that form in a child process).  EZPZ_DEBUG=params: which form a launch took, on stderr.
inline bool params_lds_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("EZPZ_PARAMS_LDS");
        return !(e && e[0] == '0');
    }();
    return on;
}

// What a `positions` list becomes on the device -- the list-walk teams' side array (per constraint of the table: its place in the
// list, or none) or the interpreter's overlay -- kept on the system for a caller that repeats its list.  (launch_mu is held.)
inline bool driven_slots_cached(const EzpzSystem& s, const uint32_t* positions, size_t n_param, bool for_comp, uint32_t route) {
    const EzpzSystem::DrivenParams& d = s.driven;
    return d.valid && d.for_comp == for_comp && d.route == route && d.positions.size() == n_param &&
           std::equal(positions, positions + n_param, d.positions.begin());
}
inline int driven_slots(EzpzSystem& s, const uint32_t* positions, size_t n_param, const std::vector<uint32_t>& slot_of_pos, bool for_comp,
                        uint32_t route = EZPZ_PARAMS_ROUTE_DEFAULT) {
    EzpzSystem::DrivenParams& d = s.driven;
    if (driven_slots_cached(s, positions, n_param, for_comp, route)) return EZPZ_OK;
    d.valid = false;
    std::vector<uint32_t> table;
    if (route == EZPZ_PARAMS_ROUTE_FRONTS) {
        table = slot_of_pos;  // (the fronts' records carry the caller's position: the map itself)
    } else if (for_comp) {
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
    d.route = route;
    d.valid = true;
    return EZPZ_OK;
}

// The request's argument checks and the map from caller position to place in the list (kNoParamSlot: not driven).
inline int driven_slot_map(const EzpzSystem& s, const uint32_t* positions, size_t n_param, std::vector<uint32_t>& slot_of_pos) {
    const size_t n_cs = s.host_has_param.size();
    slot_of_pos.assign(std::max<size_t>(n_cs, 1), kNoParamSlot);
    for (size_t j = 0; j < n_param; ++j) {
        const uint32_t pos = positions[j];
        if (pos >= n_cs || slot_of_pos[pos] != kNoParamSlot || !s.host_has_param[pos]) return EZPZ_ERR_INVALID_ARGUMENT;
        slot_of_pos[pos] = (uint32_t)j;
    }
    return EZPZ_OK;
}

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
// The launch: a.params / par_slot / n_param set; sweep: a.steps solves per sweep in one launch (the SWP build).
int front_params_launch(EzpzSystem& s, SolveArgs& a, bool sweep, hipStream_t stream);

}  // namespace ezpz
