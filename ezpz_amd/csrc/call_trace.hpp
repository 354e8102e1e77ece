// Per-stage time stamps of one ezpz_solve call (diagnostic; tools/solve_call_breakdown.py).  The calling thread hands the
// library a buffer with ezpz_debug_call_trace; while it is set, every stage boundary of the one-call path appends an
// (id, CLOCK_MONOTONIC nanoseconds) pair.  Without a buffer a stamp is one thread-local load and a branch.
#pragma once
#include <time.h>

#include <cstddef>
#include <cstdint>

namespace ezpz {

enum CallStage : uint32_t {
    CALL_ENTER = 1,        // ezpz_solve entered
    CALL_PLAN = 2,         // request recognised (compare with the cached plan / scans + symbolic phase on a miss)
    CALL_SIDES = 3,        // sides inferred from the guesses, tier chosen
    CALL_LOCKED = 4,       // system lock + device selected
    CALL_STAGED = 5,       // guesses where the kernel reads them
    CALL_LAUNCHED = 6,     // kernel enqueued
    CALL_COMPLETE = 7,     // completion seen by the host
    CALL_UNPACKED = 8,     // values / status copied out of the staging buffers
    CALL_FINISHED = 9,     // unsatisfied list, warnings, outcome filled in
    CALL_RETURN = 10,
    // a request the process has not seen (or ezpz_cache_clear): the symbolic phase, between CALL_ENTER and CALL_SIDES
    COLD_PLAN_BUILT = 20,     // tiers, lint, validation (build_plan)
    COLD_ANALYSED = 21,       // analyze_into: components / classes / elimination order / lists (Model::new's counterpart)
    COLD_UPLOADED = 22,       // device allocations + program upload
    COLD_KERNEL_FOUND = 23,   // the specialised kernel's registry entry (source text compared)
    // ezpz_system_sweep_params_device (sweep.hip)
    SWEEP_TABLE_UPLOADED = 30,  // a `positions` list other than the system's last one: waited for earlier launches, copied its table
    SWEEP_LAUNCHED = 31,        // the one launch of the sweep enqueued
    // ezpz_system_redundancy_device (redundancy.hip)
    REDUNDANCY_PREPARED = 40,  // something blocking first: tables built, a focus list other than the last one's, a buffer that had to grow
    REDUNDANCY_LAUNCHED = 41,  // gather, evaluation and the analysis kernel enqueued
    REDUNDANCY_PLACED_LANE = 42,         // ... the analysis with one lane per (system, component)
    REDUNDANCY_PLACED_TEAM_LDS = 43,     // ... or one workgroup per system, its workspace in LDS
    REDUNDANCY_PLACED_TEAM_GLOBAL = 44,  // ... or in global memory
    // ezpz_system_measure_device and its siblings (measure.hip)
    MEASURE_TABLE_UPLOADED = 50,  // a record list other than the system's last one (or its CSR, first asked for): waited, packed, copied
    MEASURE_LAUNCHED = 51,        // the entry's kernels enqueued
    MEASURE_PLACED_ROW = 52,      // ... its measure launch staged the rows in LDS
    MEASURE_PLACED_DIRECT = 53,   // ... or gathered them from global memory
    // ezpz_system_tolerance_mc_device (tolerance_mc.hip), around the stamps of the entries its rounds are made of
    MC_TABLES_UPLOADED = 60,  // other distributions, limits or ranges than the last run's, or a workspace that had to grow: waited, copied
    MC_LAUNCHED = 61,         // every round of the run enqueued
    // ezpz_system_seek_targets_device (seek.hip), around the stamps of the entries its rounds are made of
    SEEK_TABLES_UPLOADED = 70,  // other tables than the last run's, or a workspace that had to grow: waited, copied
    SEEK_LAUNCHED = 71,         // every round of every chunk enqueued (the host form: run)
    // ezpz_branch_cluster_device and ezpz_system_solve_branches_device (branches.hip), the latter around the stamps of the solve entry
    BRANCH_TABLES_UPLOADED = 80,  // other compared variables or distributions than the last run's, or a workspace that had to grow: waited, copied
    BRANCH_LAUNCHED = 81,         // every round of the run enqueued
    // ezpz_mc_moments_device (mc_moments.hip)
    MOMENTS_WORKSPACE_GROWN = 90,  // a workspace that had to grow: waited for the last call's launches, allocated
    MOMENTS_LAUNCHED = 91,         // every round of the reduction enqueued
    // ezpz_mc_sobol_sums_device (mc_sobol.hip)
    SOBOL_WORKSPACE_GROWN = 100,  // a workspace that had to grow: waited for the last call's launches, allocated
    SOBOL_LAUNCHED = 101,         // every round of the reduction enqueued
    // ezpz_mc_quantiles_device (mc_quantiles.hip)
    QUANTILES_WORKSPACE_GROWN = 110,  // a workspace that had to grow: waited for the last call's launches, allocated
    QUANTILES_LAUNCHED = 111,         // every digit pass of the selection enqueued
    // ezpz_mc_effects_device (mc_effects.hip)
    EFFECTS_WORKSPACE_GROWN = 120,  // a workspace that had to grow: waited for the last call's launches, allocated
    EFFECTS_LAUNCHED = 121,         // every round of the reduction enqueued
    // ezpz_mc_factorial_device (mc_factorial.hip)
    FACTORIAL_WORKSPACE_GROWN = 130,  // a workspace that had to grow: waited for the last call's launches, allocated
    FACTORIAL_LAUNCHED = 131,         // the gather, the strided levels, the walk and the close enqueued
    // ezpz_sketch_image_device (sketch_image.hip)
    IMAGE_WORKSPACE_GROWN = 140,  // another item list than the last call's, or a workspace that had to grow: waited, copied
    IMAGE_LAUNCHED = 141,         // every round's two passes enqueued
};

struct CallTrace {
    uint64_t* buf = nullptr;
    size_t cap = 0, n = 0;
};
extern thread_local CallTrace t_call_trace;

inline void call_stamp(uint32_t id) {
    CallTrace& t = t_call_trace;
    if (__builtin_expect(t.buf != nullptr, 0) && t.n + 2 <= t.cap) {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        t.buf[t.n++] = id;
        t.buf[t.n++] = (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
    }
}

}  // namespace ezpz
