// What the launches of the FRONTAL shape share (front.hip: the plain and the probe launch; front_params.hip: the PAR and SWP
// builds): the kernel's argument block from a launch's SolveArgs and the system's plan, and the launch itself -- persistent
// workgroups for systems on one workgroup, as many resident slots as the device holds for systems on several.
#pragma once
#include "system.hpp"

#include "front_kernel.hip.hpp"

namespace ezpz {

// What a probe launch adds to a solve launch (FrontArgs::probe_*).
struct FrontProbe {
    uint32_t m = 0;
    double* out = nullptr;
    const double* in = nullptr;
    double scale = 1e-11;
};

inline FrontArgs front_args_for(const EzpzSystem& s, SolveArgs& args, const FrontProbe& probe) {
    const FrontPlan& plan = *s.fronts;
    FrontArgs fa{};
    fa.plan = static_cast<const unsigned char*>(s.dev_fronts);
    fa.n_wgs = plan.n_wgs;
    fa.n_vars = plan.n_vars;
    fa.n_cons = plan.n_cons;
    fa.x0 = args.x0;
    fa.x_out = args.x_out;
    fa.status = args.status;
    fa.unsat_mask = args.unsat_mask;
    fa.warn_log = args.warn_log;
    fa.warn_cap = args.warn_cap;
    fa.max_iterations = args.max_iterations;
    fa.batch = args.batch;
    fa.residual_tolerance = args.residual_tolerance;
    fa.step_tolerance = args.step_tolerance;
    fa.initial_lambda = args.initial_lambda;
    fa.unit_weights = plan.unit_weights ? 1u : 0u;
    fa.tab_lds_bytes = (plan.tab_bytes_max + 15u) & ~15u;
    fa.ws_doubles = plan.ws_doubles_max;
    fa.n_chunks = plan.n_chunks;
    fa.bad_chunk0 = plan.bad_chunk0;
    fa.verdict_chunk = plan.verdict_chunk;
    fa.scratch = nullptr;
    fa.scratch_stride = 0;
    fa.probe_m = probe.m;  // (front_launch_probe)
    fa.probe_out = probe.out;
    fa.probe_in = probe.in;
    fa.probe_scale = probe.scale;
    fa.stamps = args.stamps;
    fa.done = args.done;
    fa.done.request = nullptr;  // (this kernel does not stay resident between calls)
    args.done.request = nullptr;
    return fa;
}

// Workgroups of `kernel` a CU holds with `lds_bytes` of dynamic LDS.  (Runtime calls that cost more than a small solve: callers keep the answer.)
template <class K>
int front_per_cu(const EzpzSystem& s, K kernel, size_t lds_bytes, int& per_cu) {
    const FrontPlan& plan = *s.fronts;
    if (lds_bytes > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lim.lds_bytes));
    per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)plan.threads, lds_bytes));
    return EZPZ_OK;
}

// The launch: `capacity` workgroups of this kernel fit the device, `slots_wanted` work items can run side by side (systems, or
// sweeps), `items` is what the launch works through in all (the budget of the scratch's sequence numbers).
template <class K, class ARGS>
int front_launch_on(EzpzSystem& s, K kernel, ARGS& fa, uint64_t capacity, size_t lds_bytes, uint64_t slots_wanted, uint64_t items,
                    hipStream_t stream) {
    const FrontPlan& plan = *s.fronts;
    const uint32_t G = plan.n_wgs;
    if (G == 1) {
        // persistent workgroups: a few per CU's worth of the batch
        const uint32_t grid = (uint32_t)std::min<uint64_t>(slots_wanted, capacity * 2);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(plan.threads), lds_bytes, stream, fa);
        HIP_TRY(hipGetLastError());
        return EZPZ_OK;
    }
    if (capacity < G) return EZPZ_ERR_TOO_LARGE;
    const uint32_t slots = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(slots_wanted, capacity / G));
    const uint32_t stride = front_scratch_bytes(plan.n_chunks);
    if (s.front_scratch.cap < (size_t)slots * stride) {
        int rc = s.front_scratch.ensure((size_t)slots * stride);
        if (rc != EZPZ_OK) return rc;
        HIP_TRY(hipMemsetAsync(s.front_scratch.p, 0, s.front_scratch.cap, stream));
    }
    fa.scratch = s.front_scratch.p;
    fa.scratch_stride = stride;
    fa.done.request = nullptr;
    // (slots x G never exceeds what the device holds: launch_resident.  Per LM iteration a factorisation's hops up and down the tree and the reductions of the LM control -- at most a few per level;
    // the sequence numbers of the scratch start again before they wrap: system.hpp)
    return launch_resident(s.device, stream, s.front_scratch.p, s.front_scratch.cap, s.front_seq_used, items,
                           16ull * ((uint64_t)fa.max_iterations + 4) * std::max<uint32_t>(1, plan.n_levels), [&] {
                               hipLaunchKernelGGL(kernel, dim3(slots * G), dim3(plan.threads), lds_bytes, stream, fa);
                               HIP_TRY(hipGetLastError());
                               return EZPZ_OK;
                           });
}

}  // namespace ezpz
