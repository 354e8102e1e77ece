// Which instantiation of lm_solve_kernel a launch of a system on ONE workgroup per system (or less) takes: sub-wavefront teams,
// the wavefront-partitioned workgroup, the barrier workgroup with its workspace in LDS or in global memory, the record walk.
// Included by the four translation units that instantiate those kernels: launch.hip (PAR = false: every entry point but two),
// params.hip (PAR = true: ezpz_system_solve_batch_params, whose systems bring their own constraint parameters), sweep.hip
// (PAR and SWP: ezpz_system_sweep_params, a chain of such solves per system in one launch; `batch` counts sweeps there) and
// guarded_sweep.hip (GRD: ezpz_system_sweep_guarded, the sweep with step control in the team; no partitioned workgroup) -- the
// four sets of builds compile side by side.  (The caller holds the system's launch lock.)
#pragma once
#include "system.hpp"

#include "lm_kernel.hip.hpp"

namespace ezpz {

// `lds_bytes`: the launch's dynamic LDS -- the system's, plus the teams' parameter copies of a PAR launch.
// (ARGS: SolveArgs, or the guarded builds' GuardedSolveArgs -- guarded_sweep.hip, the one place that passes it)
template <bool PAR, bool SWP, int TEAM, int MODE, bool LDSWS, bool PLDS, bool LIN, bool DENSE = false, int REC = 0, class ARGS>
int launch_kernel(EzpzSystem& s, const ARGS& args, uint32_t grid, size_t lds_bytes, hipStream_t stream) {
    constexpr bool GRD = std::is_same<ARGS, GuardedSolveArgs>::value;
    auto kernel = lm_solve_kernel<TEAM, MODE, LDSWS, PLDS, LIN, false, DENSE, REC, PAR, SWP, GRD>;
    // hipFuncAttributeMaxDynamicSharedMemorySize belongs to the kernel, not to the system: raised once per kernel
    // build and device, to everything the device allows, so that systems of different sizes sharing a build never
    // lower each other's limit
    static std::atomic<bool> raised[16];
    if (lds_bytes > 48 * 1024 && !raised[s.device & 15].load(std::memory_order_acquire)) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)s.lim.lds_bytes));
        raised[s.device & 15].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(s.block_threads), lds_bytes, stream, args);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

// Every team shape comes in two builds: all 25 kinds, or the nine linear kinds only (`linear_only` topologies).
template <bool PAR, bool SWP, int TEAM, int MODE, bool LDSWS, bool PLDS, class ARGS>
int launch_variant(EzpzSystem& s, const ARGS& args, uint32_t grid, size_t lds_bytes, hipStream_t stream) {
    if (s.linear_only) return launch_kernel<PAR, SWP, TEAM, MODE, LDSWS, PLDS, true>(s, args, grid, lds_bytes, stream);
    return launch_kernel<PAR, SWP, TEAM, MODE, LDSWS, PLDS, false>(s, args, grid, lds_bytes, stream);
}

template <bool PAR, bool SWP, int TEAM, class ARGS>
int launch_sub(EzpzSystem& s, const ARGS& args, uint32_t grid, size_t lds_bytes, hipStream_t stream) {
    if constexpr (TEAM == 4) {  // <= 8 variables: dense factor layout, solved in registers (always staged)
        if (s.counts.dense)
            return s.linear_only ? launch_kernel<PAR, SWP, TEAM, MODE_SUB, true, true, true, true>(s, args, grid, lds_bytes, stream)
                                 : launch_kernel<PAR, SWP, TEAM, MODE_SUB, true, true, false, true>(s, args, grid, lds_bytes, stream);
    }
    return s.prog_in_lds ? launch_variant<PAR, SWP, TEAM, MODE_SUB, true, true>(s, args, grid, lds_bytes, stream)
                         : launch_variant<PAR, SWP, TEAM, MODE_SUB, true, false>(s, args, grid, lds_bytes, stream);
}

// The system's workspace in global memory -- the lanes kernel's, the list walk's when its workspace or its Jacobian lives there -- is
// one per system object: `launch` runs behind the last launch that used it, whatever stream that was, and leaves its own completion
// behind when it succeeds.
template <class Launch>
int on_workspace(EzpzSystem& s, hipStream_t stream, Launch&& launch) {
    HIP_TRY(s.lanes_done ? hipStreamWaitEvent(stream, s.lanes_done, 0) : hipEventCreateWithFlags(&s.lanes_done, hipEventDisableTiming));
    const int rc = launch();
    if (rc == EZPZ_OK) HIP_TRY(hipEventRecord(s.lanes_done, stream));
    return rc;
}

template <bool PAR, bool SWP = false, class ARGS>
int list_walk_one_workgroup(EzpzSystem& s, ARGS& args, size_t lds_bytes, hipStream_t stream) {
    constexpr bool GRD = std::is_same<ARGS, GuardedSolveArgs>::value;
    if constexpr (GRD) {  // (no guarded build of the partitioned workgroup: its wavefronts are an item apart)
        if (s.mode == MODE_PART) return EZPZ_ERR_INVALID_ARGUMENT;
    }
    uint32_t grid;
    if (s.mode == MODE_SUB) {
        const uint32_t tpb = s.block_threads / s.team_size;
        uint64_t blocks = (args.batch + tpb - 1) / tpb;
        grid = (uint32_t)std::min<uint64_t>(blocks, (uint64_t)s.lim.cus * 32);
        switch (s.team_size) {
        case 1: return launch_sub<PAR, SWP, 1>(s, args, grid, lds_bytes, stream);
        case 2: return launch_sub<PAR, SWP, 2>(s, args, grid, lds_bytes, stream);
        case 4: return launch_sub<PAR, SWP, 4>(s, args, grid, lds_bytes, stream);
        case 8: return launch_sub<PAR, SWP, 8>(s, args, grid, lds_bytes, stream);
        case 16: return launch_sub<PAR, SWP, 16>(s, args, grid, lds_bytes, stream);
        case 32: return launch_sub<PAR, SWP, 32>(s, args, grid, lds_bytes, stream);
        default: return launch_sub<PAR, SWP, 64>(s, args, grid, lds_bytes, stream);
        }
    }
    const uint32_t per_cu = s.lds_ws ? (uint32_t)std::max<size_t>(1, s.lim.lds_bytes / std::max<size_t>(lds_bytes, 1))
                                     : 2048u / s.block_threads;
    // Workgroups: twice what the device holds at once where a workgroup serves several systems side by side (sub-wavefront teams)
    // or owns a workspace in global memory; a workgroup per system -- up to 32 times what the device holds -- where it solves one
    // system at a time in its LDS: the dispatcher then hands a free place the next system, whatever the systems before it took
    // (a jittered batch's systems take 4 to 10 iterations) and whoever else occupies places on the device -- sketch150 x 32 768
    // at x1 / x2 / x4 / x8 / x32: 3.58 / 3.62 / 3.70 / 3.82 / 3.91 M solves/s; starting a workgroup costs a few microseconds
    // against the ~250 of a system.
    // (a list of systems on the device -- the lanes' stragglers: `batch` is the list's capacity, the systems are a few hundred)
    const uint32_t rounds = (s.lds_ws && s.mode != MODE_SUB && !args.sys_list) ? 32u : 2u;
    grid = (uint32_t)std::min<uint64_t>(args.batch, (uint64_t)s.lim.cus * std::min<uint32_t>(per_cu, 8) * rounds);
    if (s.rec && s.rec_jglobal)  // (a workgroup's Jacobian values in global memory: at most 256 MiB of them per system object)
        grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(grid, (1ull << 25) / ((s.counts.zj + 2) & ~1ull)));
    if (!s.lds_ws) {
        // the workspace in global memory is one per system object (like the lanes kernel's)
        int rc = s.gws_dev.ensure((size_t)grid * s.ws_doubles);
        if (rc != EZPZ_OK) return rc;
        args.gws = s.gws_dev.p;
        return on_workspace(s, stream, [&] {
            if constexpr (!GRD) {
                if (s.mode == MODE_PART) return launch_variant<PAR, SWP, 64, MODE_PART, false, false>(s, args, grid, lds_bytes, stream);
            }
            return !s.rec              ? launch_variant<PAR, SWP, 64, MODE_WGB, false, false>(s, args, grid, lds_bytes, stream)
                   : s.linear_only     ? launch_kernel<PAR, SWP, 64, MODE_WGB, false, false, true, false, 2>(s, args, grid, lds_bytes, stream)
                                       : launch_kernel<PAR, SWP, 64, MODE_WGB, false, false, false, false, 2>(s, args, grid, lds_bytes, stream);
        });
    }
    const bool staged = s.prog_in_lds;
    if constexpr (!GRD) {
        if (s.mode == MODE_PART)
            return staged ? launch_variant<PAR, SWP, 64, MODE_PART, true, true>(s, args, grid, lds_bytes, stream)
                          : launch_variant<PAR, SWP, 64, MODE_PART, true, false>(s, args, grid, lds_bytes, stream);
    }
    if (!s.rec)
        return staged ? launch_variant<PAR, SWP, 64, MODE_WGB, true, true>(s, args, grid, lds_bytes, stream)
                      : launch_variant<PAR, SWP, 64, MODE_WGB, true, false>(s, args, grid, lds_bytes, stream);
    // one connected system, its linear solve as a record walk
    auto walk = [&] {
        if (s.linear_only)
            return staged ? launch_kernel<PAR, SWP, 64, MODE_WGB, true, true, true, false, 1>(s, args, grid, lds_bytes, stream)
                          : launch_kernel<PAR, SWP, 64, MODE_WGB, true, false, true, false, 1>(s, args, grid, lds_bytes, stream);
        return staged ? launch_kernel<PAR, SWP, 64, MODE_WGB, true, true, false, false, 1>(s, args, grid, lds_bytes, stream)
                      : launch_kernel<PAR, SWP, 64, MODE_WGB, true, false, false, false, 1>(s, args, grid, lds_bytes, stream);
    };
    if (!s.rec_jglobal) return walk();
    // the Jacobian's values of every workgroup in global memory: one array per system object, like the workspace
    int rc = s.gws_dev.ensure((size_t)grid * ((s.counts.zj + 2) & ~1u));
    if (rc != EZPZ_OK) return rc;
    args.gws = s.gws_dev.p;
    return on_workspace(s, stream, walk);
}

}  // namespace ezpz
