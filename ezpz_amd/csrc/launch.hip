// Kernel dispatch: which instantiation of lm_solve_kernel / which component, lane or specialised kernel a launch of an
// EzpzSystem takes (launch), the device-pointer entry point of the C ABI and the evaluation-only kernel.  The only
// translation unit that instantiates the list-walk / record-walk kernels (lm_kernel.hip.hpp).
#include "system.hpp"

#include "list_walk_launch.hip.hpp"

using namespace ezpz;

namespace {

std::mutex g_grid_mu;
hipEvent_t g_grid_event[16] = {};  // per device: completion of the last launch of this process whose workgroups wait for each other

}  // namespace
namespace ezpz {
thread_local uint64_t t_call_batch = 0;

// Every workgroup of the launch must become resident (they wait for each other).  The launch never asks for more than the device
// holds, and such launches of this process are chained on one event per device, so two of them are never half-resident at the same
// time whatever streams they were enqueued on; other kernels only delay residency.  (hipLaunchCooperativeKernel gives the same
// guarantee across processes but costs 21 us per launch, more than a third of a 200 000-variable solve; another process running
// them on the same device at the same time is not supported.)
int launch_resident(int device, hipStream_t stream, void* scratch, size_t scratch_bytes, uint64_t& seq_used, uint64_t batch,
                    uint64_t exchanges_per_system, const std::function<int()>& launch) {
    std::lock_guard<std::mutex> lock(g_grid_mu);
    hipEvent_t& ev = g_grid_event[device & 15];
    HIP_TRY(ev ? hipStreamWaitEvent(stream, ev, 0) : hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (seq_budget_spent(seq_used, batch, exchanges_per_system)) HIP_TRY(hipMemsetAsync(scratch, 0, scratch_bytes, stream));
    const int rc = launch();
    if (rc != EZPZ_OK) return rc;
    HIP_TRY(hipEventRecord(ev, stream));
    return EZPZ_OK;
}

// Launches of one system that share device state -- the counters its workgroups draw their systems from, the redo lists of its
// `_fast` entry, whose count a call's last launch zeroes for the NEXT call -- run one after the other whatever streams they are
// enqueued on: a launch on another stream than the last one waits for everything enqueued there.  (An event per launch instead cost the
// back-to-back launches of one stream two runtime calls and a barrier packet each.)
bool JitLaunchState::chain(hipStream_t on) {
    bool ok = true;
    if (!done) ok = hipEventCreateWithFlags(&done, hipEventDisableTiming) == hipSuccess;
    if (ok && used && stream != on) {
        ok = hipEventRecord(done, stream) == hipSuccess && hipStreamWaitEvent(on, done, 0) == hipSuccess;
        if (!ok) {  // (the old stream is gone: whatever ran on it is awaited the blunt way)
            (void)hipGetLastError();
            ok = hipDeviceSynchronize() == hipSuccess;
        }
    }
    if (!ok) (void)hipGetLastError();
    return ok;
}

bool JitLaunchState::tickets(hipStream_t on) {
    // (a launch that is being recorded into a graph keeps fixed shares: a replay would find the counters elsewhere)
    if (stream_capturing(on)) return false;
    bool ok = ticket.p != nullptr;
    if (!ok && ticket.ensure(8 * 1024) == EZPZ_OK) {  // (jit_kernel.hip.hpp: kTicketStride words apart)
        ok = hipMemset(ticket.p, 0, 8 * 1024 * sizeof(unsigned int)) == hipSuccess;
        for (unsigned int& b : ticket_base) b = 0;
    }
    ok = ok && chain(on);
    if (!ok) (void)hipGetLastError();
    return ok;
}

int JitLaunchState::redo_lists(uint64_t batch, hipStream_t on) {
    for (auto& list : redo)
        if (list.cap < batch + 1) {
            int rc = list.ensure(batch + 1);  // (synchronises the device: nobody reads the old one any more)
            if (rc != EZPZ_OK) return rc;
            HIP_TRY(hipMemsetAsync(list.p, 0, sizeof(unsigned int), on));
        }
    if (!redo_seen) {
        HIP_TRY(hipHostMalloc((void**)&redo_seen, sizeof(unsigned int), hipHostMallocMapped));
        *redo_seen = 0;
        HIP_TRY(hipHostGetDevicePointer((void**)&redo_seen_dev, redo_seen, 0));
    }
    return EZPZ_OK;
}

void JitLaunchState::commit(const JitEnqueued& e, uint64_t batch, hipStream_t on) {
    // What a kernel of `wgs` workgroups over `batch` systems has drawn from each counter: counter c hands out its share of the systems
    // beyond the workgroups' own, and `in_vain` values more to each of its workgroups (the loop draws once per system it solves, the
    // last time in vain; `_fast` asks for its guesses a system ahead: twice in vain)
    auto advance = [&](const JitEnqueued::Kernel& k, unsigned int in_vain) {
        if (!k.tickets) return;
        for (uint64_t c = 0; c < 8; ++c) {
            const uint64_t wgs_c = (k.wgs + 7 - c) / 8, beyond = batch - k.wgs;
            ticket_base[c] += (unsigned int)(in_vain * wgs_c + (beyond > c ? (beyond - c + 7) / 8 : 0));
        }
    };
    advance(e.fast, 2);
    advance(e.loop, 1);
    if (e.fast.ran) turn ^= 1u;  // (the next call's list is the one this call's loop has zeroed)
    if (e.fast.ran || e.loop.tickets) stream = on, used = true;
}

int JitLaunchState::resync(hipStream_t on) {
    if (ticket.p) HIP_TRY(hipMemsetAsync(ticket.p, 0, ticket.cap * sizeof(unsigned int), on));
    for (auto& list : redo)
        if (list.p) HIP_TRY(hipMemsetAsync(list.p, 0, sizeof(unsigned int), on));
    for (unsigned int& b : ticket_base) b = 0;
    turn = 0;
    stream = on, used = true;  // (a launch on another stream waits for the zeroing: chain)
    return EZPZ_OK;
}

}  // namespace ezpz
namespace {

// Grid team: G workgroups per system, all of a launch's workgroups resident at once, as many systems in flight as
// the device holds.
template <bool LIN>
int launch_grid_kernel(EzpzSystem& s, SolveArgs& args, hipStream_t stream) {
    if (stream_capturing(stream)) return EZPZ_ERR_INVALID_ARGUMENT;  // (launch_resident)
    auto kernel = lm_solve_kernel<64, MODE_PART, true, true, LIN, true>;
    if (s.grid_capacity == 0) {  // once per system: these two runtime calls cost more than the solve
        if (s.lds_bytes > 48 * 1024)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lim.lds_bytes));
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)s.block_threads, s.lds_bytes));
        s.grid_capacity = (uint64_t)s.lim.cus * (uint64_t)std::max(per_cu, 1);
    }
    const uint64_t capacity = s.grid_capacity;
    if (capacity < s.grid_wgs) return EZPZ_ERR_TOO_LARGE;
    const uint32_t slots = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(args.batch, capacity / s.grid_wgs));
    int rc;
    if (!s.dev_grid_blob) {  // first launch: the workgroups' sub-programs and their views
        HIP_TRY(hipMalloc(&s.dev_grid_blob, s.grid_blob.size()));
        HIP_TRY(hipMemcpy(s.dev_grid_blob, s.grid_blob.data(), s.grid_blob.size(), hipMemcpyHostToDevice));
        std::vector<ProgramView> views = s.host_grid_views;
        for (ProgramView& pv : views) {
            pv.base = static_cast<const unsigned char*>(s.dev_grid_blob) + pv.blob_bytes;
            pv.blob_bytes = 0;
        }
        if ((rc = s.grid_views.ensure(views.size())) != EZPZ_OK) return rc;
        HIP_TRY(hipMemcpy(s.grid_views.p, views.data(), views.size() * sizeof(ProgramView), hipMemcpyHostToDevice));
    }
    if (s.grid_scratch.cap < slots) {
        if ((rc = s.grid_scratch.ensure(slots)) != EZPZ_OK) return rc;
        HIP_TRY(hipMemsetAsync(s.grid_scratch.p, 0, s.grid_scratch.cap * sizeof(GridScratch), stream));
    }
    args.grid_scratch = s.grid_scratch.p;
    args.grid_views = s.grid_views.p;
    args.grid_wgs = s.grid_wgs;
    // (three exchanges per LM iteration and a few around them; the sequence numbers start again before they wrap: system.hpp)
    return launch_resident(s.device, stream, s.grid_scratch.p, s.grid_scratch.cap * sizeof(GridScratch), s.grid_seq_used, args.batch,
                           3ull * ((uint64_t)args.max_iterations + 4), [&] {
                               hipLaunchKernelGGL(kernel, dim3(slots * s.grid_wgs), dim3(s.block_threads), s.lds_bytes, stream, args);
                               HIP_TRY(hipGetLastError());
                               return EZPZ_OK;
                           });
}

// The specialised kernel of a block system with the state its launches share (JitLaunchState): the host's totals follow what went
// out.  A call that went out only in part leaves the device's counters and redo counts zeroed behind it, for the fallback and the
// calls after it.
int jit_launch(EzpzSystem& s, const CompLaunch& L, hipStream_t stream, uint32_t grid_slots, uint32_t fast_slots) {
    const JitEnqueued e = comp_jit_launch(s.jit, *s.comp, s.dev_comp, L, s.device, s.lim.cus, stream, s.jit_state, grid_slots, fast_slots);
    if (e.rc == EZPZ_OK)
        s.jit_state.commit(e, L.batch, stream);
    else if ((e.fast.ran || e.loop.ran) && s.jit_state.resync(stream) != EZPZ_OK)
        return EZPZ_ERR_HIP;
    return e.rc;
}

// The class-specialised kernel of a system spread over several workgroups (CompPlan::jit_wgs > 1): as many systems in
// flight as the device holds whole teams of; every workgroup of the launch must be resident (launch_resident).
int launch_jit_grid(EzpzSystem& s, CompLaunch L, hipStream_t stream) {
    if (stream_capturing(stream)) return EZPZ_ERR_INVALID_ARGUMENT;  // (launch_resident)
    L.done.request = nullptr;  // (several workgroups per system: never resident)
    JitLaunchState& js = s.jit_state;
    const uint32_t G = s.comp->jit_wgs;
    const uint64_t capacity = comp_jit_capacity(s.jit, *s.comp, s.device, s.lim.cus);
    if (capacity < G) return EZPZ_ERR_TOO_LARGE;
    const uint32_t slots = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(L.batch, capacity / G));
    // (a linear system: the kernel that does not wait for its verdicts goes first -- leaner, so more systems in flight -- and the
    // loop solves what it lists)
    const uint32_t fast_slots = (uint32_t)(comp_jit_capacity_fast(s.jit, *s.comp, s.device, s.lim.cus) / G);
    const uint32_t most = std::max(slots, fast_slots);
    if (js.scratch.cap < (size_t)most * kJitGridScratchBytes) {
        // (sized for the device, not the call: a later, larger call must find the sequence numbers the slots have reached)
        const uint32_t all = (uint32_t)std::max<uint64_t>(most, std::max<uint64_t>(capacity / G, fast_slots));
        int rc = js.scratch.ensure((size_t)all * kJitGridScratchBytes);
        if (rc != EZPZ_OK) return rc;
        HIP_TRY(hipMemsetAsync(js.scratch.p, 0, js.scratch.cap, stream));
    }
    const bool lists = fast_slots && comp_jit_fast_ok(s.jit, *s.comp, L, s.device, s.lim.cus) && !stream_capturing(stream);
    if (lists) {
        int rc = js.redo_lists(L.batch, stream);
        if (rc != EZPZ_OK) return rc;
    }
    // (the loop's three exchanges per LM iteration, the ring's one per system: the sequence numbers start again before they wrap)
    return launch_resident(s.device, stream, js.scratch.p, js.scratch.cap, js.seq_used, L.batch, 3ull * ((uint64_t)L.max_iterations + 4),
                           [&] { return jit_launch(s, L, stream, slots, lists ? fast_slots : 0); });
}


// The list-walk teams of a system (lm_kernel.hip.hpp), whatever their shape: sub-wavefront teams, workgroups with their
// workspace in LDS or in global memory, grid teams.  (launch() holds the system's launch lock.)
int launch_list_walk(EzpzSystem& s, SolveArgs& args, hipStream_t stream) {
    // a resident launch (DoneWord::request) is one workgroup that keeps nothing another launch of this system waits for:
    // not a grid team, not a shape whose workspace or Jacobian lives in the system's one global scratch
    if (s.grid_wgs > 1 || args.batch != 1 || (s.mode != MODE_SUB && (!s.lds_ws || (s.rec && s.rec_jglobal)))) args.done.request = nullptr;
    if (s.mode != MODE_SUB && s.grid_wgs > 1) {
        // (a grid team starts every system from its guesses: its shared warning counter has no resumed value)
        if (args.resume) return EZPZ_ERR_INVALID_ARGUMENT;
        return s.linear_only ? launch_grid_kernel<true>(s, args, stream) : launch_grid_kernel<false>(s, args, stream);
    }
    return list_walk_one_workgroup<false>(s, args, s.lds_bytes, stream);
}

// launch() asks its routes in turn; each serves the call (EZPZ_OK), fails it (an error), or leaves it to the next (kNextRoute).
constexpr int kNextRoute = 1;

// A device-filling batch of one connected sketch: lanes across the batch (batch_kernel.hip.hpp).
int route_lanes(EzpzSystem& s, SolveArgs& args, hipStream_t stream) {
    constexpr uint64_t kNoLanesWorkspace = ~0ull;  // the allocation failed once: not tried again on every call
    if (!s.lanes || args.batch < s.lanes_min) return kNextRoute;
    args.done.request = nullptr;
    if (s.lanes_ws_waves == 0) {
        // one workspace per wavefront the device holds (capped at 24 GiB of the 288: fewer wavefronts then)
        uint64_t waves = batch_launch_waves(s.lim.cus);
        const uint64_t per = (uint64_t)s.lanes->rows * 512;
        while (waves > 4 && waves * per > (24ull << 30)) waves /= 2;
        s.lanes_ws_waves = s.lanes_ws.ensure((size_t)(waves * per / 8)) == EZPZ_OK ? waves : kNoLanesWorkspace;
    }
    if (s.lanes_ws_waves == kNoLanesWorkspace) return kNextRoute;
    int teams = EZPZ_OK;
    const int rc = on_workspace(s, stream, [&]() -> int {
        // the systems the lanes give up (stragglers, batch_kernel.hip.hpp) are listed on the device and resumed by this
        // system's list-walk teams right after: an indirect batch whose count stays on the device
        // (room for every wavefront handing over its threshold's worth of lanes once: a list that overflows leaves the lanes their tail)
        const uint64_t strag_most = std::min<uint64_t>(s.lanes_ws_waves, (args.batch + 63) / 64) * batch_straggler_lanes();
        const uint32_t strag_cap = args.batch < (1ull << 32) && args.batch >= 256 && strag_most
                                       ? (uint32_t)std::min<uint64_t>(args.batch, std::max<uint64_t>(4096, strag_most)) : 0u;
        bool list_ok = strag_cap && s.strag_list.ensure(strag_cap) == EZPZ_OK && s.strag_count.ensure(1) == EZPZ_OK &&
                       s.strag_state.ensure(strag_cap) == EZPZ_OK;
        if (list_ok && hipMemsetAsync(s.strag_count.p, 0, sizeof(uint32_t), stream) != hipSuccess) {
            (void)hipGetLastError();
            list_ok = false;
        }
        if (batch_launch(*s.lanes, s.dev_lanes, s.lanes_ws.p, s.lanes_ws_waves, s.counts.n_cons, comp_launch_args(args), stream,
                         list_ok ? s.strag_list.p : nullptr, list_ok ? s.strag_count.p : nullptr, list_ok ? strag_cap : 0u,
                         list_ok ? s.strag_state.p : nullptr) != EZPZ_OK)
            return kNextRoute;
        if (list_ok) {
            args.sys_list = s.strag_list.p;
            args.sys_count = s.strag_count.p;
            args.resume = s.strag_state.p;  // (the teams go on from the values the lanes left in x_out)
            args.batch = strag_cap;
            teams = launch_list_walk(s, args, stream);
        }
        return EZPZ_OK;  // (recorded after the teams: the next launch of this system, on whatever stream, resets the list's count)
    });
    return rc == EZPZ_OK ? teams : rc;
}

// One connected sketch as a tree of dense fronts (fronts.cpp): every call of a system created for one solve, the small calls of a
// system created for batches.
int route_fronts(EzpzSystem& s, SolveArgs& args, hipStream_t stream) {
    if (!s.fronts || args.resume || args.sys_list || (t_call_batch ? t_call_batch : args.batch) > s.front_max_batch) return kNextRoute;
    // (a launch that is being recorded into a graph: fronts on several workgroups allocate and zero their scratch on first use and
    // chain their launches on the process-wide event of launch_resident -- neither may end up inside a capture, which would also
    // leave that event unusable for the launches after it.  A system created for batches has its other shapes and takes them; a
    // system the fronts alone serve says so)
    if (s.fronts->n_wgs > 1 && stream_capturing(stream)) return s.front_max_batch == 0xFFFFFFFFu ? EZPZ_ERR_INVALID_ARGUMENT : kNextRoute;
    return front_launch(s, args, stream);
}

// One solve (or a few) of a small system built for latency: one wavefront per system, sweeps and assembly across its lanes
// (jit_kernel.hip.hpp: wave_kernel), compiled like the lane kernel.
int route_wave_jit(EzpzSystem& s, SolveArgs& args, hipStream_t stream) {
    if (!s.lane || !s.wave_jit || args.batch > (uint64_t)s.lim.cus) return kNextRoute;
    if (s.launches.load(std::memory_order_relaxed) == 0) comp_jit_probe(s.wave_jit);
    int st = comp_jit_state(s.wave_jit);
    if (st == 0 && (jit_sync() || s.launches.load(std::memory_order_relaxed) >= s.lim.policy.jit_after_launches)) st = comp_jit_request(s.wave_jit, jit_sync());
    return st == 2 && wave_jit_launch(s.wave_jit, *s.lane, comp_launch_args(args), s.device, s.lim.cus, stream) == EZPZ_OK ? EZPZ_OK : kNextRoute;
}

// A small system: one lane per system once the specialised kernel is compiled.
int route_lane_jit(EzpzSystem& s, SolveArgs& args, hipStream_t stream) {
    if (!s.lane || !s.jit) return kNextRoute;
    int st = comp_jit_state(s.jit);
    const EzpzLaunchPolicy& pol = s.lim.policy;
    if (st == 0 && (args.batch >= pol.jit_lane_min_batch || jit_sync() || s.launches.fetch_add(1) >= pol.jit_after_launches))
        st = comp_jit_request(s.jit, jit_sync());
    return st == 2 && lane_jit_launch(s.jit, *s.lane, comp_launch_args(args), s.device, s.lim.cus, stream) == EZPZ_OK ? EZPZ_OK : kNextRoute;
}

// A block system's compiled kernel in one of its three forms; anything but EZPZ_OK leaves the call to the interpreter.
int launch_block_jit(EzpzSystem& s, SolveArgs& args, const CompLaunch& L, hipStream_t stream) {
    if (s.comp->jit_wgs > 1) {
        const int rc = launch_jit_grid(s, L, stream);
        if (rc == EZPZ_OK) args.done.request = nullptr;
        return rc;
    }
    JitLaunchState& js = s.jit_state;
    if (comp_jit_fast_ok(s.jit, *s.comp, L, s.device, s.lim.cus) && !stream_capturing(stream) && js.redo_lists(L.batch, stream) == EZPZ_OK &&
        js.chain(stream)) {
        // a linear system: the kernel that does not wait for the LM control's verdicts, then the loop over the systems it lists
        // (jit_kernel.hip.hpp: solve_kernel_fast).  Never inside a capture: the redo list is zeroed by the NEXT call's launches,
        // which a replay does not run
        const uint32_t fast_slots = (uint32_t)std::min<uint64_t>(comp_jit_capacity_fast(s.jit, *s.comp, s.device, s.lim.cus), 0xFFFFFFFFull);
        return jit_launch(s, L, stream, 0, fast_slots);
    }
    return jit_launch(s, L, stream, 0, 0);  // the loop alone
}

// Many small components in few classes: the class-specialised kernel once it is compiled -- large batches start its compilation
// (background thread) -- else one lane per component on the interpreter (comp_kernel.hip.hpp).
int route_blocks(EzpzSystem& s, SolveArgs& args, hipStream_t stream) {
    if (!s.comp) return kNextRoute;
    const CompLaunch L = comp_launch_args(args);
    if (s.jit) {
        const bool sync = jit_sync();
        int st = comp_jit_state(s.jit);
        const EzpzLaunchPolicy& pol = s.lim.policy;
        const bool big = args.batch >= pol.jit_comp_min_batch || args.batch * (uint64_t)s.counts.n_vars >= pol.jit_comp_min_values;
        if (st == 0 && (big || sync || s.launches.fetch_add(1) >= pol.jit_after_launches)) st = comp_jit_request(s.jit, sync);
        if (st == 2 && launch_block_jit(s, args, L, stream) == EZPZ_OK) return EZPZ_OK;
    }
    if (s.comp->interpretable) return comp_launch(*s.comp, s.dev_comp, L, s.device, s.lim.cus, s.lim.lds_bytes, stream);
    return kNextRoute;  // (a system too large for the interpreter's LDS state: the list-walk grid team until the compiled kernel is ready)
}

int launch(EzpzSystem& s, SolveArgs& args, hipStream_t stream) {
    if (args.batch == 0) return EZPZ_OK;
    // enqueueing on one EzpzSystem from several threads (each on its own stream) is allowed: what a launch creates on
    // first use -- workspaces, events, occupancy figures -- is created under this lock, and launches that share a
    // workspace are chained on an event
    std::lock_guard<std::mutex> launch_lock(s.launch_mu);
    if (args.batch != 1) args.done.request = nullptr;  // (residency is for one-call launches: one system, one workgroup)
    int rc = route_lanes(s, args, stream);
    if (rc == kNextRoute) rc = route_fronts(s, args, stream);
    if (rc != kNextRoute) return rc;
    if (s.jit && s.launches.load(std::memory_order_relaxed) == 0) comp_jit_probe(s.jit);  // the kernel may be in the on-disk cache
    for (auto route : {route_wave_jit, route_lane_jit, route_blocks})
        if ((rc = route(s, args, stream)) != kNextRoute) return rc;
    return launch_list_walk(s, args, stream);
}

void fill_cfg(SolveArgs& a, const EzpzConfig* cfg) {
    EzpzConfig d;
    ezpz_default_config(&d);
    if (!cfg) cfg = &d;
    a.max_iterations = (uint32_t)std::min<uint64_t>(cfg->max_iterations, 0xFFFFFFFFull);
    a.residual_tolerance = cfg->residual_tolerance;
    a.step_tolerance = cfg->step_tolerance;
    a.initial_lambda = cfg->initial_lambda;
}

}  // namespace

namespace ezpz {

unsigned long long* g_stamps = nullptr;

// (`resident`: whether the launch stays on the device for further requests, DoneWord::request)
int solve_batch_device_impl(EzpzSystem* sys, const double* x0_dev, size_t batch, const EzpzConfig* cfg, double* x_out_dev,
                                   EzpzStatus* status_dev, uint8_t* unsat_mask_dev, uint64_t* warn_log_dev, uint32_t warn_cap,
                                   void* stream, const DoneWord& done, bool* resident) {
    if (!sys || (batch && (!x_out_dev || !status_dev))) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch && sys->counts.n_vars && !x0_dev) return EZPZ_ERR_INVALID_ARGUMENT;
    EZPZ_ON_DEVICE(sys->device);
    SolveArgs a = solve_args_for(sys, x0_dev, batch, cfg, x_out_dev, status_dev, unsat_mask_dev, warn_log_dev, warn_cap);
    a.done = done;
    const int rc = launch(*sys, a, static_cast<hipStream_t>(stream));
    if (resident) *resident = rc == EZPZ_OK && a.done.request != nullptr;
    return rc;
}

// The same call as the component, lane and wavefront kernels take it.
CompLaunch comp_launch_args(const SolveArgs& args) {
    CompLaunch L{};
    L.x0 = args.x0;
    L.x_out = args.x_out;
    L.status = args.status;
    L.unsat_mask = args.unsat_mask;
    L.warn_log = args.warn_log;
    L.warn_cap = args.warn_cap;
    L.batch = args.batch;
    L.max_iterations = args.max_iterations;
    L.residual_tolerance = args.residual_tolerance;
    L.step_tolerance = args.step_tolerance;
    L.initial_lambda = args.initial_lambda;
    L.done = args.done;
    return L;
}

// The argument block of the list-walk kernels for a call on `sys` (device pointers; no completion word).
SolveArgs solve_args_for(EzpzSystem* sys, const double* x0_dev, size_t batch, const EzpzConfig* cfg, double* x_out_dev,
                         EzpzStatus* status_dev, uint8_t* unsat_mask_dev, uint64_t* warn_log_dev, uint32_t warn_cap) {
    SolveArgs a{};
    a.p = sys->view;
    a.x0 = x0_dev;
    a.x_out = x_out_dev;
    a.status = status_dev;
    a.unsat_mask = unsat_mask_dev;
    a.warn_log = warn_cap ? warn_log_dev : nullptr;
    a.warn_cap = warn_cap;
    a.batch = batch;
    a.ws_doubles = sys->ws_doubles;
    a.prog_lds_doubles = sys->prog_lds_doubles;
    a.lvl_lds_off = sys->lvl_lds_off;
    a.lvl_tab_words = sys->lvl_tab_words;
    a.lvl_buf_words = sys->lvl_buf_words;
    a.n_dense = sys->n_dense;
    a.dense_level0 = sys->dense_level0;
    a.dense_lds_off = sys->dense_lds_off;
    a.dense_lds_doubles = sys->dense_lds_doubles;
    a.stamps = g_stamps;
    a.unit_weights = sys->unit_weights ? 1u : 0u;
    a.grid_wgs = 1;  // (gws, the grid team's scratch, the list of systems and the resumed states: none)
    if (sys->rec) {
        const unsigned char* base = static_cast<const unsigned char*>(sys->dev_program);
        a.rec_desc = reinterpret_cast<const uint2*>(base + sys->rec_desc_off);
        a.rec_chunks = reinterpret_cast<const uint4*>(base + sys->rec_chunks_off);
        a.rec_rounds = sys->rec_rounds;
        a.rec_desc_off = sys->rec_desc_lds_off;
        if (sys->rec_asm_kc) {
            a.rec_asm_cols = reinterpret_cast<const uint4*>(base + sys->rec_asm_cols_off);
            a.rec_asm_slots = reinterpret_cast<const uint4*>(base + sys->rec_asm_slots_off);
            a.rec_asm_kc = sys->rec_asm_kc;
            a.rec_asm_ks = sys->rec_asm_ks;
        }
        const uint32_t n = sys->counts.n_vars, m = sys->counts.n_rows;
        const uint32_t o_d = n + 2 * m + (sys->rec_jglobal ? 0u : sys->counts.zj), o_dd = rec_ws_base(sys->counts, sys->rec_jglobal);
        a.rec_dd_delta = o_dd - o_d;
        a.rec_zero = o_dd + n;
        a.rec_jglobal = sys->rec_jglobal ? 1u : 0u;
        a.rec_jstride = (sys->counts.zj + 2) & ~1u;  // (the values, the zero of padding pairs)
    }
    fill_cfg(a, cfg);
    return a;
}

// The systems of one topology inside a heterogeneous batch, solved IN PLACE by the lane-per-system kernel (mixed.hip): lane i
// reads its values at row_offset[i] of the caller's ragged buffer, writes them back there and its status to
// status[sys_of[i]] -- no gather into a block, no scatter back.  EZPZ_OK when it ran that way; 1 when this topology is not
// (yet) served by that kernel (not a small system, kernel not compiled): the caller gathers, calls the ordinary entry, scatters.
int lane_indexed_launch(EzpzSystem* sys, const double* x_ragged, const uint64_t* row_offset_dev, const uint32_t* sys_of_dev,
                        uint64_t count, const EzpzConfig* cfg, double* x_out_ragged, EzpzStatus* status_all, void* stream) {
    if (!sys || !sys->lane || !sys->jit || count == 0) return 1;
    std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
    int st = comp_jit_state(sys->jit);
    if (st == 0 && (count >= sys->lim.policy.jit_lane_min_batch || jit_sync())) st = comp_jit_request(sys->jit, jit_sync());
    if (st != 2) return 1;
    SolveArgs a{};
    fill_cfg(a, cfg);
    CompLaunch L = comp_launch_args(a);
    L.x0 = x_ragged;
    L.x_out = x_out_ragged;
    L.status = status_all;
    L.batch = count;
    L.row_offset = row_offset_dev;
    L.sys_of = sys_of_dev;
    return lane_jit_launch(sys->jit, *sys->lane, L, sys->device, sys->lim.cus, static_cast<hipStream_t>(stream)) == EZPZ_OK ? EZPZ_OK : 1;
}

// The pipelined host-to-host path's copy out, as a kernel (pipeline.cpp): `bytes` (a multiple of 8: rows of doubles, 32-byte
// statuses) from device memory into registered host memory through its device address.  16 bytes per lane and store where both
// addresses and the length allow it; a piece of an odd number of doubles, or one that starts on an odd double (odd n_vars and
// an odd number of systems before it), goes 8 bytes at a time.  Which engine moves a hipMemcpyAsync is the runtime's choice;
// this one is ours (tools/pcie_duplex.hip: a copy kernel out beside copies in keeps 41-43 GB/s each way whatever moves the
// copies in).
template <class T>
__global__ void __launch_bounds__(256) copy_out_kernel(const T* __restrict__ src, T* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
void launch_copy_out(void* dst_host_as_device, const void* src_dev, size_t bytes, void* stream) {
    const bool wide = ((reinterpret_cast<uintptr_t>(dst_host_as_device) | reinterpret_cast<uintptr_t>(src_dev) | bytes) & 15u) == 0;
    if (wide)
        hipLaunchKernelGGL(copy_out_kernel<uint4>, dim3(64), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint4*>(src_dev),
                           static_cast<uint4*>(dst_host_as_device), bytes / 16);
    else
        hipLaunchKernelGGL(copy_out_kernel<uint2>, dim3(64), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint2*>(src_dev),
                           static_cast<uint2*>(dst_host_as_device), bytes / 8);
}

// The evaluation-only kernel (K1: residuals and Jacobian values at given points, internal numbering) on `stream`.
void launch_eval(EzpzSystem* sys, const double* x_int_dev, size_t batch, double* r_out_dev, double* jv_out_dev, uint32_t* deg_out_dev,
                 uint32_t grid, hipStream_t stream) {
    EvalArgs e{};
    e.p = sys->view;
    e.x = x_int_dev;
    e.r_out = r_out_dev;
    e.jv_out = jv_out_dev;
    e.deg_out = deg_out_dev;
    e.batch = batch;
    hipLaunchKernelGGL(eval_kernel, dim3(grid), dim3(256), 0, stream, e);
}

}  // namespace ezpz

extern "C" {

int ezpz_system_solve_batch_device(EzpzSystem* sys, const double* x0_dev, size_t batch, const EzpzConfig* cfg,
                                   double* x_out_dev, EzpzStatus* status_dev, uint8_t* unsat_mask_dev,
                                   uint64_t* warn_log_dev, uint32_t warn_cap, void* stream) {
    if (sys) release_thread_kernel(sys->device);
    return solve_batch_device_impl(sys, x0_dev, batch, cfg, x_out_dev, status_dev, unsat_mask_dev, warn_log_dev, warn_cap, stream,
                                   DoneWord{nullptr, 0, nullptr});
}

int ezpz_system_eval_batch(EzpzSystem* sys, const double* x, size_t batch, double* r_out, double* jv_out,
                           uint32_t* degenerate_count_out) {
    if (!sys || !x || !r_out || !jv_out) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch == 0) return EZPZ_OK;
    release_thread_kernel(sys->device);
    if (int rc0 = ensure_program(sys)) return rc0;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    return ezpz::eval_batch_locked(sys, x, batch, r_out, jv_out, degenerate_count_out);
}

}  // extern "C"

// (the caller holds sys->mu, the system's device is current and its program is there: ensure_program)
int ezpz::eval_batch_locked(EzpzSystem* sys, const double* x, size_t batch, double* r_out, double* jv_out, uint32_t* degenerate_count_out) {
    const size_t n = sys->counts.n_vars, m = sys->counts.n_rows, zj = sys->counts.zj;
    DevBuf<double> xd, rd, jd;
    DevBuf<uint32_t> dd;
    int rc;
    if ((rc = xd.ensure(batch * std::max<size_t>(n, 1))) != EZPZ_OK) return rc;
    if ((rc = rd.ensure(batch * std::max<size_t>(m, 1))) != EZPZ_OK) return rc;
    if ((rc = jd.ensure(batch * std::max<size_t>(zj, 1))) != EZPZ_OK) return rc;
    if ((rc = dd.ensure(batch)) != EZPZ_OK) return rc;
    // the evaluators address values / rows by the program's internal numbering
    std::vector<double> xin(batch * std::max<size_t>(n, 1)), rin(batch * std::max<size_t>(m, 1));
    for (size_t b = 0; b < batch; ++b)
        for (size_t k = 0; k < n; ++k) xin[b * n + k] = x[b * n + sys->host_var_of[k]];
    HIP_TRY(hipMemcpy(xd.p, xin.data(), batch * n * sizeof(double), hipMemcpyHostToDevice));
    EvalArgs e{};
    e.p = sys->view;
    e.x = xd.p;
    e.r_out = rd.p;
    e.jv_out = jd.p;
    e.deg_out = dd.p;
    e.batch = batch;
    uint32_t grid = (uint32_t)std::min<size_t>(batch, 4096);
    hipLaunchKernelGGL(eval_kernel, dim3(grid), dim3(256), 0, nullptr, e);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(rin.data(), rd.p, batch * m * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < batch; ++b)
        for (size_t k = 0; k < m; ++k) r_out[b * m + sys->host_row_of[k]] = rin[b * m + k];
    HIP_TRY(hipMemcpy(jv_out, jd.p, batch * zj * sizeof(double), hipMemcpyDeviceToHost));
    if (degenerate_count_out)
        HIP_TRY(hipMemcpy(degenerate_count_out, dd.p, batch * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return EZPZ_OK;
}
