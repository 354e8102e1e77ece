// Dimension sensitivities on the FRONTAL shape: the route ezpz_system_set_sensitivity_route selects for
// ezpz_system_param_sensitivity[_device] on a system whose frontal plan serves every call -- one factorisation per work item,
// many right-hand sides, whatever the size of the component.  The only translation unit that instantiates front_sens_kernel;
// the builds of front.hip and front_params.hip are what they were.  The tables come from front_sens_plan.cpp; the list they
// were made for is a KeptList (system.hpp), whose event this route alone stays out of while its stream is being captured.
#include "driven_params.hpp"
#include "front_launch.hip.hpp"
#include "front_sens_kernel.hip.hpp"

using namespace ezpz;

namespace {

// The route's plan of a `positions` list, kept on the system for a caller that repeats its list (touched under launch_mu).
struct FrontSensPlan {
    KeptList list;
    DevBuf<uint32_t> tabs, par_slot;
    uint64_t capacity = 0;  // workgroups of the build the device holds at once (0 = not asked yet)
};

FrontSensPlan& plan_of(EzpzSystem& s) {
    if (!s.front_sens) s.front_sens = std::make_shared<FrontSensPlan>();
    return *static_cast<FrontSensPlan*>(s.front_sens.get());
}

int capacity_of(EzpzSystem& s, FrontSensPlan& P) {
    if (P.capacity) return EZPZ_OK;
    int per_cu = 0;
    if (s.fronts->linear_only) {
        if (int rc = front_per_cu(s, front_sens_kernel<true>, s.fronts->lds_bytes, per_cu)) return rc;
    } else {
        if (int rc = front_per_cu(s, front_sens_kernel<false>, s.fronts->lds_bytes, per_cu)) return rc;
    }
    P.capacity = (uint64_t)s.lim.cus * (uint64_t)std::max(per_cu, 1);
    return EZPZ_OK;
}

// Right-hand sides per work item: as few chunks per system as keep the device's places busy, never fewer right-hand sides per
// chunk than policy.hpp's minimum (every chunk repeats the factorisation); EZPZ_SENS_FRONTS_RHS_PER_ITEM=<n> overrides per call.
void chunking(const EzpzSystem& s, uint64_t capacity, size_t n_param, size_t batch, uint32_t& rhs_per_item, uint32_t& items_per_system) {
    const uint64_t k = std::max<size_t>(n_param, 1), places = std::max<uint64_t>(1, capacity / s.fronts->n_wgs);
    uint64_t chunks = (places + std::max<size_t>(batch, 1) - 1) / std::max<size_t>(batch, 1);
    chunks = std::max<uint64_t>(1, std::min<uint64_t>(chunks, k / kFrontSensMinRhsPerItem));
    uint64_t per = (k + chunks - 1) / chunks;
    if (const char* e = std::getenv("EZPZ_SENS_FRONTS_RHS_PER_ITEM")) {
        const long v = std::atol(e);
        if (v > 0) per = std::min<uint64_t>((uint64_t)v, k);
    }
    rhs_per_item = (uint32_t)per;
    items_per_system = (uint32_t)((k + per - 1) / per);
}

}  // namespace

namespace ezpz {

int front_sens_plan_info(EzpzSystem& s, size_t n_param, EzpzSensitivityPlan& out) {
    FrontSensPlan& P = plan_of(s);
    if (int rc = capacity_of(s, P)) return rc;
    out = EzpzSensitivityPlan{};
    out.n_components = s.fronts->n_components;
    out.route = EZPZ_SENSITIVITY_ROUTE_FRONTS;
    out.front_workgroups = s.fronts->n_wgs;
    chunking(s, P.capacity, n_param, 1, out.rhs_per_item, out.items_per_system);
    out.front_lds_bytes = (uint32_t)s.fronts->lds_bytes;
    return EZPZ_OK;
}

// (launch_mu is held, the system's device current, the request's arguments checked, batch and n_param not zero)
int front_sens_launch(EzpzSystem& s, const double* x_dev, const uint32_t* positions, size_t n_param, const std::vector<uint32_t>& slot_of_pos,
                      const double* params_dev, size_t batch, double lambda, double* S_dev, uint32_t* status_dev, uint32_t* deg_dev,
                      hipStream_t st) {
    const FrontPlan& plan = *s.fronts;
    FrontSensPlan& P = plan_of(s);
    if (!P.list.same(positions, n_param)) {
        std::vector<uint32_t> tabs;
        if (!front_sens_tables(plan, positions, n_param, tabs)) return EZPZ_ERR_INVALID_ARGUMENT;
        int rc;
        if ((rc = P.list.before_overwrite()) != EZPZ_OK) return rc;
        P.list.valid = false;
        if ((rc = P.tabs.ensure(tabs.size())) != EZPZ_OK) return rc;
        if ((rc = P.par_slot.ensure(slot_of_pos.size())) != EZPZ_OK) return rc;
        HIP_TRY(hipMemcpy(P.tabs.p, tabs.data(), tabs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(P.par_slot.p, slot_of_pos.data(), slot_of_pos.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (int rc2 = capacity_of(s, P)) return rc2;
        P.list.keep(positions, n_param);
    }
    const size_t n_vars = s.counts.n_vars;
    // (a launch that is being recorded into a graph takes no part in the list's event -- this route alone: its replays read the
    // tables of the list it was recorded with, which the caller keeps repeating)
    const bool take_part = !stream_capturing(st);
    if (int rc = P.list.order_behind(st, take_part)) return rc;
    HIP_TRY(hipMemsetAsync(status_dev, 0, batch * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(S_dev, 0, batch * n_param * n_vars * sizeof(double), st));
    if (deg_dev) HIP_TRY(hipMemsetAsync(deg_dev, 0, batch * sizeof(uint32_t), st));
    FrontSensArgs fa{};
    fa.plan = static_cast<const unsigned char*>(s.dev_fronts);
    fa.n_wgs = plan.n_wgs;
    fa.n_vars = plan.n_vars;
    fa.n_cons = plan.n_cons;
    fa.x0 = x_dev;
    fa.batch = batch;
    fa.unit_weights = plan.unit_weights ? 1u : 0u;
    fa.tab_lds_bytes = (plan.tab_bytes_max + 15u) & ~15u;
    fa.ws_doubles = plan.ws_doubles_max;
    fa.n_chunks = plan.n_chunks;
    fa.bad_chunk0 = plan.bad_chunk0;
    fa.verdict_chunk = plan.verdict_chunk;
    fa.params = params_dev;
    fa.par_slot = P.par_slot.p;
    fa.tabs = P.tabs.p;
    fa.S = S_dev;
    fa.sens_status = status_dev;
    fa.deg = deg_dev;
    fa.lambda = lambda;
    fa.n_param = (uint32_t)n_param;
    chunking(s, P.capacity, n_param, batch, fa.rhs_per_item, fa.items_per_system);
    // (the budget of the scratch's sequence numbers: a pass per right-hand side and one for the factorisation, where the solve
    // counts LM iterations)
    fa.max_iterations = fa.rhs_per_item;
    const uint64_t items = (uint64_t)batch * fa.items_per_system;
    int rc = plan.linear_only ? front_launch_on(s, front_sens_kernel<true>, fa, P.capacity, plan.lds_bytes, items, items, st)
                              : front_launch_on(s, front_sens_kernel<false>, fa, P.capacity, plan.lds_bytes, items, items, st);
    if (rc != EZPZ_OK) return rc;
    {
        const uint64_t row = (uint64_t)n_param * n_vars;
        const dim3 grid((uint32_t)std::min<uint64_t>((row + 255) / 256, 64), (uint32_t)std::min<uint64_t>(batch, 65535));
        hipLaunchKernelGGL(front_sens_finish_kernel, grid, dim3(256), 0, st, S_dev, (const uint32_t*)status_dev, row, (uint64_t)batch);
        HIP_TRY(hipGetLastError());
    }
    return P.list.record(st, take_part);
}

}  // namespace ezpz

extern "C" int ezpz_system_set_sensitivity_route(EzpzSystem* sys, uint32_t route) {
    if (!sys || route > EZPZ_SENSITIVITY_ROUTE_FRONTS) return EZPZ_ERR_INVALID_ARGUMENT;
    // only a system whose frontal plan serves every call, as for ezpz_system_set_params_route
    if (route == EZPZ_SENSITIVITY_ROUTE_FRONTS && !(sys->fronts && sys->dev_fronts && sys->front_max_batch == ~0ull))
        return EZPZ_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
    if (sys->sens_route == route) return EZPZ_OK;
    // (the launches of the route that is left are through before the next call takes the other one)
    if (sys->front_sens && plan_of(*sys).list.done) {
        EZPZ_ON_DEVICE(sys->device);
        if (int rc = plan_of(*sys).list.before_overwrite()) return rc;
    }
    sys->sens_route = route;
    return EZPZ_OK;
}
