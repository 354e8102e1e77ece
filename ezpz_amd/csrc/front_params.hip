// Driven dimensions and sweeps on the FRONTAL shape: the route ezpz_system_set_params_route selects for
// ezpz_system_solve_batch_params and ezpz_system_sweep_params on a system whose frontal plan serves every call.  The only
// translation unit that instantiates the PAR and SWP builds of front_solve_kernel; front.hip's builds are what they were.
// front_params_launch is the route launcher driven.cpp's enqueue calls for both entries.
#include "driven_params.hpp"
#include "front_launch.hip.hpp"

using namespace ezpz;

namespace {

template <bool LIN, bool SWP>
int lds_plan_build(EzpzSystem& s, uint32_t n_param, FrontParLds& out) {
    const FrontPlan& plan = *s.fronts;
    auto kernel = front_solve_kernel<LIN, true, SWP>;
    EzpzSystem::FrontPar& c = s.front_par[SWP ? 1 : 0];
    if (c.capacity == 0) {  // once per system and build, like front.hip's
        if (int rc = front_per_cu(s, kernel, plan.lds_bytes, c.per_cu)) return rc;
        c.capacity = (uint64_t)s.lim.cus * (uint64_t)std::max(c.per_cu, 1);
    }
    const size_t base = (plan.lds_bytes + 15) & ~size_t(15), with = base + (size_t)n_param * sizeof(double);
    if (c.n_param != n_param) {
        bool in_lds = params_lds_enabled() && with <= s.lim.lds_bytes;
        if (in_lds) {
            int per_cu = 0;
            if (int rc = front_per_cu(s, kernel, with, per_cu)) return rc;
            in_lds = per_cu >= 1 && per_cu == c.per_cu;
        }
        c.in_lds = in_lds;
        c.n_param = n_param;
    }
    out.in_lds = c.in_lds;
    out.bytes = (uint32_t)(c.in_lds ? with : plan.lds_bytes);
    out.off = c.in_lds ? (uint32_t)(base / 8) : 0u;
    return EZPZ_OK;
}

template <bool LIN, bool SWP>
int launch_build(EzpzSystem& s, SolveArgs& a, hipStream_t stream) {
    FrontParLds L;
    if (int rc = lds_plan_build<LIN, SWP>(s, a.n_param, L)) return rc;
    FrontParArgs fa{};
    static_cast<FrontArgs&>(fa) = front_args_for(s, a, FrontProbe{});
    fa.params = a.params;
    fa.par_slot = a.par_slot;
    fa.n_param = a.n_param;
    fa.par_lds_off = L.off;
    fa.steps = SWP ? a.steps : 1u;
    debug_params_line(s, a.n_param, L.in_lds, 0, s.fronts->lds_bytes, L.bytes);
    // (a sweep's steps run one behind the other on its slot: `batch` items side by side, batch x steps in all)
    return front_launch_on(s, front_solve_kernel<LIN, true, SWP>, fa, s.front_par[SWP ? 1 : 0].capacity, L.bytes, fa.batch,
                           fa.batch * (uint64_t)fa.steps, stream);
}

// The build of a system and a call.
struct Build {
    int (*lds_plan)(EzpzSystem&, uint32_t, FrontParLds&);
    int (*launch)(EzpzSystem&, SolveArgs&, hipStream_t);
};
template <bool LIN, bool SWP>
constexpr Build kBuild{lds_plan_build<LIN, SWP>, launch_build<LIN, SWP>};
const Build& build_of(const EzpzSystem& s, bool sweep) {
    const bool lin = s.fronts->linear_only;
    if (sweep) return lin ? kBuild<true, true> : kBuild<false, true>;
    return lin ? kBuild<true, false> : kBuild<false, false>;
}

}  // namespace

namespace ezpz {

int front_params_lds_plan(EzpzSystem& s, size_t n_param, bool sweep, FrontParLds& out) {
    if (!s.fronts || !s.dev_fronts) return EZPZ_ERR_INVALID_ARGUMENT;
    return build_of(s, sweep).lds_plan(s, (uint32_t)n_param, out);
}

int front_params_launch(EzpzSystem& s, SolveArgs& a, bool sweep, hipStream_t stream) {
    if (!s.fronts || !s.dev_fronts || !a.n_param || !a.params || !a.par_slot || (sweep && !a.steps)) return EZPZ_ERR_INVALID_ARGUMENT;
    return build_of(s, sweep).launch(s, a, stream);
}

}  // namespace ezpz

extern "C" int ezpz_system_set_params_route(EzpzSystem* sys, uint32_t route) {
    if (!sys || route > EZPZ_PARAMS_ROUTE_FRONTS) return EZPZ_ERR_INVALID_ARGUMENT;
    // only a system whose frontal plan serves every call (batch-auto systems that take the fronts for small calls alone: not served)
    if (route == EZPZ_PARAMS_ROUTE_FRONTS && !(sys->fronts && sys->dev_fronts && sys->front_max_batch == ~0ull))
        return EZPZ_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> launch_lock(sys->launch_mu);
    if (sys->params_route == route) return EZPZ_OK;
    // (the launches that read the other route's table are through before the next call of either entry replaces it)
    if (sys->driven.list.done) {
        EZPZ_ON_DEVICE(sys->device);
        if (int rc = sys->driven.list.before_overwrite()) return rc;
    }
    sys->params_route = route;
    return EZPZ_OK;
}
