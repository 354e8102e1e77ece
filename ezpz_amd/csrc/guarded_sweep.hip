// Guarded sweeps: ezpz_system_sweep_guarded, its device form and its plan entry (the rule is stated with the entry in
// ezpz_amd.h).  The sweep of sweep.hip with one policy in it -- a step that fails is halved, a sweep holds on to its last accepted
// answer -- decided where the values live: the team that owns a sweep runs its attempts as items of the sweep's loop (the GRD
// builds of lm_solve_kernel, instantiated here and nowhere else) on the sub-wavefront teams, the barrier workgroup and the record
// walk.  The other routes of the params entry have no such build; the host form runs the rule for them as rounds of
// ezpz_system_solve_batch_params, one attempt per round for every sweep still inside its step.
#include <cmath>

#include "driven_params.hpp"
#include "host_stage.hpp"
#include "list_walk_launch.hip.hpp"

using namespace ezpz;

namespace {

bool guard_config_ok(const EzpzGuardConfig& g) { return g.max_halvings <= 20 && g.max_attempts >= 1 && std::isfinite(g.max_move); }

// the routes with a GRD build (the fronts, the interpreter and the partitioned workgroup are follow-ups: DESIGN.md 12)
bool route_in_kernel(uint32_t route) {
    return route == EZPZ_SWEEP_SUB_WAVEFRONT_TEAMS || route == EZPZ_SWEEP_BARRIER_WORKGROUP || route == EZPZ_SWEEP_RECORD_WALK;
}

// p_u of the rule: three operations, each rounded by itself (this file is built without contraction, like the kernels)
inline double between(double pa, double pb, double u) { return u == 1.0 ? pb : pa + u * (pb - pa); }

// The rule from the host, for the routes the device form declines: every round is one params call over the whole batch.
int guarded_rounds(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params0, const double* params,
                   size_t steps, size_t batch, const EzpzConfig* cfg, const EzpzGuardConfig& g, double* x_out, EzpzStatus* status,
                   EzpzGuardStep* guard, double* params_reached, uint8_t* unsat_mask, uint64_t* warn_log, uint32_t warn_cap) {
    const size_t n = sys->counts.n_vars, C = sys->counts.n_cons;
    const bool want_log = warn_log && warn_cap;
    const double h_min = std::ldexp(1.0, -(int)g.max_halvings);
    std::vector<double> xs(x0, x0 + batch * n), ps(params0, params0 + batch * n_param), pa(batch * n_param), pu(batch * n_param);
    std::vector<double> x_try(batch * std::max<size_t>(n, 1));
    std::vector<EzpzStatus> st_try(batch);
    std::vector<uint8_t> mask_try(unsat_mask ? batch * std::max<size_t>(C, 1) : 0);
    std::vector<uint64_t> log_try(want_log ? batch * (size_t)warn_cap : 0);
    std::vector<double> t(batch), h(batch);
    std::vector<uint32_t> attempts(batch), accepted(batch);
    std::vector<uint8_t> inside(batch);
    for (size_t k = 0; k < steps; ++k) {
        const double* pb = params + k * batch * n_param;
        pa = ps;
        for (size_t b = 0; b < batch; ++b) {
            t[b] = 0.0;
            h[b] = 1.0;
            attempts[b] = accepted[b] = 0;
            inside[b] = 1;
        }
        for (size_t left = batch; left;) {
            for (size_t b = 0; b < batch; ++b)
                for (size_t j = 0; j < n_param; ++j)  // (a finished sweep solves again where it stands: its results are ignored)
                    pu[b * n_param + j] = inside[b] ? between(pa[b * n_param + j], pb[b * n_param + j], t[b] + h[b]) : ps[b * n_param + j];
            if (int rc = ezpz_system_solve_batch_params(sys, xs.data(), positions, n_param, pu.data(), batch, cfg, x_try.data(), st_try.data(),
                                                        unsat_mask ? mask_try.data() : nullptr, want_log ? log_try.data() : nullptr, warn_cap))
                return rc;
            for (size_t b = 0; b < batch; ++b) {
                if (!inside[b]) continue;
                const size_t row = k * batch + b;
                bool accept = st_try[b].converged == 1 && st_try[b].n_unsatisfied == 0;
                if (accept && g.max_move > 0.0)
                    for (size_t i = 0; i < n; ++i)
                        if (!(std::fabs(x_try[b * n + i] - xs[b * n + i]) <= g.max_move)) accept = false;
                ++attempts[b];
                status[row] = st_try[b];
                if (unsat_mask && C) std::memcpy(unsat_mask + row * C, mask_try.data() + b * C, C);
                if (want_log)
                    std::memcpy(warn_log + row * warn_cap, log_try.data() + b * (size_t)warn_cap,
                                std::min<size_t>(st_try[b].n_warnings, warn_cap) * sizeof(uint64_t));
                if (accept) {
                    std::copy_n(x_try.data() + b * n, n, xs.data() + b * n);
                    std::copy_n(pu.data() + b * n_param, n_param, ps.data() + b * n_param);
                    t[b] += h[b];
                    ++accepted[b];
                } else {
                    h[b] *= 0.5;
                }
                if (t[b] >= 1.0 || attempts[b] >= g.max_attempts || (!accept && h[b] < h_min)) {
                    inside[b] = 0;
                    --left;
                }
            }
        }
        std::copy(xs.begin(), xs.end(), x_out + k * batch * n);
        std::copy(ps.begin(), ps.end(), params_reached + k * batch * n_param);
        for (size_t b = 0; b < batch; ++b) guard[k * batch + b] = EzpzGuardStep{t[b], attempts[b], accepted[b]};
    }
    return EZPZ_OK;
}

}  // namespace

int ezpz::list_walk_guarded_launch(EzpzSystem& s, GuardedSolveArgs& a, uint32_t route, hipStream_t stream) {
    const ParLds L = par_lds_plan(s, a.n_param);
    a.par_lds_off = L.off;
    static const bool say = debug_topic("params");
    if (say)
        std::fprintf(stderr, "[ezpz guarded sweep] %zu sweeps of %zu steps, %u values per step %s (route %u, LDS %zu of %zu bytes)\n",
                     (size_t)a.batch, (size_t)a.steps, a.n_param, L.in_lds ? "staged in LDS" : "read from global memory", route, L.bytes,
                     s.lim.lds_bytes);
    return list_walk_one_workgroup<true, true>(s, a, L.bytes, stream);
}

extern "C" {

void ezpz_default_guard_config(EzpzGuardConfig* out) {
    if (!out) return;
    out->max_halvings = 4;
    out->max_attempts = 12;
    out->max_move = 0.0;
}

int ezpz_system_sweep_guarded_plan(EzpzSystem* sys, const uint32_t* positions, size_t n_param, EzpzSweepPlan* out) {
    if (!sys || !out || !n_param) return EZPZ_ERR_INVALID_ARGUMENT;
    EzpzSweepPlan p{};
    if (int rc = ezpz_system_sweep_params_plan(sys, positions, n_param, &p)) return rc;
    p.in_kernel = route_in_kernel(p.route) ? 1u : 0u;
    *out = p;
    return EZPZ_OK;
}

int ezpz_system_sweep_guarded_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                     const double* params0_dev, const double* params_dev, size_t steps, size_t batch,
                                     const EzpzConfig* cfg, const EzpzGuardConfig* guard_cfg, double* x_out_dev,
                                     EzpzStatus* status_dev, EzpzGuardStep* guard_dev, double* params_reached_dev,
                                     uint8_t* unsat_mask_dev, uint64_t* warn_log_dev, uint32_t warn_cap, void* stream) {
    if (!sys || !n_param || !params_dev) return EZPZ_ERR_INVALID_ARGUMENT;
    const bool work = steps && batch;
    if (steps > 0xFFFFFFFFull) return EZPZ_ERR_INVALID_ARGUMENT;
    if (work && (!x_out_dev || !status_dev || !params0_dev || !guard_dev || !params_reached_dev)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (work && sys->counts.n_vars && !x0_dev) return EZPZ_ERR_INVALID_ARGUMENT;
    EzpzGuardConfig g;
    ezpz_default_guard_config(&g);
    if (guard_cfg) g = *guard_cfg;
    if (!guard_config_ok(g)) return EZPZ_ERR_INVALID_ARGUMENT;
    DrivenRequest r;
    if (int rc = driven_request(sys, positions, n_param, r)) return rc;
    if (!route_in_kernel(r.sweep_route)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (!work) return EZPZ_OK;
    const GuardLaunch gl{params0_dev, params_reached_dev, guard_dev, g.max_move, std::ldexp(1.0, -(int)g.max_halvings), g.max_attempts};
    return driven_enqueue(sys, r, x0_dev, positions, n_param, params_dev, steps, batch, cfg, x_out_dev, status_dev, unsat_mask_dev,
                          warn_log_dev, warn_cap, static_cast<hipStream_t>(stream), &gl);
}

int ezpz_system_sweep_guarded(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params0,
                              const double* params, size_t steps, size_t batch, const EzpzConfig* cfg,
                              const EzpzGuardConfig* guard_cfg, double* x_out, EzpzStatus* status, EzpzGuardStep* guard,
                              double* params_reached, uint8_t* unsat_mask, uint64_t* warn_log, uint32_t warn_cap) {
    if (!sys || !n_param || !positions || !params) return EZPZ_ERR_INVALID_ARGUMENT;
    const bool work = steps && batch;
    if (steps > 0xFFFFFFFFull) return EZPZ_ERR_INVALID_ARGUMENT;
    if (work && (!x_out || !status || !params0 || !guard || !params_reached || (sys->counts.n_vars && !x0))) return EZPZ_ERR_INVALID_ARGUMENT;
    EzpzGuardConfig g;
    ezpz_default_guard_config(&g);
    if (guard_cfg) g = *guard_cfg;
    if (!guard_config_ok(g)) return EZPZ_ERR_INVALID_ARGUMENT;
    DrivenRequest r;
    if (int rc = driven_request(sys, positions, n_param, r)) return rc;
    if (!work) return EZPZ_OK;
    if (!route_in_kernel(r.sweep_route))
        return guarded_rounds(sys, x0, positions, n_param, params0, params, steps, batch, cfg, g, x_out, status, guard, params_reached,
                              unsat_mask, warn_log, warn_cap);
    // one launch: staged through a buffer of the call's own -- this form cannot hold sys->mu across the device form it calls -- with
    // x0 apart from x_out: a later step may gather from it again
    EZPZ_ON_DEVICE(sys->device);
    const size_t n = sys->counts.n_vars, C = sys->counts.n_cons, all = steps * batch;
    const bool want_log = warn_log && warn_cap;
    DevBuf<unsigned char> stage;
    const double *x0_dev, *p0_dev, *par_dev;
    double *xo_dev, *reached_dev;
    EzpzStatus* st_dev;
    EzpzGuardStep* guard_dev;
    uint8_t* mask_dev;
    uint64_t* log_dev;
    Staged io;
    io.in(x0, batch * n, x0_dev);
    io.in(params0, batch * n_param, p0_dev);
    io.in(params, all * n_param, par_dev);
    io.out(x_out, all * n, xo_dev, Staged::kPlaced);  // (the device form wants x_out whatever n is)
    io.out(status, all, st_dev);
    io.out(guard, all, guard_dev);
    io.out(params_reached, all * n_param, reached_dev);
    io.out(unsat_mask, all * C, mask_dev);
    io.room(want_log ? all * warn_cap : 0, log_dev);  // (the log goes home by copy_back_warn_log)
    int rc;
    if ((rc = io.reserve(stage)) != EZPZ_OK || (rc = io.upload(stage)) != EZPZ_OK) return rc;
    rc = ezpz_system_sweep_guarded_device(sys, x0_dev, positions, n_param, p0_dev, par_dev, steps, batch, cfg, &g, xo_dev, st_dev, guard_dev,
                                          reached_dev, mask_dev, log_dev, warn_cap, hipStreamPerThread);
    if (rc != EZPZ_OK) return rc;
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    if ((rc = io.copy_back(stage)) != EZPZ_OK) return rc;
    return want_log ? copy_back_warn_log(warn_log, log_dev, status, all, warn_cap) : EZPZ_OK;
}

}  // extern "C"
