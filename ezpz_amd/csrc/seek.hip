// Dimension targets (include/ezpz_amd.h: ezpz_seek_step, ezpz_system_seek_targets and its _device form): the host side
// of seek.hip.hpp's kernels -- the check of a request, the plan a system keeps (the rounds' workspace, the tables, the host form's
// staging) and the rounds.  A round is ezpz_system_solve_batch_params_device -> ezpz_system_param_sensitivity_device ->
// ezpz_system_measure_device -> ezpz_system_measure_response_device -> seek_step_kernel -> seek_commit_kernel, all on the caller's
// stream: the four entries are those entries themselves, with their routes, their locks and their ordering.
#include "driven_params.hpp"
#include "host_stage.hpp"
#include "measure_tables.hpp"
#include "seek.hip.hpp"

#include <limits>

using namespace ezpz;

namespace {

static_assert(sizeof(EzpzSeekConfig) == 136 && sizeof(EzpzSeekInfo) == 48, "the layouts include/ezpz_amd.h documents");

constexpr uint64_t kDefaultChunk = 65536;        // systems per pass where the caller leaves the choice ...
constexpr uint64_t kChunkBytes = 256ull << 20;   // ... while S [chunk][n_param][n_vars] stays below this
constexpr uint32_t kMaxIterations = 65535;

struct SeekPlan {
    std::mutex mu;  // a run holds it from its first upload to its last enqueue
    // The completion of the last run's launches: a run on another stream goes behind it, and whatever a run overwrites from the
    // host -- the tables, a buffer that has to grow -- waits for it first
    LaunchOrder order;
    std::vector<double> tab_kept;  // what `tab` holds
    DevBuf<double> tab;            // weight | tol [n_meas] each, then lo | hi | scale [n_param] each
    DevBuf<double> x_trial, p_trial, S, m_trial, D_trial, D_best;
    DevBuf<EzpzStatus> solve_status;
    DevBuf<uint32_t> sens_status;
    DevBuf<uint8_t> flags, verdict;
    DevBuf<unsigned int> active;
    DevBuf<unsigned char> host_stage;  // the host form's staging (host_stage.hpp)
};

SeekPlan& plan_of(EzpzSystem* sys) {
    std::lock_guard<std::mutex> lock(sys->mu);
    if (!sys->seek) sys->seek = std::make_shared<SeekPlan>();
    return *static_cast<SeekPlan*>(sys->seek.get());
}

struct Request {
    EzpzSeekConfig c;
    std::vector<double> tab;  // weight | tol | lo | hi | scale
    uint64_t chunk = 0;
};

// The configuration's own errors, and its tables with the defaults filled in.
int check_config(const EzpzSeekConfig* cfg, size_t n_param, size_t n_meas, Request& r) {
    ezpz_default_seek_config(&r.c);
    if (cfg) r.c = *cfg;
    const EzpzSeekConfig& c = r.c;
    if (n_param > EZPZ_SEEK_MAX_PARAMS || n_meas > EZPZ_SEEK_MAX_TARGETS || c.max_iterations > kMaxIterations) return EZPZ_ERR_TOO_LARGE;
    const double inf = std::numeric_limits<double>::infinity();
    r.tab.resize(2 * n_meas + 3 * n_param);
    double *weight = r.tab.data(), *tol = weight + n_meas, *lo = tol + n_meas, *hi = lo + n_param, *scale = hi + n_param;
    for (size_t i = 0; i < n_meas; ++i) {
        weight[i] = c.weight ? c.weight[i] : 1.0;
        tol[i] = c.tol ? c.tol[i] : 1e-6;
        if (!(weight[i] >= 0.0) || !std::isfinite(weight[i]) || !(tol[i] >= 0.0) || !std::isfinite(tol[i])) return EZPZ_ERR_INVALID_ARGUMENT;
    }
    for (size_t j = 0; j < n_param; ++j) {
        lo[j] = c.lo ? c.lo[j] : -inf;
        hi[j] = c.hi ? c.hi[j] : inf;
        scale[j] = c.scale ? c.scale[j] : 1.0;
        if (!(lo[j] <= hi[j]) || !(scale[j] > 0.0) || !std::isfinite(scale[j])) return EZPZ_ERR_INVALID_ARGUMENT;
    }
    auto pos_finite = [](double v) { return v > 0.0 && std::isfinite(v); };
    if (!pos_finite(c.mu0) || !pos_finite(c.mu_up) || !pos_finite(c.mu_down) || !pos_finite(c.mu_min) || !pos_finite(c.mu_max) ||
        !(c.mu_up > 1.0) || !(c.mu_down < 1.0) || c.mu_min > c.mu0 || c.mu0 > c.mu_max || !(c.step_tol >= 0.0) || !std::isfinite(c.step_tol) ||
        !(c.sens_lambda >= 0.0) || !std::isfinite(c.sens_lambda))
        return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

// Every argument error of a run, before anything is enqueued or written.  The value pointers are only compared with NULL.
int check_run(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params0,
              const EzpzConstraint* records, size_t n_meas, const double* targets, size_t batch, const EzpzSeekConfig* cfg,
              const void* params_out, const void* x_out, const void* m_out, const void* info_out, hipStream_t stream, Request& r) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    if (int rc = check_config(cfg, n_param, n_meas, r)) return rc;
    std::vector<uint32_t> words;
    if (int rc = measure_pack_records(records, n_meas, sys->counts.n_vars, words)) return rc;
    // the params entry's and the sensitivity entry's errors: the list, a system either declines, a capture their fronts refuse
    if (n_param) {
        DrivenRequest driven;
        if (int rc = driven_request(sys, positions, n_param, driven)) return rc;
        EzpzSensitivityPlan sens;
        if (int rc = ezpz_system_param_sensitivity_plan(sys, positions, n_param, &sens)) return rc;
        if (stream_capturing(stream) && ((driven.params_route == EZPZ_PARAMS_ROUTE_FRONTS && sys->fronts->n_wgs > 1) ||
                                         (sens.route == EZPZ_SENSITIVITY_ROUTE_FRONTS && sens.front_workgroups > 1)))
            return EZPZ_ERR_INVALID_ARGUMENT;
    }
    if (batch > 0xFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    if (batch && n_param && n_meas &&
        (!params0 || !targets || !params_out || !x_out || !m_out || !info_out || (sys->counts.n_vars && !x0)))
        return EZPZ_ERR_INVALID_ARGUMENT;
    uint64_t chunk = r.c.chunk;
    if (chunk == 0) {
        chunk = kDefaultChunk;
        while (chunk > 64 && chunk * std::max<uint64_t>(n_param, 1) * std::max<uint64_t>(sys->counts.n_vars, 1) * sizeof(double) > kChunkBytes) chunk /= 2;
    }
    chunk = (chunk + 63) / 64 * 64;
    r.chunk = std::min<uint64_t>(chunk, (std::max<uint64_t>(batch, 1) + 63) / 64 * 64);
    return EZPZ_OK;
}

uint32_t stride_grid(uint64_t items, const EzpzSystem* sys) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, (uint64_t)sys->lim.cus * 16));
}

// What the host writes before a run: the tables and the workspace of a chunk, behind the last run's launches.
int prepare(SeekPlan& P, const Request& r, size_t n, size_t n_param, size_t n_meas) {
    const uint64_t chunk = r.chunk;
    const size_t rounds = (size_t)r.c.max_iterations + 1;
    const bool new_tables = r.tab != P.tab_kept;
    const bool grows = chunk * n > P.x_trial.cap || chunk * n_param > P.p_trial.cap || chunk * n_param * n > P.S.cap ||
                       chunk * n_meas > P.m_trial.cap || chunk * n_meas * n_param > P.D_trial.cap || chunk > P.solve_status.cap ||
                       rounds > P.active.cap;
    if (!new_tables && !grows) return EZPZ_OK;
    int rc;
    if ((rc = P.order.before_overwrite()) != EZPZ_OK) return rc;
    P.tab_kept.clear();
    if ((rc = P.tab.ensure(r.tab.size())) != EZPZ_OK) return rc;
    HIP_TRY(hipMemcpy(P.tab.p, r.tab.data(), r.tab.size() * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = P.x_trial.ensure(chunk * n)) != EZPZ_OK || (rc = P.p_trial.ensure(chunk * n_param)) != EZPZ_OK ||
        (rc = P.S.ensure(chunk * n_param * n)) != EZPZ_OK || (rc = P.m_trial.ensure(chunk * n_meas)) != EZPZ_OK ||
        (rc = P.flags.ensure(chunk * n_meas)) != EZPZ_OK || (rc = P.D_trial.ensure(chunk * n_meas * n_param)) != EZPZ_OK ||
        (rc = P.D_best.ensure(chunk * n_meas * n_param)) != EZPZ_OK || (rc = P.solve_status.ensure(chunk)) != EZPZ_OK ||
        (rc = P.sens_status.ensure(chunk)) != EZPZ_OK || (rc = P.verdict.ensure(chunk)) != EZPZ_OK ||
        (rc = P.active.ensure(rounds)) != EZPZ_OK)
        return rc;
    P.tab_kept = r.tab;
    call_stamp(SEEK_TABLES_UPLOADED);
    return EZPZ_OK;
}

template <int T>
void launch_step(const seek::StepArgs& a, hipStream_t stream) {
    const uint32_t per_wg = 256 / T;
    hipLaunchKernelGGL(seek::seek_step_kernel<T>, dim3((a.count + per_wg - 1) / per_wg), dim3(256), 0, stream, a);
}

// One chunk's whole loop, device pointers throughout: the plan's mutex is held, the system's device current, the request checked,
// the workspace prepared, count > 0.  `early_exit`: the host form -- after each round the host reads that round's counter of
// unfinished systems and stops at zero.
int run_chunk(EzpzSystem* sys, SeekPlan& P, const Request& r, const double* x0_dev, const uint32_t* positions, size_t n_param,
              const double* params0_dev, const EzpzConstraint* records, size_t n_meas, const double* targets_dev, size_t count,
              double* params_out, double* x_out, double* m_out, EzpzSeekInfo* info_out, double* trace_out, bool early_exit,
              hipStream_t stream) {
    const size_t n = sys->counts.n_vars;
    const EzpzSeekConfig& c = r.c;
    const uint32_t rounds = c.max_iterations + 1;
    int rc;
    seek::StepArgs a{};
    a.solve_status = P.solve_status.p;
    a.sens_status = P.sens_status.p;
    a.m_trial = P.m_trial.p;
    a.flags = P.flags.p;
    a.D_trial = P.D_trial.p;
    a.targets = targets_dev;
    a.weight = P.tab.p;
    a.tol = a.weight + n_meas;
    a.lo = a.tol + n_meas;
    a.hi = a.lo + n_param;
    a.scale = a.hi + n_param;
    a.p = params_out;
    a.m = m_out;
    a.D = P.D_best.p;
    a.info = info_out;
    a.trace = trace_out;
    a.p_trial = P.p_trial.p;
    a.verdict = P.verdict.p;
    a.active = P.active.p;
    a.count = (uint32_t)count, a.n_param = (uint32_t)n_param, a.n_meas = (uint32_t)n_meas, a.max_iterations = c.max_iterations;
    a.mu0 = c.mu0, a.mu_up = c.mu_up, a.mu_down = c.mu_down, a.mu_min = c.mu_min, a.mu_max = c.mu_max, a.step_tol = c.step_tol;
    HIP_TRY(hipMemsetAsync(P.active.p, 0, rounds * sizeof(unsigned int), stream));
    if (n && x0_dev != x_out) HIP_TRY(hipMemcpyAsync(x_out, x0_dev, count * n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(seek::seek_start_kernel, dim3(stride_grid(count * n_param, sys)), dim3(256), 0, stream, params0_dev, a.lo, a.hi,
                       (uint32_t)n_param, (uint64_t)count, params_out, P.p_trial.p);
    HIP_TRY(hipGetLastError());
    for (uint32_t round = 0; round < rounds; ++round) {
        if ((rc = ezpz_system_solve_batch_params_device(sys, x_out, positions, n_param, P.p_trial.p, count, &c.inner, P.x_trial.p,
                                                        P.solve_status.p, nullptr, nullptr, 0, stream)) != EZPZ_OK ||
            (rc = ezpz_system_param_sensitivity_device(sys, P.x_trial.p, positions, n_param, P.p_trial.p, count, c.sens_lambda, P.S.p,
                                                       P.sens_status.p, nullptr, stream)) != EZPZ_OK ||
            (rc = ezpz_system_measure_device(sys, records, n_meas, P.x_trial.p, count, P.m_trial.p, P.flags.p, nullptr, stream)) != EZPZ_OK ||
            (rc = ezpz_system_measure_response_device(sys, records, n_meas, P.x_trial.p, P.S.p, n_param, count, nullptr, P.D_trial.p,
                                                      nullptr, nullptr, stream)) != EZPZ_OK)
            return rc;
        a.round = round;
        if (n_param <= 4)
            launch_step<4>(a, stream);
        else if (n_param <= 8)
            launch_step<8>(a, stream);
        else
            launch_step<16>(a, stream);
        if (n) hipLaunchKernelGGL(seek::seek_commit_kernel, dim3(stride_grid(count * 64, sys)), dim3(256), 0, stream, P.verdict.p, P.x_trial.p, x_out, (uint32_t)n, (uint64_t)count);
        HIP_TRY(hipGetLastError());
        if (early_exit) {
            unsigned int left = 0;
            HIP_TRY(hipStreamSynchronize(stream));
            HIP_TRY(hipMemcpy(&left, P.active.p + round, sizeof(left), hipMemcpyDeviceToHost));
            if (left == 0) break;
        }
    }
    return EZPZ_OK;
}

}  // namespace

extern "C" {

void ezpz_default_seek_config(EzpzSeekConfig* cfg) {
    if (!cfg) return;
    cfg->weight = cfg->tol = cfg->lo = cfg->hi = cfg->scale = nullptr;
    cfg->max_iterations = 40;
    cfg->chunk = 0;
    cfg->mu0 = 1e-3, cfg->mu_up = 10.0, cfg->mu_down = 0.1, cfg->mu_min = 1e-12, cfg->mu_max = 1e12;
    cfg->step_tol = 1e-12;
    ezpz_default_config(&cfg->inner);
    cfg->sens_lambda = cfg->inner.initial_lambda;
}

int ezpz_seek_step(size_t n_param, size_t n_meas, const double* p, const double* m, const double* D, const double* targets,
                   const EzpzSeekConfig* cfg, double mu, double* p_trial_out, double* delta_out, uint32_t* held_out) {
    Request r;
    if (int rc = check_config(cfg, n_param, n_meas, r)) return rc;
    if (n_param == 0 || !p || !p_trial_out || !delta_out || (n_meas && (!m || !D || !targets))) return EZPZ_ERR_INVALID_ARGUMENT;
    const double *weight = r.tab.data(), *lo = weight + 2 * n_meas, *hi = lo + n_param, *scale = hi + n_param;
    return seek::step_host((uint32_t)n_param, (uint32_t)n_meas, p, m, D, targets, weight, lo, hi, scale, mu, r.c.step_tol, p_trial_out,
                           delta_out, held_out);
}

int ezpz_system_seek_targets_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                    const double* params0_dev, const EzpzConstraint* records, size_t n_meas, const double* targets_dev,
                                    size_t batch, const EzpzSeekConfig* cfg, double* params_out_dev, double* x_out_dev, double* m_out_dev,
                                    EzpzSeekInfo* info_out_dev, double* cost_trace_out_dev, void* stream) {
    Request r;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = check_run(sys, x0_dev, positions, n_param, params0_dev, records, n_meas, targets_dev, batch, cfg, params_out_dev, x_out_dev,
                           m_out_dev, info_out_dev, st, r))
        return rc;
    if (batch == 0 || n_param == 0 || n_meas == 0) return EZPZ_OK;
    SeekPlan& P = plan_of(sys);
    std::lock_guard<std::mutex> lock(P.mu);
    EZPZ_ON_DEVICE(sys->device);
    release_thread_kernel(sys->device);
    const size_t n = sys->counts.n_vars, trace_row = (size_t)r.c.max_iterations + 1;
    int rc;
    if ((rc = prepare(P, r, n, n_param, n_meas)) != EZPZ_OK || (rc = P.order.order_behind(st)) != EZPZ_OK) return rc;
    for (size_t first = 0; first < batch; first += r.chunk) {
        const size_t count = std::min<size_t>(r.chunk, batch - first);
        if ((rc = run_chunk(sys, P, r, x0_dev + first * n, positions, n_param, params0_dev + first * n_param, records, n_meas,
                            targets_dev + first * n_meas, count, params_out_dev + first * n_param, x_out_dev + first * n,
                            m_out_dev + first * n_meas, info_out_dev + first,
                            cost_trace_out_dev ? cost_trace_out_dev + first * trace_row : nullptr, false, st)) != EZPZ_OK)
            return rc;
    }
    call_stamp(SEEK_LAUNCHED);
    return P.order.record(st);
}

int ezpz_system_seek_targets(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params0,
                             const EzpzConstraint* records, size_t n_meas, const double* targets, size_t batch, const EzpzSeekConfig* cfg,
                             double* params_out, double* x_out, double* m_out, EzpzSeekInfo* info_out, double* cost_trace_out) {
    Request r;
    hipStream_t st = hipStreamPerThread;
    if (int rc = check_run(sys, x0, positions, n_param, params0, records, n_meas, targets, batch, cfg, params_out, x_out, m_out, info_out, st, r))
        return rc;
    if (batch == 0 || n_param == 0 || n_meas == 0) return EZPZ_OK;
    for (size_t k = 0; k < batch * n_meas; ++k)
        if (!std::isfinite(targets[k])) return EZPZ_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < batch * n_param; ++k)
        if (!std::isfinite(params0[k])) return EZPZ_ERR_INVALID_ARGUMENT;
    SeekPlan& P = plan_of(sys);
    std::lock_guard<std::mutex> lock(P.mu);
    EZPZ_ON_DEVICE(sys->device);
    release_thread_kernel(sys->device);
    const size_t n = sys->counts.n_vars, trace_row = (size_t)r.c.max_iterations + 1, chunk = r.chunk;
    int rc;
    if ((rc = prepare(P, r, n, n_param, n_meas)) != EZPZ_OK) return rc;
    if ((rc = P.order.order_behind(st)) != EZPZ_OK) return rc;
    for (size_t first = 0; first < batch; first += chunk) {
        const size_t count = std::min<size_t>(chunk, batch - first);
        // the chunk's list (the first chunk is the largest: only its reserve() allocates); x0 and x_out share a place
        const double *p0_dev, *targets_dev;
        double *x_dev, *p_dev, *m_dev, *trace_dev;
        EzpzSeekInfo* info_dev;
        Staged io;
        io.inout(x0 + first * n, count * n, x_out + first * n, count * n, x_dev, Staged::kPlaced);  // (the solve entry wants its x whatever n is)
        io.in(params0 + first * n_param, count * n_param, p0_dev);
        io.in(targets + first * n_meas, count * n_meas, targets_dev);
        io.out(params_out + first * n_param, count * n_param, p_dev);
        io.out(m_out + first * n_meas, count * n_meas, m_dev);
        io.out(info_out + first, count, info_dev);
        io.out(cost_trace_out ? cost_trace_out + first * trace_row : nullptr, count * trace_row, trace_dev);
        if ((rc = io.reserve(P.host_stage)) != EZPZ_OK || (rc = io.upload(P.host_stage)) != EZPZ_OK) return rc;
        if ((rc = run_chunk(sys, P, r, x_dev, positions, n_param, p0_dev, records, n_meas, targets_dev, count, p_dev, x_dev, m_dev, info_dev,
                            trace_dev, true, st)) != EZPZ_OK)
            return rc;
        HIP_TRY(hipStreamSynchronize(st));
        if ((rc = io.copy_back(P.host_stage)) != EZPZ_OK) return rc;
    }
    call_stamp(SEEK_LAUNCHED);
    return P.order.record(st);
}

}  // extern "C"
