// Monte-Carlo tolerance analysis (include/ezpz_amd.h: ezpz_mc_sample, ezpz_system_tolerance_mc and its _device form; DESIGN.md
// 3k): the host side of tolerance_mc.hip.hpp's kernels -- the check of a request, the plan a system keeps (the round's workspace,
// the sampler's and the limits' tables, the host form's buffers) and the rounds.  A round is sampler -> copies of x0 ->
// ezpz_system_solve_batch_params_device -> ezpz_system_measure_device -> reduction, all on the caller's stream: the driven solve
// and the measurement are those entries themselves, with their routes, their locks and their ordering.  The run with contributors
// (ezpz_system_tolerance_mc_contrib[_device]) is the same run on the same plan: one more enqueue per round behind the
// reduction -- mc_moments.hip's, on the round's params, m, flags and ok -- and the closing kernel behind the last round.  The run
// with Sobol indices (ezpz_system_tolerance_sobol[_device]) is a second run on the same plan, run_sobol() below: k' + 2
// sub-rounds a round, mc_sobol.hip's reduction behind the last one.  The run with quantiles (ezpz_system_tolerance_mc_quantiles[_device];
// DESIGN.md 3p) is run() again: every round's m, flags and ok kept on the device, mc_quantiles.hip's selection behind the last round.
#include "driven_params.hpp"
#include "mc_moments.hip.hpp"
#include "mc_quantiles.hip.hpp"
#include "mc_sobol.hip.hpp"
#include "measure_tables.hpp"
#include "tolerance_mc.hip.hpp"

using namespace ezpz;

namespace {

static_assert(sizeof(EzpzMcDist) == 24 && sizeof(EzpzMcStats) == 88 && sizeof(EzpzMcTotals) == 24 && sizeof(EzpzMcConfig) == 16,
              "the layouts include/ezpz_amd.h documents");

constexpr uint32_t kBlock = 256;              // samples per block of the sums: fixed by the interface
constexpr uint32_t kMaxHistBins = 64;
constexpr uint64_t kDefaultChunk = 65536;     // samples per round where the caller leaves the choice ...
constexpr uint64_t kChunkValueBytes = 256ull << 20;  // ... while one of the round's two value arrays stays below this

struct McPlan {
    std::mutex mu;  // a run holds it from its first upload to its last enqueue
    // The completion of the last run's launches: a run on another stream goes behind it, and whatever a run overwrites from the
    // host -- the tables, a buffer that has to grow -- waits for it first
    LaunchOrder order;
    std::vector<unsigned char> tables_kept;  // what `dist` and `tab` hold
    DevBuf<mc::Dist> dist;
    DevBuf<double> tab;  // lim_lo | lim_hi | hist_lo | hist_scale, [n_meas] each, | the draw's nominal [n_param]
    DevBuf<double> x_in, x_out, params, m, nominal, part_f;
    DevBuf<uint64_t> part_arg;
    DevBuf<uint32_t> part_n;
    DevBuf<uint8_t> flags, ok;
    DevBuf<EzpzStatus> status;
    DevBuf<unsigned int> ticket;
    // the host form's buffers
    DevBuf<double> x0_in;
    DevBuf<EzpzMcStats> stats_out;
    DevBuf<EzpzMcTotals> totals_out;
    DevBuf<uint64_t> hist_out;
    // the run with contributors: the moments' workspace, and the host form's buffers
    mcm::MomentWork moment_work;
    DevBuf<double> contrib_out;  // moments | cov | beta | contrib | r2
    DevBuf<uint64_t> contrib_words;  // EzpzMcMomentsInfo | dropped
    // the run with Sobol indices: the round's rows -- [k + 2][chunk][n_meas] values and flags, [k + 2][chunk] ok bytes
    // -- the sums' workspace, and the host form's buffers
    DevBuf<double> rows_f;
    DevBuf<uint8_t> rows_flags, rows_ok;
    sobol::SumWork sobol_work;
    DevBuf<double> sobol_out;  // sums | var | first | total | first_var | total_var
    DevBuf<uint64_t> sobol_words;  // n_complete
    // the run with quantiles: every sample's m, flags and ok -- samples x n_meas x 9 + samples bytes, the one
    // workspace here that grows with samples -- the selection's workspace, and the host form's buffer
    DevBuf<double> all_m;
    DevBuf<uint8_t> all_flags, all_ok;
    mcq::SelectWork select_work;
    DevBuf<EzpzMcQuantile> quant_out;
};

McPlan& plan_of(EzpzSystem* sys) {
    std::lock_guard<std::mutex> lock(sys->mu);
    if (!sys->tolerance_mc) sys->tolerance_mc = std::make_shared<McPlan>();
    return *static_cast<McPlan*>(sys->tolerance_mc.get());
}

// The argument errors of the distributions, and the sampler's table.
int check_dists(const EzpzMcDist* dist, const double* nominal, size_t n_param, std::vector<mc::Dist>& out) {
    out.clear();
    if (n_param == 0) return EZPZ_OK;
    if (!dist || !nominal || n_param > 0xFFFFFFFEull) return EZPZ_ERR_INVALID_ARGUMENT;
    out.resize(n_param);
    uint32_t corners = 0;
    for (size_t j = 0; j < n_param; ++j) {
        const EzpzMcDist& d = dist[j];
        if (d.kind > EZPZ_MC_CORNER || !std::isfinite(d.a) || !std::isfinite(d.b) || !std::isfinite(nominal[j]))
            return EZPZ_ERR_INVALID_ARGUMENT;
        if (d.kind == EZPZ_MC_UNIFORM && d.a > d.b) return EZPZ_ERR_INVALID_ARGUMENT;
        if (d.kind == EZPZ_MC_NORMAL && (d.a < 0.0 || d.b < 0.0 || (d.b > 0.0 && d.b < 1.0))) return EZPZ_ERR_INVALID_ARGUMENT;
        uint32_t rank = 0;
        if (d.kind == EZPZ_MC_CORNER) {
            if (corners == mc::kMaxCorners) return EZPZ_ERR_INVALID_ARGUMENT;
            rank = corners++;
        }
        out[j] = mc::Dist{d.kind, rank, d.a, d.b, nominal[j]};
    }
    return EZPZ_OK;
}

struct Request {
    std::vector<mc::Dist> dists;
    std::vector<uint32_t> words;  // the packed measurement records (compared by the measure entry against its kept list)
    std::vector<double> tab;      // lim_lo | lim_hi | hist_lo | hist_scale | the draw's nominal
    bool limits = false;
    uint32_t hist_bins = 0;
    uint64_t seed = 0, chunk = 0;
};

// Every argument error of a run, before anything is enqueued or written.  `x0`, `stats`, `totals`, `hist` are only compared with NULL.
int check_run(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist, const double* nominal,
              const EzpzConstraint* records, size_t n_meas, const double* lim_lo, const double* lim_hi, const double* hist_lo,
              const double* hist_hi, uint64_t samples, const EzpzMcConfig* mc_cfg, const void* stats, const void* totals, const void* hist,
              hipStream_t stream, Request& r) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    EzpzMcConfig c;
    ezpz_default_mc_config(&c);
    if (mc_cfg) c = *mc_cfg;
    if (c.hist_bins > kMaxHistBins) return EZPZ_ERR_INVALID_ARGUMENT;
    if ((lim_lo != nullptr) != (lim_hi != nullptr)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (c.hist_bins && n_meas && (!hist_lo || !hist_hi)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (int rc = measure_pack_records(records, n_meas, sys->counts.n_vars, r.words)) return rc;
    r.tab.assign(4 * n_meas, 0.0);
    for (size_t i = 0; i < n_meas; ++i) {
        if (lim_lo) {
            if (!(lim_lo[i] <= lim_hi[i])) return EZPZ_ERR_INVALID_ARGUMENT;
            r.tab[i] = lim_lo[i], r.tab[n_meas + i] = lim_hi[i];
        }
        if (c.hist_bins) {
            if (!(hist_hi[i] > hist_lo[i]) || !std::isfinite(hist_lo[i]) || !std::isfinite(hist_hi[i])) return EZPZ_ERR_INVALID_ARGUMENT;
            r.tab[2 * n_meas + i] = hist_lo[i];
            r.tab[3 * n_meas + i] = (double)c.hist_bins / (hist_hi[i] - hist_lo[i]);
        }
    }
    // the params entry's errors: the list, a system it declines, a capture its fronts refuse
    DrivenRequest driven;
    if (n_param) {
        if (int rc = driven_request(sys, positions, n_param, driven)) return rc;
        if (driven.params_route == EZPZ_PARAMS_ROUTE_FRONTS && sys->fronts->n_wgs > 1 && stream_capturing(stream))
            return EZPZ_ERR_INVALID_ARGUMENT;
    }
    std::vector<double> own;
    if (n_param && !nominal) {
        own.resize(n_param);
        for (size_t j = 0; j < n_param; ++j) own[j] = sys->host_cs[positions[j]].param;
        nominal = own.data();
    }
    if (int rc = check_dists(dist, nominal, n_param, r.dists)) return rc;
    for (size_t j = 0; j < n_param; ++j) r.tab.push_back(nominal[j]);
    if (samples && (!stats || !totals || (c.hist_bins && n_meas && !hist) || (sys->counts.n_vars && !x0))) return EZPZ_ERR_INVALID_ARGUMENT;
    r.limits = lim_lo != nullptr;
    r.hist_bins = c.hist_bins;
    r.seed = c.seed;
    uint64_t chunk = c.chunk;
    if (chunk == 0) {
        chunk = kDefaultChunk;
        while (chunk > kBlock && chunk * std::max<uint64_t>(sys->counts.n_vars, 1) * sizeof(double) > kChunkValueBytes) chunk /= 2;
    }
    chunk = (chunk + kBlock - 1) / kBlock * kBlock;
    r.chunk = std::min<uint64_t>(chunk, (std::max<uint64_t>(samples, 1) + kBlock - 1) / kBlock * kBlock);
    return EZPZ_OK;
}

uint32_t stride_grid(uint64_t items, const EzpzSystem* sys) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, (uint64_t)sys->lim.cus * 16));
}

struct Keep {
    double* params;
    double* m;
    uint8_t* flags;
    uint8_t* ok;
    bool host;  // the keep_* pointers are host memory: a round waits for its launches and copies out
};

// The outputs of a run with contributors (device pointers) and its checked configuration; moments == NULL: the plain run.
struct Contrib {
    double* moments = nullptr;
    EzpzMcMomentsInfo* info = nullptr;
    double *cov = nullptr, *beta = nullptr, *contrib = nullptr, *r2 = nullptr;
    uint64_t* dropped = nullptr;
    double pivot_rel = 0.0;
};

// The argument errors the contributors add to a run's; the pointers are only compared with NULL.
int check_contrib(size_t n_param, size_t n_meas, uint64_t samples, const EzpzMcContribConfig* cc, Contrib& c) {
    if (int rc = mcm::check_shape(n_param, n_meas)) return rc;
    if (int rc = mcm::check_config(cc, c.pivot_rel)) return rc;
    if (samples && (!c.moments || !c.info || !c.cov || !c.dropped || (n_meas && !c.r2) || (n_meas && n_param && (!c.beta || !c.contrib))))
        return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

// The quantiles of a run (probs: host memory; out: a device pointer in run()) and the checked z; n_q == 0: the plain run.
struct Quant {
    const double* probs = nullptr;
    size_t n_q = 0;
    EzpzMcQuantile* out = nullptr;
    double z = 0.0;
};

int copy_out(void* dst, const void* src, size_t bytes, bool host, hipStream_t stream) {
    if (!dst || !bytes) return EZPZ_OK;
    if (host)
        HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    else
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
    return EZPZ_OK;
}

// The run, device pointers throughout (but Keep's, see there): the plan's mutex is held, the system's device current, the request
// checked and samples > 0.
int run(EzpzSystem* sys, McPlan& P, Request& r, const double* x0_dev, const uint32_t* positions, const EzpzConstraint* records,
        uint64_t samples, const EzpzConfig* cfg, EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, uint64_t* hist_dev, const Keep& keep,
        const Contrib& contrib, const Quant& quant, hipStream_t stream) {
    release_thread_kernel(sys->device);
    const size_t n = sys->counts.n_vars, n_param = r.dists.size(), n_meas = r.words.size() / kMeasureRecWords;
    const uint64_t chunk = r.chunk, blocks = chunk / kBlock;
    int rc;
    // ---- what the host writes: behind the last run's launches ----
    std::vector<unsigned char> tables(r.dists.size() * sizeof(mc::Dist) + r.tab.size() * sizeof(double));
    if (!r.dists.empty()) std::memcpy(tables.data(), r.dists.data(), r.dists.size() * sizeof(mc::Dist));
    if (!r.tab.empty()) std::memcpy(tables.data() + r.dists.size() * sizeof(mc::Dist), r.tab.data(), r.tab.size() * sizeof(double));
    const bool new_tables = tables != P.tables_kept;
    const bool grows = chunk * n > P.x_in.cap || chunk * n_param > P.params.cap || chunk * n_meas > P.m.cap || chunk > P.status.cap ||
                       blocks * n_meas * 4 > P.part_f.cap || blocks * (2 * n_meas + 2) > P.part_n.cap || n_meas > P.nominal.cap ||
                       !P.ticket.p || (contrib.moments && P.moment_work.grows(blocks, (uint32_t)(n_param + n_meas)));
    // the rows the selection reads: the caller's device buffers where given, else the plan's
    const bool select = quant.n_q != 0;
    double* all_m = !keep.host && keep.m ? keep.m : nullptr;
    uint8_t* all_flags = !keep.host && keep.flags ? keep.flags : nullptr;
    uint8_t* all_ok = !keep.host && keep.ok ? keep.ok : nullptr;
    const bool select_grows = select && ((!all_m && samples * n_meas > P.all_m.cap) || (!all_flags && samples * n_meas > P.all_flags.cap) ||
                                         (!all_ok && samples > P.all_ok.cap) || P.select_work.grows((uint32_t)n_meas, (uint32_t)quant.n_q));
    if (new_tables || grows || select_grows) {
        if ((rc = P.order.before_overwrite()) != EZPZ_OK) return rc;
        P.tables_kept.clear();
        if ((rc = P.dist.ensure(n_param)) != EZPZ_OK || (rc = P.tab.ensure(r.tab.size())) != EZPZ_OK) return rc;
        if (n_param) HIP_TRY(hipMemcpy(P.dist.p, r.dists.data(), n_param * sizeof(mc::Dist), hipMemcpyHostToDevice));
        if (!r.tab.empty()) HIP_TRY(hipMemcpy(P.tab.p, r.tab.data(), r.tab.size() * sizeof(double), hipMemcpyHostToDevice));
        if ((rc = P.x_in.ensure(chunk * n)) != EZPZ_OK || (rc = P.x_out.ensure(chunk * n)) != EZPZ_OK ||
            (rc = P.params.ensure(chunk * n_param)) != EZPZ_OK || (rc = P.m.ensure(chunk * n_meas)) != EZPZ_OK ||
            (rc = P.flags.ensure(chunk * n_meas)) != EZPZ_OK || (rc = P.status.ensure(chunk)) != EZPZ_OK ||
            (rc = P.ok.ensure(chunk)) != EZPZ_OK || (rc = P.nominal.ensure(n_meas)) != EZPZ_OK ||
            (rc = P.part_f.ensure(blocks * n_meas * 4)) != EZPZ_OK || (rc = P.part_arg.ensure(blocks * n_meas * 2)) != EZPZ_OK ||
            (rc = P.part_n.ensure(blocks * (2 * n_meas + 2))) != EZPZ_OK)
            return rc;
        if (!P.ticket.p) {
            if ((rc = P.ticket.ensure(1)) != EZPZ_OK) return rc;
            HIP_TRY(hipMemset(P.ticket.p, 0, P.ticket.cap * sizeof(unsigned int)));
        }
        if (contrib.moments && (rc = P.moment_work.ensure(blocks, (uint32_t)(n_param + n_meas))) != EZPZ_OK) return rc;
        if (select && ((!all_m && (rc = P.all_m.ensure(samples * n_meas)) != EZPZ_OK) ||
                       (!all_flags && (rc = P.all_flags.ensure(samples * n_meas)) != EZPZ_OK) ||
                       (!all_ok && (rc = P.all_ok.ensure(samples)) != EZPZ_OK) ||
                       (rc = P.select_work.ensure((uint32_t)n_meas, (uint32_t)quant.n_q)) != EZPZ_OK))
            return rc;
        P.tables_kept = std::move(tables);
        call_stamp(MC_TABLES_UPLOADED);
    }
    if ((rc = P.order.order_behind(stream)) != EZPZ_OK) return rc;
    // ---- nominal[i] = m(record i, x0), 0 where the guard fires ----
    if (n_meas && (rc = ezpz_system_measure_device(sys, records, n_meas, x0_dev, 1, P.nominal.p, nullptr, nullptr, stream)) != EZPZ_OK) return rc;
    if (r.hist_bins && n_meas) HIP_TRY(hipMemsetAsync(hist_dev, 0, n_meas * (r.hist_bins + 2) * sizeof(uint64_t), stream));
    mc::ReduceArgs a{};
    a.m = P.m.p;
    a.flags = P.flags.p;
    a.status = P.status.p;
    a.nominal = P.nominal.p;
    a.lim_lo = r.limits ? P.tab.p : nullptr;
    a.lim_hi = r.limits ? P.tab.p + n_meas : nullptr;
    a.hist_lo = P.tab.p + 2 * n_meas;
    a.hist_scale = P.tab.p + 3 * n_meas;
    a.samples = samples;
    a.n_meas = (uint32_t)n_meas;
    a.hist_bins = n_meas ? r.hist_bins : 0;
    a.part_d = P.part_f.p;
    a.part_d2 = a.part_d + blocks * n_meas;
    a.part_min = a.part_d2 + blocks * n_meas;
    a.part_max = a.part_min + blocks * n_meas;
    a.part_argmin = P.part_arg.p;
    a.part_argmax = a.part_argmin + blocks * n_meas;
    a.part_valid = P.part_n.p;
    a.part_in = a.part_valid + blocks * n_meas;
    a.part_ok = a.part_in + blocks * n_meas;
    a.part_all_in = a.part_ok + blocks;
    a.ticket = P.ticket.p;
    a.ok = P.ok.p;
    a.stats = stats_dev;
    a.totals = totals_dev;
    a.hist = hist_dev;
    mcm::MomentArgs mo{};
    mo.params = P.params.p;
    mo.m = P.m.p;
    mo.flags = P.flags.p;
    mo.ok = P.ok.p;
    mo.nominal_p = P.tab.p + 4 * n_meas;
    mo.nominal_m = P.nominal.p;
    mo.samples = samples;
    mo.k = (uint32_t)n_param;
    mo.n_meas = (uint32_t)n_meas;
    mo.moments = contrib.moments;
    mo.info = contrib.info;
    for (uint64_t first = 0; first < samples; first += chunk) {
        const uint64_t count = std::min<uint64_t>(chunk, samples - first);
        if (n_param) hipLaunchKernelGGL(mc::mc_sample_kernel, dim3(stride_grid(count * n_param, sys)), dim3(256), 0, stream, P.dist.p, r.seed, first, count, (uint32_t)n_param, P.params.p);
        if (n) hipLaunchKernelGGL(mc::mc_broadcast_kernel, dim3(stride_grid(count * n, sys)), dim3(256), 0, stream, x0_dev, (uint32_t)n, count, P.x_in.p);
        HIP_TRY(hipGetLastError());
        if ((rc = ezpz_system_solve_batch_params_device(sys, P.x_in.p, positions, n_param, P.params.p, count, cfg, P.x_out.p, P.status.p,
                                                        nullptr, nullptr, 0, stream)) != EZPZ_OK)
            return rc;
        if (n_meas && (rc = ezpz_system_measure_device(sys, records, n_meas, P.x_out.p, count, P.m.p, P.flags.p, nullptr, stream)) != EZPZ_OK)
            return rc;
        a.first = first;
        a.count = count;
        a.first_round = first == 0;
        hipLaunchKernelGGL(mc::mc_reduce_kernel, dim3((uint32_t)((count + kBlock - 1) / kBlock)), dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
        if (contrib.moments) {
            mo.first = first;
            mo.count = count;
            mo.first_round = first == 0;
            if ((rc = mcm::enqueue_moments(P.moment_work, mo, stream)) != EZPZ_OK) return rc;
        }
        if (select) {  // (a caller's device buffer is filled by the copies below)
            if ((rc = copy_out(all_m ? nullptr : P.all_m.p + first * n_meas, P.m.p, count * n_meas * sizeof(double), false, stream)) != EZPZ_OK ||
                (rc = copy_out(all_flags ? nullptr : P.all_flags.p + first * n_meas, P.flags.p, count * n_meas, false, stream)) != EZPZ_OK ||
                (rc = copy_out(all_ok ? nullptr : P.all_ok.p + first, P.ok.p, count, false, stream)) != EZPZ_OK)
                return rc;
        }
        if (keep.params || keep.m || keep.flags || keep.ok) {
            if (keep.host) HIP_TRY(hipStreamSynchronize(stream));
            if ((rc = copy_out(keep.params ? keep.params + first * n_param : nullptr, P.params.p, count * n_param * sizeof(double), keep.host, stream)) != EZPZ_OK ||
                (rc = copy_out(keep.m ? keep.m + first * n_meas : nullptr, P.m.p, count * n_meas * sizeof(double), keep.host, stream)) != EZPZ_OK ||
                (rc = copy_out(keep.flags ? keep.flags + first * n_meas : nullptr, P.flags.p, count * n_meas, keep.host, stream)) != EZPZ_OK ||
                (rc = copy_out(keep.ok ? keep.ok + first : nullptr, P.ok.p, count, keep.host, stream)) != EZPZ_OK)
                return rc;
        }
    }
    if (contrib.moments) {
        mcm::ContribArgs c{};
        c.moments = contrib.moments;
        c.info = contrib.info;
        c.k = (uint32_t)n_param;
        c.m = (uint32_t)n_meas;
        c.pivot_rel = contrib.pivot_rel;
        c.cov = contrib.cov, c.beta = contrib.beta, c.contrib = contrib.contrib, c.r2 = contrib.r2, c.dropped = contrib.dropped;
        if ((rc = mcm::enqueue_contributors(c, stream)) != EZPZ_OK) return rc;
    }
    if (select && (rc = mcq::enqueue_select(P.select_work, all_m ? all_m : P.all_m.p, all_flags ? all_flags : P.all_flags.p,
                                            all_ok ? all_ok : P.all_ok.p, samples, (uint32_t)n_meas, quant.probs, (uint32_t)quant.n_q, quant.z,
                                            quant.out, sys->lim.cus, stream)) != EZPZ_OK)
        return rc;
    call_stamp(MC_LAUNCHED);
    return P.order.record(stream);
}

// The device form of both runs: the request checked, then the rounds.
int run_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist, const double* nominal,
               const EzpzConstraint* records, size_t n_meas, const double* lim_lo, const double* lim_hi, const double* hist_lo,
               const double* hist_hi, uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats_dev,
               EzpzMcTotals* totals_dev, uint64_t* hist_dev, const Keep& keep, const EzpzMcContribConfig* cc, Contrib* contrib,
               const EzpzMcQuantileConfig* qc, Quant* quant, hipStream_t stream) {
    Request r;
    if (int rc = check_run(sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg,
                           stats_dev, totals_dev, hist_dev, stream, r))
        return rc;
    if (contrib)
        if (int rc = check_contrib(n_param, n_meas, samples, cc, *contrib)) return rc;
    if (quant)
        if (int rc = mcq::check(samples, n_meas, quant->probs, quant->n_q, qc, sys, quant->out, quant->z)) return rc;  // (the rows are the run's own)
    if (samples == 0) return EZPZ_OK;
    McPlan& P = plan_of(sys);
    std::lock_guard<std::mutex> lock(P.mu);
    EZPZ_ON_DEVICE(sys->device);
    return run(sys, P, r, x0_dev, positions, records, samples, cfg, stats_dev, totals_dev, hist_dev, keep, contrib ? *contrib : Contrib{},
               quant ? *quant : Quant{}, stream);
}

// The host form of both runs: the plan's buffers for x0 and the outputs, the rounds, the copies back once the stream has drained.
// `contrib` holds host pointers here.
int run_host(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist, const double* nominal,
             const EzpzConstraint* records, size_t n_meas, const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
             uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats, EzpzMcTotals* totals, uint64_t* hist,
             const Keep& keep, const EzpzMcContribConfig* cc, Contrib* contrib, const EzpzMcQuantileConfig* qc, Quant* quant) {
    Request r;
    if (int rc = check_run(sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, stats,
                           totals, hist, hipStreamPerThread, r))
        return rc;
    if (contrib)
        if (int rc = check_contrib(n_param, n_meas, samples, cc, *contrib)) return rc;
    if (quant)
        if (int rc = mcq::check(samples, n_meas, quant->probs, quant->n_q, qc, sys, quant->out, quant->z)) return rc;  // (the rows are the run's own)
    if (samples == 0) return EZPZ_OK;
    McPlan& P = plan_of(sys);
    std::lock_guard<std::mutex> lock(P.mu);
    EZPZ_ON_DEVICE(sys->device);
    const size_t n = sys->counts.n_vars, hist_words = n_meas * (r.hist_bins ? r.hist_bins + 2 : 0);
    const size_t K = n_param + n_meas, E = contrib ? mcm::entries_of((uint32_t)K) : 0, km = n_param * n_meas;
    int rc;
    // (the buffers of an earlier host call are idle: it waited for its launches)
    if ((rc = P.x0_in.ensure(n)) != EZPZ_OK || (rc = P.stats_out.ensure(n_meas)) != EZPZ_OK || (rc = P.totals_out.ensure(1)) != EZPZ_OK ||
        (rc = P.hist_out.ensure(hist_words)) != EZPZ_OK)
        return rc;
    Contrib dev;
    if (contrib) {
        if ((rc = P.contrib_out.ensure(E + K * K + 2 * km + n_meas)) != EZPZ_OK || (rc = P.contrib_words.ensure(3)) != EZPZ_OK) return rc;
        dev.moments = P.contrib_out.p;
        dev.cov = dev.moments + E;
        dev.beta = dev.cov + K * K;
        dev.contrib = dev.beta + km;
        dev.r2 = dev.contrib + km;
        dev.info = reinterpret_cast<EzpzMcMomentsInfo*>(P.contrib_words.p);
        dev.dropped = P.contrib_words.p + 2;
        dev.pivot_rel = contrib->pivot_rel;
    }
    Quant qdev;
    if (quant && quant->n_q) {
        if ((rc = P.quant_out.ensure(n_meas * quant->n_q)) != EZPZ_OK) return rc;
        qdev = *quant;
        qdev.out = P.quant_out.p;
    }
    if (n) HIP_TRY(hipMemcpy(P.x0_in.p, x0, n * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = run(sys, P, r, P.x0_in.p, positions, records, samples, cfg, P.stats_out.p, P.totals_out.p, P.hist_out.p, keep, dev, qdev,
                  hipStreamPerThread)) != EZPZ_OK)
        return rc;
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    if (n_meas) HIP_TRY(hipMemcpy(stats, P.stats_out.p, n_meas * sizeof(EzpzMcStats), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(totals, P.totals_out.p, sizeof(EzpzMcTotals), hipMemcpyDeviceToHost));
    if (hist_words) HIP_TRY(hipMemcpy(hist, P.hist_out.p, hist_words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (contrib) {
        HIP_TRY(hipMemcpy(contrib->moments, dev.moments, E * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(contrib->cov, dev.cov, K * K * sizeof(double), hipMemcpyDeviceToHost));
        if (km) HIP_TRY(hipMemcpy(contrib->beta, dev.beta, km * sizeof(double), hipMemcpyDeviceToHost));
        if (km) HIP_TRY(hipMemcpy(contrib->contrib, dev.contrib, km * sizeof(double), hipMemcpyDeviceToHost));
        if (n_meas) HIP_TRY(hipMemcpy(contrib->r2, dev.r2, n_meas * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(contrib->info, dev.info, sizeof(EzpzMcMomentsInfo), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(contrib->dropped, dev.dropped, sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (qdev.n_q) HIP_TRY(hipMemcpy(quant->out, qdev.out, n_meas * qdev.n_q * sizeof(EzpzMcQuantile), hipMemcpyDeviceToHost));
    return EZPZ_OK;
}

// ---- the run with Sobol indices (ezpz_system_tolerance_sobol[_device]) -----------------------------------------------
// The same plan, the same kernels and entries as run(), which stays what it is: a round is k' + 2 sub-rounds -- pick sampler, copies
// of x0, the params entry, the measure entry into the round's rows -- with mc_reduce_kernel behind A's, mc_sobol_kernel behind the
// last one and the closing kernel behind the last round.
struct SobolOut {  // the outputs (device pointers in run_sobol) and the checked configuration
    double* sums = nullptr;
    uint64_t* n_complete = nullptr;
    double *var = nullptr, *first = nullptr, *total = nullptr, *first_var = nullptr, *total_var = nullptr;
    uint64_t seed_b = 0;
    uint32_t fixed_mask = 0;
};

struct KeepRows {
    double* f;
    uint8_t *flags, *ok;
    bool host;  // host memory: a round waits for its launches and copies out
};

// The argument errors the indices add to a run's, and the run's chunk; the pointers are only compared with NULL.
int check_sobol(const EzpzSystem* sys, size_t n_param, size_t n_meas, uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzSobolConfig* sc,
                Request& r, SobolOut& o) {
    if (int rc = sobol::check_shape(n_param, n_meas)) return rc;
    EzpzSobolConfig c;
    sobol::default_config(&c);
    if (sc) c = *sc;
    if (c.seed_b == r.seed) return EZPZ_ERR_INVALID_ARGUMENT;
    o.seed_b = c.seed_b;
    o.fixed_mask = 0;
    for (size_t j = 0; j < n_param; ++j) {
        if (r.dists[j].kind == EZPZ_MC_CORNER) return EZPZ_ERR_INVALID_ARGUMENT;
        if (r.dists[j].kind == EZPZ_MC_FIXED) o.fixed_mask |= 1u << j;
    }
    if (samples && (!o.sums || !o.n_complete || !o.var || (n_param && (!o.first || !o.total || !o.first_var || !o.total_var))))
        return EZPZ_ERR_INVALID_ARGUMENT;
    if (!(mc_cfg && mc_cfg->chunk)) {  // the library's choice: the rows and the copies of x0 each below the round's bound
        const uint64_t per_sample = std::max<uint64_t>({(uint64_t)sys->counts.n_vars, (uint64_t)(n_param + 2) * n_meas, 1}) * sizeof(double);
        const uint64_t chunk = std::max<uint64_t>(std::min<uint64_t>(kChunkValueBytes / per_sample, kDefaultChunk) / kBlock * kBlock, kBlock);
        r.chunk = std::min<uint64_t>(chunk, (std::max<uint64_t>(samples, 1) + kBlock - 1) / kBlock * kBlock);
    }
    return EZPZ_OK;
}

// rows of `width` bytes, `height` of them, between pitched arrays
int copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, bool host, hipStream_t stream) {
    if (!dst || !width || !height) return EZPZ_OK;
    if (host)
        HIP_TRY(hipMemcpy2D(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost));
    else
        HIP_TRY(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, stream));
    return EZPZ_OK;
}

// Device pointers throughout (but KeepRows', see there): the plan's mutex is held, the system's device current, the request checked
// and samples > 0.
int run_sobol(EzpzSystem* sys, McPlan& P, Request& r, const double* x0_dev, const uint32_t* positions, const EzpzConstraint* records,
              uint64_t samples, const EzpzConfig* cfg, EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, const SobolOut& out,
              const KeepRows& keep, hipStream_t stream) {
    release_thread_kernel(sys->device);
    const size_t n = sys->counts.n_vars, n_param = r.dists.size(), n_meas = r.words.size() / kMeasureRecWords, R = n_param + 2;
    const uint64_t chunk = r.chunk, blocks = chunk / kBlock;
    int rc;
    // ---- what the host writes: behind the last run's launches ----
    std::vector<unsigned char> tables(r.dists.size() * sizeof(mc::Dist) + r.tab.size() * sizeof(double));
    if (!r.dists.empty()) std::memcpy(tables.data(), r.dists.data(), r.dists.size() * sizeof(mc::Dist));
    if (!r.tab.empty()) std::memcpy(tables.data() + r.dists.size() * sizeof(mc::Dist), r.tab.data(), r.tab.size() * sizeof(double));
    const bool new_tables = tables != P.tables_kept;
    const bool grows = chunk * n > P.x_in.cap || chunk * n_param > P.params.cap || chunk > P.status.cap || blocks * n_meas * 4 > P.part_f.cap ||
                       blocks * (2 * n_meas + 2) > P.part_n.cap || n_meas > P.nominal.cap || !P.ticket.p || R * chunk * n_meas > P.rows_f.cap ||
                       R * chunk > P.rows_ok.cap || P.sobol_work.grows(blocks, (uint32_t)n_param, (uint32_t)n_meas);
    if (new_tables || grows) {
        if ((rc = P.order.before_overwrite()) != EZPZ_OK) return rc;
        P.tables_kept.clear();
        if ((rc = P.dist.ensure(n_param)) != EZPZ_OK || (rc = P.tab.ensure(r.tab.size())) != EZPZ_OK) return rc;
        if (n_param) HIP_TRY(hipMemcpy(P.dist.p, r.dists.data(), n_param * sizeof(mc::Dist), hipMemcpyHostToDevice));
        if (!r.tab.empty()) HIP_TRY(hipMemcpy(P.tab.p, r.tab.data(), r.tab.size() * sizeof(double), hipMemcpyHostToDevice));
        if ((rc = P.x_in.ensure(chunk * n)) != EZPZ_OK || (rc = P.x_out.ensure(chunk * n)) != EZPZ_OK ||
            (rc = P.params.ensure(chunk * n_param)) != EZPZ_OK || (rc = P.status.ensure(chunk)) != EZPZ_OK ||
            (rc = P.nominal.ensure(n_meas)) != EZPZ_OK || (rc = P.part_f.ensure(blocks * n_meas * 4)) != EZPZ_OK ||
            (rc = P.part_arg.ensure(blocks * n_meas * 2)) != EZPZ_OK || (rc = P.part_n.ensure(blocks * (2 * n_meas + 2))) != EZPZ_OK ||
            (rc = P.rows_f.ensure(R * chunk * n_meas)) != EZPZ_OK || (rc = P.rows_flags.ensure(R * chunk * n_meas)) != EZPZ_OK ||
            (rc = P.rows_ok.ensure(R * chunk)) != EZPZ_OK)
            return rc;
        if (!P.ticket.p) {
            if ((rc = P.ticket.ensure(1)) != EZPZ_OK) return rc;
            HIP_TRY(hipMemset(P.ticket.p, 0, P.ticket.cap * sizeof(unsigned int)));
        }
        if ((rc = P.sobol_work.ensure(blocks, (uint32_t)n_param, (uint32_t)n_meas)) != EZPZ_OK) return rc;
        P.tables_kept = std::move(tables);
        call_stamp(MC_TABLES_UPLOADED);
    }
    if ((rc = P.order.order_behind(stream)) != EZPZ_OK) return rc;
    if ((rc = ezpz_system_measure_device(sys, records, n_meas, x0_dev, 1, P.nominal.p, nullptr, nullptr, stream)) != EZPZ_OK) return rc;
    mc::ReduceArgs a{};  // A's rows through the plain run's reduction: no limits, no histogram
    a.m = P.rows_f.p;
    a.flags = P.rows_flags.p;
    a.status = P.status.p;
    a.nominal = P.nominal.p;
    a.hist_lo = P.tab.p + 2 * n_meas;
    a.hist_scale = P.tab.p + 3 * n_meas;
    a.samples = samples;
    a.n_meas = (uint32_t)n_meas;
    a.part_d = P.part_f.p;
    a.part_d2 = a.part_d + blocks * n_meas;
    a.part_min = a.part_d2 + blocks * n_meas;
    a.part_max = a.part_min + blocks * n_meas;
    a.part_argmin = P.part_arg.p;
    a.part_argmax = a.part_argmin + blocks * n_meas;
    a.part_valid = P.part_n.p;
    a.part_in = a.part_valid + blocks * n_meas;
    a.part_ok = a.part_in + blocks * n_meas;
    a.part_all_in = a.part_ok + blocks;
    a.ticket = P.ticket.p;
    a.ok = P.rows_ok.p;
    a.stats = stats_dev;
    a.totals = totals_dev;
    sobol::SumArgs su{};
    su.f = P.rows_f.p;
    su.flags = P.rows_flags.p;
    su.ok = P.rows_ok.p;
    su.nominal_m = P.nominal.p;
    su.stride_s = n_meas, su.stride_r = chunk * n_meas;
    su.ok_stride_s = 1, su.ok_stride_r = chunk;
    su.k = (uint32_t)n_param, su.m = (uint32_t)n_meas, su.fixed_mask = out.fixed_mask;
    su.sums = out.sums;
    su.n_complete = out.n_complete;
    for (uint64_t first = 0; first < samples; first += chunk) {
        const uint64_t count = std::min<uint64_t>(chunk, samples - first);
        for (size_t row = 0; row < R; ++row) {
            if (row >= 2 && ((out.fixed_mask >> (row - 2)) & 1u)) continue;  // AB_j == A: not solved
            const uint32_t pick = row == 0 ? mc::kPickNone : row == 1 ? mc::kPickAll : (uint32_t)(row - 2);
            if (n_param) hipLaunchKernelGGL(mc::mc_sample_pick_kernel, dim3(stride_grid(count * n_param, sys)), dim3(256), 0, stream, P.dist.p, r.seed, out.seed_b, pick, first, count, (uint32_t)n_param, P.params.p);
            if (n) hipLaunchKernelGGL(mc::mc_broadcast_kernel, dim3(stride_grid(count * n, sys)), dim3(256), 0, stream, x0_dev, (uint32_t)n, count, P.x_in.p);
            HIP_TRY(hipGetLastError());
            if ((rc = ezpz_system_solve_batch_params_device(sys, P.x_in.p, positions, n_param, P.params.p, count, cfg, P.x_out.p, P.status.p,
                                                            nullptr, nullptr, 0, stream)) != EZPZ_OK)
                return rc;
            if ((rc = ezpz_system_measure_device(sys, records, n_meas, P.x_out.p, count, P.rows_f.p + row * chunk * n_meas,
                                                 P.rows_flags.p + row * chunk * n_meas, nullptr, stream)) != EZPZ_OK)
                return rc;
            if (row == 0) {
                a.first = first;
                a.count = count;
                a.first_round = first == 0;
                hipLaunchKernelGGL(mc::mc_reduce_kernel, dim3((uint32_t)((count + kBlock - 1) / kBlock)), dim3(256), 0, stream, a);
                HIP_TRY(hipGetLastError());
            } else if ((rc = sobol::enqueue_ok(P.status.p, count, P.rows_ok.p + row * chunk, stream)) != EZPZ_OK) {
                return rc;
            }
        }
        su.count = count;
        su.first_round = first == 0;
        if ((rc = sobol::enqueue_sums(P.sobol_work, su, stream)) != EZPZ_OK) return rc;
        if (keep.f || keep.flags || keep.ok) {
            if (keep.host) HIP_TRY(hipStreamSynchronize(stream));
            for (size_t row = 0; row < R; ++row) {
                const size_t src = row >= 2 && ((out.fixed_mask >> (row - 2)) & 1u) ? 0 : row;  // (a FIXED j: a copy of row 0)
                if ((rc = copy_rows(keep.f ? keep.f + (first * R + row) * n_meas : nullptr, R * n_meas * sizeof(double), P.rows_f.p + src * chunk * n_meas,
                                    n_meas * sizeof(double), n_meas * sizeof(double), count, keep.host, stream)) != EZPZ_OK ||
                    (rc = copy_rows(keep.flags ? keep.flags + (first * R + row) * n_meas : nullptr, R * n_meas, P.rows_flags.p + src * chunk * n_meas,
                                    n_meas, n_meas, count, keep.host, stream)) != EZPZ_OK ||
                    (rc = copy_rows(keep.ok ? keep.ok + first * R + row : nullptr, R, P.rows_ok.p + src * chunk, 1, 1, count, keep.host, stream)) != EZPZ_OK)
                    return rc;
            }
        }
    }
    sobol::CloseArgs c{};
    c.sums = out.sums;
    c.n_complete = out.n_complete;
    c.k = (uint32_t)n_param, c.m = (uint32_t)n_meas;
    c.var = out.var, c.first = out.first, c.total = out.total, c.first_var = out.first_var, c.total_var = out.total_var;
    if ((rc = sobol::enqueue_close(c, stream)) != EZPZ_OK) return rc;
    call_stamp(MC_LAUNCHED);
    return P.order.record(stream);
}

int sobol_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist, const double* nominal,
                 const EzpzConstraint* records, size_t n_meas, uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg,
                 const EzpzSobolConfig* sc, EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, SobolOut& out, const KeepRows& keep,
                 hipStream_t stream) {
    Request r;
    if (int rc = check_run(sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, nullptr, nullptr, nullptr, nullptr, samples, mc_cfg,
                           stats_dev, totals_dev, nullptr, stream, r))
        return rc;
    if (int rc = check_sobol(sys, n_param, n_meas, samples, mc_cfg, sc, r, out)) return rc;
    if (samples == 0) return EZPZ_OK;
    McPlan& P = plan_of(sys);
    std::lock_guard<std::mutex> lock(P.mu);
    EZPZ_ON_DEVICE(sys->device);
    return run_sobol(sys, P, r, x0_dev, positions, records, samples, cfg, stats_dev, totals_dev, out, keep, stream);
}

// `out` holds host pointers here.
int sobol_host(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist, const double* nominal,
               const EzpzConstraint* records, size_t n_meas, uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg,
               const EzpzSobolConfig* sc, EzpzMcStats* stats, EzpzMcTotals* totals, SobolOut& out, const KeepRows& keep) {
    Request r;
    if (int rc = check_run(sys, x0, positions, n_param, dist, nominal, records, n_meas, nullptr, nullptr, nullptr, nullptr, samples, mc_cfg, stats,
                           totals, nullptr, hipStreamPerThread, r))
        return rc;
    if (int rc = check_sobol(sys, n_param, n_meas, samples, mc_cfg, sc, r, out)) return rc;
    if (samples == 0) return EZPZ_OK;
    McPlan& P = plan_of(sys);
    std::lock_guard<std::mutex> lock(P.mu);
    EZPZ_ON_DEVICE(sys->device);
    const size_t n = sys->counts.n_vars, E = n_meas * sobol::width_of((uint32_t)n_param), km = n_param * n_meas;
    int rc;
    // (the buffers of an earlier host call are idle: it waited for its launches)
    if ((rc = P.x0_in.ensure(n)) != EZPZ_OK || (rc = P.stats_out.ensure(n_meas)) != EZPZ_OK || (rc = P.totals_out.ensure(1)) != EZPZ_OK ||
        (rc = P.sobol_out.ensure(E + n_meas + 4 * km)) != EZPZ_OK || (rc = P.sobol_words.ensure(n_meas)) != EZPZ_OK)
        return rc;
    SobolOut dev = out;
    dev.sums = P.sobol_out.p;
    dev.var = dev.sums + E;
    dev.first = dev.var + n_meas;
    dev.total = dev.first + km;
    dev.first_var = dev.total + km;
    dev.total_var = dev.first_var + km;
    dev.n_complete = P.sobol_words.p;
    if (n) HIP_TRY(hipMemcpy(P.x0_in.p, x0, n * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = run_sobol(sys, P, r, P.x0_in.p, positions, records, samples, cfg, P.stats_out.p, P.totals_out.p, dev, keep, hipStreamPerThread)) != EZPZ_OK)
        return rc;
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    HIP_TRY(hipMemcpy(stats, P.stats_out.p, n_meas * sizeof(EzpzMcStats), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(totals, P.totals_out.p, sizeof(EzpzMcTotals), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out.sums, dev.sums, E * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out.n_complete, dev.n_complete, n_meas * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out.var, dev.var, n_meas * sizeof(double), hipMemcpyDeviceToHost));
    if (km) {
        HIP_TRY(hipMemcpy(out.first, dev.first, km * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out.total, dev.total, km * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out.first_var, dev.first_var, km * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out.total_var, dev.total_var, km * sizeof(double), hipMemcpyDeviceToHost));
    }
    return EZPZ_OK;
}

}  // namespace

extern "C" {

void ezpz_default_mc_config(EzpzMcConfig* mc_cfg) {
    if (!mc_cfg) return;
    mc_cfg->seed = 0;
    mc_cfg->chunk = 0;
    mc_cfg->hist_bins = 0;
}

int ezpz_mc_sample(uint64_t seed, const EzpzMcDist* dist, const double* nominal, size_t n_param, uint64_t first, size_t count,
                   double* params_out) {
    std::vector<mc::Dist> dists;
    if (int rc = check_dists(dist, nominal, n_param, dists)) return rc;
    if (count && n_param && !params_out) return EZPZ_ERR_INVALID_ARGUMENT;
    for (size_t s = 0; s < count; ++s)
        for (size_t j = 0; j < n_param; ++j) params_out[s * n_param + j] = mc::draw(seed, first + s, (uint32_t)j, dists[j]);
    return EZPZ_OK;
}

int ezpz_system_tolerance_mc_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                    const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo,
                                    const double* lim_hi, const double* hist_lo, const double* hist_hi, uint64_t samples,
                                    const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev,
                                    uint64_t* hist_dev, double* keep_params_dev, double* keep_m_dev, uint8_t* keep_flags_dev,
                                    uint8_t* keep_ok_dev, void* stream) {
    return run_device(sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                      stats_dev, totals_dev, hist_dev, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, nullptr, nullptr,
                      nullptr, nullptr, (hipStream_t)stream);
}

int ezpz_system_tolerance_mc(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                             const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo, const double* lim_hi,
                             const double* hist_lo, const double* hist_hi, uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg,
                             EzpzMcStats* stats, EzpzMcTotals* totals, uint64_t* hist, double* keep_params, double* keep_m,
                             uint8_t* keep_flags, uint8_t* keep_ok) {
    return run_host(sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg, stats,
                    totals, hist, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, nullptr, nullptr, nullptr, nullptr);
}

int ezpz_system_tolerance_mc_contrib_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                            const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                            const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                            uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats_dev,
                                            EzpzMcTotals* totals_dev, uint64_t* hist_dev, double* keep_params_dev, double* keep_m_dev,
                                            uint8_t* keep_flags_dev, uint8_t* keep_ok_dev, const EzpzMcContribConfig* cc, double* moments_dev,
                                            EzpzMcMomentsInfo* info_dev, double* cov_dev, double* beta_dev, double* contrib_dev,
                                            double* r2_dev, uint64_t* dropped_dev, void* stream) {
    Contrib c;
    c.moments = moments_dev, c.info = info_dev, c.cov = cov_dev, c.beta = beta_dev, c.contrib = contrib_dev, c.r2 = r2_dev, c.dropped = dropped_dev;
    return run_device(sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                      stats_dev, totals_dev, hist_dev, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, cc, &c,
                      nullptr, nullptr, (hipStream_t)stream);
}

int ezpz_system_tolerance_mc_contrib(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                     const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo,
                                     const double* lim_hi, const double* hist_lo, const double* hist_hi, uint64_t samples,
                                     const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats, EzpzMcTotals* totals,
                                     uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags, uint8_t* keep_ok,
                                     const EzpzMcContribConfig* cc, double* moments, EzpzMcMomentsInfo* info, double* cov, double* beta,
                                     double* contrib, double* r2, uint64_t* dropped) {
    Contrib c;
    c.moments = moments, c.info = info, c.cov = cov, c.beta = beta, c.contrib = contrib, c.r2 = r2, c.dropped = dropped;
    return run_host(sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg, stats,
                    totals, hist, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, cc, &c, nullptr, nullptr);
}

int ezpz_system_tolerance_mc_quantiles_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                              const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records,
                                              size_t n_meas, const double* lim_lo, const double* lim_hi, const double* hist_lo,
                                              const double* hist_hi, uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg,
                                              EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, uint64_t* hist_dev,
                                              double* keep_params_dev, double* keep_m_dev, uint8_t* keep_flags_dev,
                                              uint8_t* keep_ok_dev, const double* probs, size_t n_q, const EzpzMcQuantileConfig* qc,
                                              EzpzMcQuantile* out_dev, void* stream) {
    Quant q;
    q.probs = probs, q.n_q = n_q, q.out = out_dev;
    return run_device(sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                      stats_dev, totals_dev, hist_dev, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, nullptr, nullptr,
                      qc, &q, (hipStream_t)stream);
}

int ezpz_system_tolerance_mc_quantiles(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param,
                                       const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                       const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                       uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats,
                                       EzpzMcTotals* totals, uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags,
                                       uint8_t* keep_ok, const double* probs, size_t n_q, const EzpzMcQuantileConfig* qc,
                                       EzpzMcQuantile* out) {
    Quant q;
    q.probs = probs, q.n_q = n_q, q.out = out;
    return run_host(sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg, stats,
                    totals, hist, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, nullptr, nullptr, qc, &q);
}

int ezpz_system_tolerance_sobol_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                       const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                       uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, const EzpzSobolConfig* sc,
                                       EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, double* sums_dev, uint64_t* n_complete_dev,
                                       double* var_dev, double* first_dev, double* total_dev, double* first_var_dev, double* total_var_dev,
                                       double* keep_f_dev, uint8_t* keep_flags_dev, uint8_t* keep_ok_dev, void* stream) {
    SobolOut o;
    o.sums = sums_dev, o.n_complete = n_complete_dev, o.var = var_dev, o.first = first_dev, o.total = total_dev;
    o.first_var = first_var_dev, o.total_var = total_var_dev;
    return sobol_device(sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, samples, mc_cfg, cfg, sc, stats_dev, totals_dev, o,
                        KeepRows{keep_f_dev, keep_flags_dev, keep_ok_dev, false}, (hipStream_t)stream);
}

int ezpz_system_tolerance_sobol(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                const double* nominal, const EzpzConstraint* records, size_t n_meas, uint64_t samples,
                                const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, const EzpzSobolConfig* sc, EzpzMcStats* stats,
                                EzpzMcTotals* totals, double* sums, uint64_t* n_complete, double* var, double* first, double* total,
                                double* first_var, double* total_var, double* keep_f, uint8_t* keep_flags, uint8_t* keep_ok) {
    SobolOut o;
    o.sums = sums, o.n_complete = n_complete, o.var = var, o.first = first, o.total = total, o.first_var = first_var, o.total_var = total_var;
    return sobol_host(sys, x0, positions, n_param, dist, nominal, records, n_meas, samples, mc_cfg, cfg, sc, stats, totals, o,
                      KeepRows{keep_f, keep_flags, keep_ok, true});
}

}  // extern "C"
