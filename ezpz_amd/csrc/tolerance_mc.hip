// Monte-Carlo tolerance analysis (include/ezpz_amd.h: ezpz_mc_sample, ezpz_system_tolerance_mc and its _device form; DESIGN.md
// 3k): the host side of tolerance_mc.hip.hpp's kernels -- the check of a request, the plan a system keeps (the round's workspace,
// the sampler's and the limits' tables, the host forms' buffers) and the rounds.  Every kind of run is one pipeline with a tail of
// its own.  enter() checks the request and takes the plan; prepare() brings the plan's tables and buffers to what the run needs --
// Needs lists every buffer with its count once, and both "does anything grow" and "grow it" are that list -- and measures the
// nominal; sub_round() is sampler -> copies of x0 -> ezpz_system_solve_batch_params_device -> ezpz_system_measure_device, all on
// the caller's stream: the driven solve and the measurement are those entries themselves, with their routes, their locks and their
// ordering.  What a kind adds stands in its run function alone:
//   run()        one sub-round a round and the reduction behind it; with contributors (ezpz_system_tolerance_mc_contrib[_device];
//                DESIGN.md 3n) one more enqueue per round behind the reduction -- mc_moments.hip's, on the round's params, m, flags
//                and ok -- and the closing kernel behind the last round; with quantiles (ezpz_system_tolerance_mc_quantiles[_device];
//                DESIGN.md 3p) every round's m, flags and ok kept on the device, mc_quantiles.hip's selection behind the last round;
//                with effects (ezpz_system_tolerance_mc_effects[_device]) one more enqueue per round behind the
//                reduction -- mc_effects.hip's, on the same four arrays and the run's edges -- and its closing kernel behind the last
//                round; with factorial effects (ezpz_system_tolerance_mc_factorial[_device]) every round's m, flags and ok
//                kept on the device as for the quantiles, mc_factorial.hip's transform behind the last round
//   run_sobol()  (ezpz_system_tolerance_sobol[_device]) k' + 2 sub-rounds a round into the round's rows, the reduction
//                behind A's, mc_sobol.hip's sums behind the last one and its closing kernel behind the last round
// A host form is its run between the upload of x0 and the copies back of its Staged outputs.
#include "driven_params.hpp"
#include "mc_effects.hip.hpp"
#include "mc_factorial.hip.hpp"
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
// samples per round where the caller leaves the choice: kDefaultSampleChunk, while one of the round's two value arrays stays below
constexpr uint64_t kChunkValueBytes = 256ull << 20;

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
    // the host forms' buffers: x0, and every output of the call side by side (Staged below)
    DevBuf<double> x0_in;
    DevBuf<unsigned char> host_out;
    // the run with contributors: the moments' workspace
    mcm::MomentWork moment_work;
    // the run with Sobol indices: the round's rows -- [k + 2][chunk][n_meas] values and flags, [k + 2][chunk] ok bytes
    // -- and the sums' workspace
    DevBuf<double> rows_f;
    DevBuf<uint8_t> rows_flags, rows_ok;
    sobol::SumWork sobol_work;
    // the run with quantiles: every sample's m, flags and ok -- samples x n_meas x 9 + samples bytes, the one
    // workspace here that grows with samples -- and the selection's workspace
    DevBuf<double> all_m;
    DevBuf<uint8_t> all_flags, all_ok;
    mcq::SelectWork select_work;
    // the run with effects: the cells' workspace, and the edges [k][bins - 1] with what the buffer holds
    mce::EffectWork effect_work;
    DevBuf<double> effect_edges;
    std::vector<double> effect_edges_kept;
    // the run with factorial effects: the rows in all_m, all_flags and all_ok as for the quantiles, and the transform's
    // workspace -- the [n_meas][2^kc] work array and the block sums
    mcf::FactorialWork factorial_work;
};

McPlan& plan_of(EzpzSystem* sys) {
    std::lock_guard<std::mutex> lock(sys->mu);
    if (!sys->tolerance_mc) sys->tolerance_mc = std::make_shared<McPlan>();
    return *static_cast<McPlan*>(sys->tolerance_mc.get());
}

// What every entry is given, as given: a device form's pointers and stream, or a host form's pointers and hipStreamPerThread.  (The
// Sobol entries have no limits and no histogram.)
struct Call {
    EzpzSystem* sys;
    const double* x0;
    const uint32_t* positions;  // the driving dimensions: [n_param], with their dist and nominal
    size_t n_param;
    const EzpzMcDist* dist;
    const double* nominal;
    const EzpzConstraint* records;  // the reference dimensions: [n_meas], with their limits and histogram ranges
    size_t n_meas;
    const double *lim_lo, *lim_hi, *hist_lo, *hist_hi;
    uint64_t samples;
    const EzpzMcConfig* mc_cfg;
    const EzpzConfig* cfg;
    EzpzMcStats* stats;    // the outputs every kind has
    EzpzMcTotals* totals;
    uint64_t* hist;
    hipStream_t stream;
};

struct Request {
    std::vector<mc::Dist> dists;
    std::vector<uint32_t> words;  // the packed measurement records (compared by the measure entry against its kept list)
    std::vector<double> tab;      // lim_lo | lim_hi | hist_lo | hist_scale | the draw's nominal
    bool limits = false;
    bool sequence = false;  // some dimension is flagged (EZPZ_MC_SEQUENCE): the round's sampler is the walk
    uint32_t hist_bins = 0;
    uint64_t seed = 0, chunk = 0;
};

uint64_t whole_blocks(uint64_t samples) { return (std::max<uint64_t>(samples, 1) + kBlock - 1) / kBlock * kBlock; }

// Every argument error of a run, before anything is enqueued or written.  `x0`, `stats`, `totals`, `hist` are only compared with NULL.
int check_run(const Call& c, Request& r) {
    EzpzSystem* sys = c.sys;
    const size_t n_param = c.n_param, n_meas = c.n_meas;
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    EzpzMcConfig conf;
    ezpz_default_mc_config(&conf);
    if (c.mc_cfg) conf = *c.mc_cfg;
    if (conf.hist_bins > kMaxHistBins) return EZPZ_ERR_INVALID_ARGUMENT;
    if ((c.lim_lo != nullptr) != (c.lim_hi != nullptr)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (conf.hist_bins && n_meas && (!c.hist_lo || !c.hist_hi)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (int rc = measure_pack_records(c.records, n_meas, sys->counts.n_vars, r.words)) return rc;
    r.tab.assign(4 * n_meas, 0.0);
    for (size_t i = 0; i < n_meas; ++i) {
        if (c.lim_lo) {
            if (!(c.lim_lo[i] <= c.lim_hi[i])) return EZPZ_ERR_INVALID_ARGUMENT;
            r.tab[i] = c.lim_lo[i], r.tab[n_meas + i] = c.lim_hi[i];
        }
        if (conf.hist_bins) {
            if (!(c.hist_hi[i] > c.hist_lo[i]) || !std::isfinite(c.hist_lo[i]) || !std::isfinite(c.hist_hi[i])) return EZPZ_ERR_INVALID_ARGUMENT;
            r.tab[2 * n_meas + i] = c.hist_lo[i];
            r.tab[3 * n_meas + i] = (double)conf.hist_bins / (c.hist_hi[i] - c.hist_lo[i]);
        }
    }
    // the params entry's errors: the list, a system it declines, a capture its fronts refuse
    DrivenRequest driven;
    if (n_param) {
        if (int rc = driven_request(sys, c.positions, n_param, driven)) return rc;
        if (driven.params_route == EZPZ_PARAMS_ROUTE_FRONTS && sys->fronts->n_wgs > 1 && stream_capturing(c.stream))
            return EZPZ_ERR_INVALID_ARGUMENT;
    }
    const double* nominal = c.nominal;
    std::vector<double> own;
    if (n_param && !nominal) {
        own.resize(n_param);
        for (size_t j = 0; j < n_param; ++j) own[j] = sys->host_cs[c.positions[j]].param;
        nominal = own.data();
    }
    if (int rc = mc::check_dists(c.dist, nominal, n_param, 0, c.samples, r.dists)) return rc;
    for (const mc::Dist& d : r.dists) r.sequence = r.sequence || d.sequence != 0;
    for (size_t j = 0; j < n_param; ++j) r.tab.push_back(nominal[j]);
    if (c.samples && (!c.stats || !c.totals || (conf.hist_bins && n_meas && !c.hist) || (sys->counts.n_vars && !c.x0))) return EZPZ_ERR_INVALID_ARGUMENT;
    r.limits = c.lim_lo != nullptr;
    r.hist_bins = conf.hist_bins;
    r.seed = conf.seed;
    uint64_t chunk = conf.chunk;
    if (chunk == 0) {
        chunk = kDefaultSampleChunk;
        while (chunk > kBlock && chunk * std::max<uint64_t>(sys->counts.n_vars, 1) * sizeof(double) > kChunkValueBytes) chunk /= 2;
    }
    chunk = (chunk + kBlock - 1) / kBlock * kBlock;
    r.chunk = std::min<uint64_t>(chunk, whole_blocks(c.samples));
    return EZPZ_OK;
}

uint32_t stride_grid(uint64_t items, const EzpzSystem* sys) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, (uint64_t)sys->lim.cus * 16));
}

// Where a caller wants every sample's values: run()'s params [samples][n_param], m and flags [samples][n_meas] and ok [samples];
// run_sobol()'s m and flags [samples][k + 2][n_meas] and ok [samples][k + 2] (no params).
struct Keep {
    double* params;
    double* m;
    uint8_t* flags;
    uint8_t* ok;
    bool host;  // the pointers are host memory: a round waits for its launches and copies out
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

// The outputs of a run with effects (device pointers in run(); edges: host memory) and its checked bins; sums == NULL: the plain run.
struct Effects {
    const double* edges = nullptr;
    double* sums = nullptr;
    uint64_t* counts = nullptr;
    double *cond_mean = nullptr, *cond_var = nullptr, *eta2 = nullptr, *first = nullptr;
    uint32_t* bins_used = nullptr;
    uint32_t bins = 0;
};

// The argument errors the effects add to a run's; the outputs are only compared with NULL, the edges are read.
int check_effects(size_t n_param, size_t n_meas, uint64_t samples, const EzpzMcEffectConfig* ec, Effects& e) {
    EzpzMcEffectConfig conf;
    mce::default_config(&conf);
    if (ec) conf = *ec;
    if (int rc = mce::check_shape(n_param, n_meas, conf.bins)) return rc;
    if (samples && (!e.edges || !e.sums || !e.counts || !e.cond_mean || !e.cond_var || !e.eta2 || !e.first || !e.bins_used))
        return EZPZ_ERR_INVALID_ARGUMENT;
    if (e.edges)
        if (int rc = mce::check_edges(e.edges, n_param, conf.bins)) return rc;
    e.bins = conf.bins;
    return EZPZ_OK;
}

// The quantiles of a run (probs: host memory; out: a device pointer in run()) and the checked z; n_q == 0: the plain run.
struct Quant {
    const double* probs = nullptr;
    size_t n_q = 0;
    EzpzMcQuantile* out = nullptr;
    double z = 0.0;
};

// The outputs of a run with factorial effects (device pointers in run()) and the number of CORNER dimensions; info == NULL: the plain run.
struct Fact {
    mcf::FactorialOut out;
    uint32_t kc = 0;
};

// The argument errors the factorial effects add to a run's; the outputs are only compared with NULL.
int check_factorial(const Call& c, const Request& r, Fact& f) {
    if (c.n_meas == 0 || c.n_meas > mcf::kMaxMeas) return EZPZ_ERR_INVALID_ARGUMENT;
    f.kc = 0;
    for (const mc::Dist& d : r.dists) {
        if (d.kind != EZPZ_MC_CORNER && d.kind != EZPZ_MC_FIXED) return EZPZ_ERR_INVALID_ARGUMENT;
        if (d.kind == EZPZ_MC_CORNER) ++f.kc;
    }
    if (f.kc == 0 || f.kc > mcf::kMaxCorners) return EZPZ_ERR_INVALID_ARGUMENT;
    if (c.samples && c.samples != 1ull << f.kc) return EZPZ_ERR_INVALID_ARGUMENT;
    const mcf::FactorialOut& o = f.out;
    if (c.samples && (!o.info || !o.main || !o.pair || !o.ss_order || !o.ss_total || !o.first || !o.total)) return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

// The outputs of a run with Sobol indices (device pointers in run_sobol) and its checked configuration.
struct SobolOut {
    double* sums = nullptr;
    uint64_t* n_complete = nullptr;
    double *var = nullptr, *first = nullptr, *total = nullptr, *first_var = nullptr, *total_var = nullptr;
    uint64_t seed_b = 0;
    uint32_t fixed_mask = 0;
};

// The argument errors the indices add to a run's, and the run's chunk; the pointers are only compared with NULL.
int check_sobol(const Call& c, const EzpzSobolConfig* sc, Request& r, SobolOut& o) {
    const size_t n_param = c.n_param, n_meas = c.n_meas;
    if (int rc = sobol::check_shape(n_param, n_meas)) return rc;
    EzpzSobolConfig s;
    sobol::default_config(&s);
    if (sc) s = *sc;
    if (s.seed_b == r.seed) return EZPZ_ERR_INVALID_ARGUMENT;
    o.seed_b = s.seed_b;
    o.fixed_mask = 0;
    for (size_t j = 0; j < n_param; ++j) {
        if (r.dists[j].kind == EZPZ_MC_CORNER) return EZPZ_ERR_INVALID_ARGUMENT;
        // (a flagged dimension's matrix B would be matrix A XOR a constant: the two are not independent, and pick-freeze needs that)
        if (r.dists[j].sequence) return EZPZ_ERR_INVALID_ARGUMENT;
        if (r.dists[j].kind == EZPZ_MC_FIXED) o.fixed_mask |= 1u << j;
    }
    if (c.samples && (!o.sums || !o.n_complete || !o.var || (n_param && (!o.first || !o.total || !o.first_var || !o.total_var))))
        return EZPZ_ERR_INVALID_ARGUMENT;
    if (!(c.mc_cfg && c.mc_cfg->chunk)) {  // the library's choice: the rows and the copies of x0 each below the round's bound
        const uint64_t per_sample = std::max<uint64_t>({(uint64_t)c.sys->counts.n_vars, (uint64_t)(n_param + 2) * n_meas, 1}) * sizeof(double);
        const uint64_t chunk = std::max<uint64_t>(std::min<uint64_t>(kChunkValueBytes / per_sample, kDefaultSampleChunk) / kBlock * kBlock, kBlock);
        r.chunk = std::min<uint64_t>(chunk, whole_blocks(c.samples));
    }
    return EZPZ_OK;
}

// What every entry does before its run, in the order the argument errors take precedence: the run's checks, the kind's own
// (`extra`), nothing to do for no samples -- up to here no output and nothing of the plan is touched -- then `body` on the plan
// with its mutex held and the system's device current.
template <class Extra, class Body>
int enter(const Call& c, Extra&& extra, Body&& body) {
    Request r;
    if (int rc = check_run(c, r)) return rc;
    if (int rc = extra(r)) return rc;
    if (c.samples == 0) return EZPZ_OK;
    McPlan& P = plan_of(c.sys);
    std::lock_guard<std::mutex> lock(P.mu);
    EZPZ_ON_DEVICE(c.sys->device);
    return body(P, r);
}

// What a run needs of the plan's device buffers (the tables and the host forms' buffers apart).  visit() is the one list of them.
struct Needs {
    uint64_t chunk, samples;
    size_t n_vars, n_param, n_meas;
    size_t rows;   // 1: run()'s m, flags and ok; k + 2: run_sobol()'s rows and sums
    bool contrib;  // the moments' workspace
    size_t n_q;    // != 0: the selection's workspace, and of every sample's m, flags and ok the stores the plan has to hold itself
    bool own_m, own_flags, own_ok;  // (false: a caller's device keep-buffer stands in)
    uint32_t effect_bins = 0;       // != 0: the cells' workspace
    uint32_t fact_kc = 0;           // != 0: the transform's workspace, and the stores of every sample's m, flags and ok as for n_q

    // Every buffer with the count it has to hold.  grow == false: does any of them have to grow (1) or none (0); grow == true:
    // grow them (EZPZ_OK or the error).  A buffer cannot be in one answer and missing from the other.
    int visit(McPlan& P, bool grow) const {
        const uint64_t blocks = chunk / kBlock;
        const uint32_t k = (uint32_t)n_param, m = (uint32_t)n_meas;
        int rc = EZPZ_OK;
        auto buf = [&](auto& b, uint64_t count) {
            if (rc == EZPZ_OK) rc = grow ? b.ensure(count) : (int)(count > b.cap);
        };
        auto work = [&](auto& w, auto... dims) {
            if (rc == EZPZ_OK) rc = grow ? w.ensure(dims...) : (int)w.grows(dims...);
        };
        buf(P.x_in, chunk * n_vars), buf(P.x_out, chunk * n_vars), buf(P.params, chunk * n_param), buf(P.status, chunk);
        buf(P.nominal, n_meas);
        buf(P.part_f, blocks * n_meas * 4), buf(P.part_arg, blocks * n_meas * 2), buf(P.part_n, blocks * (2 * n_meas + 2));
        if (rows == 1) {
            buf(P.m, chunk * n_meas), buf(P.flags, chunk * n_meas), buf(P.ok, chunk);
        } else {
            buf(P.rows_f, rows * chunk * n_meas), buf(P.rows_flags, rows * chunk * n_meas), buf(P.rows_ok, rows * chunk);
            work(P.sobol_work, blocks, k, m);
        }
        if (contrib) work(P.moment_work, blocks, k + m);
        if (n_q || fact_kc) {
            if (own_m) buf(P.all_m, samples * n_meas);
            if (own_flags) buf(P.all_flags, samples * n_meas);
            if (own_ok) buf(P.all_ok, samples);
        }
        if (n_q) work(P.select_work, m, (uint32_t)n_q);
        if (fact_kc) work(P.factorial_work, m, fact_kc);
        if (effect_bins) work(P.effect_work, blocks, k * effect_bins * m);
        return rc;
    }
};

// What the host writes before a run's launches, behind the last run's, and the nominal: nominal[i] = m(record i, x0), 0 where
// the guard fires.  `c` holds device pointers.
int prepare(McPlan& P, const Request& r, const Call& c, const Needs& need) {
    release_thread_kernel(c.sys->device);
    const size_t dist_bytes = r.dists.size() * sizeof(mc::Dist), tab_bytes = r.tab.size() * sizeof(double);
    int rc;
    std::vector<unsigned char> tables(dist_bytes + tab_bytes);
    if (dist_bytes) std::memcpy(tables.data(), r.dists.data(), dist_bytes);
    if (tab_bytes) std::memcpy(tables.data() + dist_bytes, r.tab.data(), tab_bytes);
    if (tables != P.tables_kept || !P.ticket.p || need.visit(P, false)) {
        if ((rc = P.order.before_overwrite()) != EZPZ_OK) return rc;
        P.tables_kept.clear();
        if ((rc = P.dist.ensure(r.dists.size())) != EZPZ_OK || (rc = P.tab.ensure(r.tab.size())) != EZPZ_OK) return rc;
        if (dist_bytes) HIP_TRY(hipMemcpy(P.dist.p, r.dists.data(), dist_bytes, hipMemcpyHostToDevice));
        if (tab_bytes) HIP_TRY(hipMemcpy(P.tab.p, r.tab.data(), tab_bytes, hipMemcpyHostToDevice));
        if ((rc = need.visit(P, true)) != EZPZ_OK) return rc;
        if (!P.ticket.p) {
            if ((rc = P.ticket.ensure(1)) != EZPZ_OK) return rc;
            HIP_TRY(hipMemset(P.ticket.p, 0, P.ticket.cap * sizeof(unsigned int)));
        }
        P.tables_kept = std::move(tables);
        call_stamp(MC_TABLES_UPLOADED);
    }
    if ((rc = P.order.order_behind(c.stream)) != EZPZ_OK) return rc;
    // (run() measures where there are records; run_sobol() always does: check_sobol has seen to n_meas >= 1)
    if (need.n_meas || need.rows != 1)
        return ezpz_system_measure_device(c.sys, c.records, need.n_meas, c.x0, 1, P.nominal.p, nullptr, nullptr, c.stream);
    return EZPZ_OK;
}

// The reduction of the rows m, flags [chunk][n_meas] and ok [chunk] into the statistics, on the plan's partial sums.
mc::ReduceArgs reduce_args(const McPlan& P, const Needs& need, const double* m, const uint8_t* flags, uint8_t* ok, bool limits, uint32_t hist_bins,
                           EzpzMcStats* stats, EzpzMcTotals* totals, uint64_t* hist) {
    const size_t n_meas = need.n_meas, per_part = need.chunk / kBlock * n_meas;
    mc::ReduceArgs a{};
    a.m = m;
    a.flags = flags;
    a.status = P.status.p;
    a.nominal = P.nominal.p;
    a.lim_lo = limits ? P.tab.p : nullptr;
    a.lim_hi = limits ? P.tab.p + n_meas : nullptr;
    a.hist_lo = P.tab.p + 2 * n_meas;
    a.hist_scale = P.tab.p + 3 * n_meas;
    a.samples = need.samples;
    a.n_meas = (uint32_t)n_meas;
    a.hist_bins = n_meas ? hist_bins : 0;
    a.part_d = P.part_f.p;
    a.part_d2 = a.part_d + per_part;
    a.part_min = a.part_d2 + per_part;
    a.part_max = a.part_min + per_part;
    a.part_argmin = P.part_arg.p;
    a.part_argmax = a.part_argmin + per_part;
    a.part_valid = P.part_n.p;
    a.part_in = a.part_valid + per_part;
    a.part_ok = a.part_in + per_part;
    a.part_all_in = a.part_ok + need.chunk / kBlock;
    a.ticket = P.ticket.p;
    a.ok = ok;
    a.stats = stats;
    a.totals = totals;
    a.hist = hist;
    return a;
}

int enqueue_reduce(mc::ReduceArgs& a, uint64_t first, uint64_t count, hipStream_t stream) {
    a.first = first;
    a.count = count;
    a.first_round = first == 0;
    hipLaunchKernelGGL(mc::mc_reduce_kernel, dim3((uint32_t)((count + kBlock - 1) / kBlock)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

// run_sobol()'s draw: matrix B's seed and which columns come from it (mc::kPickNone, mc::kPickAll or the column j)
struct Pick {
    uint64_t seed_b;
    uint32_t which;
};

// The sampler of a list with flagged dimensions: the walk, its table in LDS.  EZPZ_MC_SEQUENCE_KERNEL=const: the walk on constant
// memory; =direct: every point evaluated directly (A/B runs; the same bytes from all three).
void launch_sequence_sampler(const McPlan& P, const Request& r, const Call& c, uint64_t first, uint64_t count) {
    static const int variant = [] {
        const char* e = std::getenv("EZPZ_MC_SEQUENCE_KERNEL");
        return !e ? 0 : !std::strcmp(e, "const") ? 1 : !std::strcmp(e, "direct") ? 2 : 0;
    }();
    const uint32_t n_param = (uint32_t)r.dists.size();
    const uint64_t runs = (count + mc::kWalkRun - 1) / mc::kWalkRun;
    if (variant == 2)
        hipLaunchKernelGGL(mc::mc_sample_direct_kernel, dim3(stride_grid(count * n_param, c.sys)), dim3(256), 0, c.stream, P.dist.p, r.seed, first, count, n_param, P.params.p);
    else if (variant == 1)
        hipLaunchKernelGGL(mc::mc_sample_walk_kernel<false>, dim3(stride_grid(runs * n_param, c.sys)), dim3(256), 0, c.stream, P.dist.p, r.seed, first, count, n_param, P.params.p);
    else
        hipLaunchKernelGGL(mc::mc_sample_walk_kernel<true>, dim3(stride_grid(runs * n_param, c.sys)), dim3(256), 0, c.stream, P.dist.p, r.seed, first, count, n_param, P.params.p);
}

// Samples [first, first + count) drawn -- run()'s sampler for pick == NULL -- solved from copies of x0 and measured into m and flags.
int sub_round(McPlan& P, const Request& r, const Call& c, const Pick* pick, uint64_t first, uint64_t count, double* m, uint8_t* flags) {
    EzpzSystem* sys = c.sys;
    const size_t n = sys->counts.n_vars, n_param = r.dists.size(), n_meas = r.words.size() / kMeasureRecWords;
    int rc;
    if (n_param && pick)
        hipLaunchKernelGGL(mc::mc_sample_pick_kernel, dim3(stride_grid(count * n_param, sys)), dim3(256), 0, c.stream, P.dist.p, r.seed, pick->seed_b, pick->which, first, count, (uint32_t)n_param, P.params.p);
    else if (n_param && r.sequence)
        launch_sequence_sampler(P, r, c, first, count);
    else if (n_param)
        hipLaunchKernelGGL(mc::mc_sample_kernel, dim3(stride_grid(count * n_param, sys)), dim3(256), 0, c.stream, P.dist.p, r.seed, first, count, (uint32_t)n_param, P.params.p);
    if (n) hipLaunchKernelGGL(mc::mc_broadcast_kernel, dim3(stride_grid(count * n, sys)), dim3(256), 0, c.stream, c.x0, (uint32_t)n, count, P.x_in.p);
    HIP_TRY(hipGetLastError());
    if ((rc = ezpz_system_solve_batch_params_device(sys, P.x_in.p, c.positions, n_param, P.params.p, count, c.cfg, P.x_out.p, P.status.p, nullptr,
                                                    nullptr, 0, c.stream)) != EZPZ_OK)
        return rc;
    return n_meas ? ezpz_system_measure_device(sys, c.records, n_meas, P.x_out.p, count, m, flags, nullptr, c.stream) : EZPZ_OK;
}

int copy_out(void* dst, const void* src, size_t bytes, bool host, hipStream_t stream) {
    if (!dst || !bytes) return EZPZ_OK;
    if (host)
        HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    else
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
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

// The edges of a run with effects where its kernels read them: others than the buffer holds wait for the last run's launches first.
int upload_effect_edges(McPlan& P, const Call& c, const Effects& eff) {
    const size_t count = c.n_param * (eff.bins - 1);
    if (P.effect_edges.p && P.effect_edges_kept.size() == count && std::equal(eff.edges, eff.edges + count, P.effect_edges_kept.begin(),
                                                                               [](double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }))
        return EZPZ_OK;
    release_thread_kernel(c.sys->device);
    int rc;
    if ((rc = P.order.before_overwrite()) != EZPZ_OK) return rc;
    P.effect_edges_kept.clear();
    if ((rc = P.effect_edges.ensure(count)) != EZPZ_OK) return rc;
    HIP_TRY(hipMemcpy(P.effect_edges.p, eff.edges, count * sizeof(double), hipMemcpyHostToDevice));
    P.effect_edges_kept.assign(eff.edges, eff.edges + count);
    call_stamp(MC_TABLES_UPLOADED);
    return EZPZ_OK;
}

// The plain run, with contributors, with quantiles, with effects or with factorial effects.  Device pointers throughout (but Keep's, see there): the plan's mutex is
// held, the system's device current, the request checked and samples > 0.
int run(McPlan& P, const Request& r, const Call& c, const Keep& keep, const Contrib& contrib, const Quant& quant, const Effects& eff,
        const Fact& fact = Fact{}) {
    const size_t n_param = r.dists.size(), n_meas = r.words.size() / kMeasureRecWords;
    const uint64_t samples = c.samples, chunk = r.chunk;
    const hipStream_t stream = c.stream;
    int rc;
    // the rows the selection or the transform reads: the caller's device buffers where given, else the plan's
    const bool select = quant.n_q != 0, transform = fact.out.info != nullptr, rows_kept = select || transform;
    double* all_m = !keep.host && keep.m ? keep.m : nullptr;
    uint8_t* all_flags = !keep.host && keep.flags ? keep.flags : nullptr;
    uint8_t* all_ok = !keep.host && keep.ok ? keep.ok : nullptr;
    const Needs need{chunk, samples, c.sys->counts.n_vars, n_param, n_meas, 1, contrib.moments != nullptr, quant.n_q, !all_m, !all_flags, !all_ok,
                     eff.sums ? eff.bins : 0u, transform ? fact.kc : 0u};
    if (eff.sums && (rc = upload_effect_edges(P, c, eff)) != EZPZ_OK) return rc;
    if ((rc = prepare(P, r, c, need)) != EZPZ_OK) return rc;
    if (r.hist_bins && n_meas) HIP_TRY(hipMemsetAsync(c.hist, 0, n_meas * (r.hist_bins + 2) * sizeof(uint64_t), stream));
    mc::ReduceArgs a = reduce_args(P, need, P.m.p, P.flags.p, P.ok.p, r.limits, r.hist_bins, c.stats, c.totals, c.hist);
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
    mce::EffectArgs ef{};
    ef.params = P.params.p;
    ef.m = P.m.p;
    ef.flags = P.flags.p;
    ef.ok = P.ok.p;
    ef.nominal_m = P.nominal.p;
    ef.edges = P.effect_edges.p;
    ef.k = (uint32_t)n_param, ef.n_meas = (uint32_t)n_meas, ef.bins = eff.bins;
    ef.sums = eff.sums;
    ef.counts = eff.counts;
    for (uint64_t first = 0; first < samples; first += chunk) {
        const uint64_t count = std::min<uint64_t>(chunk, samples - first);
        if ((rc = sub_round(P, r, c, nullptr, first, count, P.m.p, P.flags.p)) != EZPZ_OK || (rc = enqueue_reduce(a, first, count, stream)) != EZPZ_OK)
            return rc;
        if (contrib.moments) {
            mo.first = first;
            mo.count = count;
            mo.first_round = first == 0;
            if ((rc = mcm::enqueue_moments(P.moment_work, mo, stream)) != EZPZ_OK) return rc;
        }
        if (eff.sums) {
            ef.count = count;
            ef.first_round = first == 0;
            if ((rc = mce::enqueue_effects(P.effect_work, ef, stream)) != EZPZ_OK) return rc;
        }
        if (rows_kept) {  // (a caller's device buffer is filled by the copies below)
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
        mcm::ContribArgs ca{};
        ca.moments = contrib.moments;
        ca.info = contrib.info;
        ca.k = (uint32_t)n_param;
        ca.m = (uint32_t)n_meas;
        ca.pivot_rel = contrib.pivot_rel;
        ca.cov = contrib.cov, ca.beta = contrib.beta, ca.contrib = contrib.contrib, ca.r2 = contrib.r2, ca.dropped = contrib.dropped;
        if ((rc = mcm::enqueue_contributors(ca, stream)) != EZPZ_OK) return rc;
    }
    if (eff.sums) {
        mce::CloseArgs cl{};
        cl.sums = eff.sums;
        cl.counts = eff.counts;
        cl.nominal_m = P.nominal.p;
        cl.k = (uint32_t)n_param, cl.m = (uint32_t)n_meas, cl.bins = eff.bins;
        cl.cond_mean = eff.cond_mean, cl.cond_var = eff.cond_var, cl.eta2 = eff.eta2, cl.first = eff.first, cl.bins_used = eff.bins_used;
        if ((rc = mce::enqueue_close(cl, stream)) != EZPZ_OK) return rc;
    }
    if (select && (rc = mcq::enqueue_select(P.select_work, all_m ? all_m : P.all_m.p, all_flags ? all_flags : P.all_flags.p,
                                            all_ok ? all_ok : P.all_ok.p, samples, (uint32_t)n_meas, quant.probs, (uint32_t)quant.n_q, quant.z,
                                            quant.out, c.sys->lim.cus, stream)) != EZPZ_OK)
        return rc;
    if (transform && (rc = mcf::enqueue_factorial(P.factorial_work, all_m ? all_m : P.all_m.p, all_flags ? all_flags : P.all_flags.p,
                                                  all_ok ? all_ok : P.all_ok.p, P.nominal.p, fact.kc, (uint32_t)n_meas, fact.out, c.sys->lim.cus,
                                                  stream)) != EZPZ_OK)
        return rc;
    call_stamp(MC_LAUNCHED);
    return P.order.record(stream);
}

// The run with Sobol indices, on the same plan, kernels and entries as run(): a round is k' + 2 sub-rounds into the round's rows,
// with the reduction behind A's, the ok bytes behind every other one, mc_sobol.hip's sums behind the last one and its closing kernel
// behind the last round.  Device pointers throughout (but Keep's): the plan's mutex is held, the system's device current, the
// request checked and samples > 0.
int run_sobol(McPlan& P, const Request& r, const Call& c, const SobolOut& out, const Keep& keep) {
    const size_t n_param = r.dists.size(), n_meas = r.words.size() / kMeasureRecWords, R = n_param + 2;
    const uint64_t samples = c.samples, chunk = r.chunk;
    const hipStream_t stream = c.stream;
    int rc;
    const Needs need{chunk, samples, c.sys->counts.n_vars, n_param, n_meas, R, false, 0, false, false, false};
    if ((rc = prepare(P, r, c, need)) != EZPZ_OK) return rc;
    // A's rows through the plain run's reduction: no limits, no histogram
    mc::ReduceArgs a = reduce_args(P, need, P.rows_f.p, P.rows_flags.p, P.rows_ok.p, false, 0, c.stats, c.totals, nullptr);
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
            const Pick pick{out.seed_b, row == 0 ? mc::kPickNone : row == 1 ? mc::kPickAll : (uint32_t)(row - 2)};
            if ((rc = sub_round(P, r, c, &pick, first, count, P.rows_f.p + row * chunk * n_meas, P.rows_flags.p + row * chunk * n_meas)) != EZPZ_OK)
                return rc;
            if ((rc = row == 0 ? enqueue_reduce(a, first, count, stream) : sobol::enqueue_ok(P.status.p, count, P.rows_ok.p + row * chunk, stream)) != EZPZ_OK)
                return rc;
        }
        su.count = count;
        su.first_round = first == 0;
        if ((rc = sobol::enqueue_sums(P.sobol_work, su, stream)) != EZPZ_OK) return rc;
        if (keep.m || keep.flags || keep.ok) {
            if (keep.host) HIP_TRY(hipStreamSynchronize(stream));
            for (size_t row = 0; row < R; ++row) {
                const size_t src = row >= 2 && ((out.fixed_mask >> (row - 2)) & 1u) ? 0 : row;  // (a FIXED j: a copy of row 0)
                if ((rc = copy_rows(keep.m ? keep.m + (first * R + row) * n_meas : nullptr, R * n_meas * sizeof(double), P.rows_f.p + src * chunk * n_meas,
                                    n_meas * sizeof(double), n_meas * sizeof(double), count, keep.host, stream)) != EZPZ_OK ||
                    (rc = copy_rows(keep.flags ? keep.flags + (first * R + row) * n_meas : nullptr, R * n_meas, P.rows_flags.p + src * chunk * n_meas,
                                    n_meas, n_meas, count, keep.host, stream)) != EZPZ_OK ||
                    (rc = copy_rows(keep.ok ? keep.ok + first * R + row : nullptr, R, P.rows_ok.p + src * chunk, 1, 1, count, keep.host, stream)) != EZPZ_OK)
                    return rc;
            }
        }
    }
    sobol::CloseArgs cl{};
    cl.sums = out.sums;
    cl.n_complete = out.n_complete;
    cl.k = (uint32_t)n_param, cl.m = (uint32_t)n_meas;
    cl.var = out.var, cl.first = out.first, cl.total = out.total, cl.first_var = out.first_var, cl.total_var = out.total_var;
    if ((rc = sobol::enqueue_close(cl, stream)) != EZPZ_OK) return rc;
    call_stamp(MC_LAUNCHED);
    return P.order.record(stream);
}

// A host form's outputs.  add() gives each a place, in order, in one device buffer; reserve() makes the buffer hold them and hands
// out the places; copy_back() brings every output home.  An entry of no elements takes no room and is not copied.
struct Staged {
    struct Entry {
        void* host;
        size_t count, size;
        void* dev;                        // the caller's device pointer for this entry: a T**
        void (*set)(void*, unsigned char*);  // ... and how to set it
        size_t offset;
    };
    std::vector<Entry> entries;

    template <class T>
    void add(T* host, size_t count, T*& dev) {
        entries.push_back(Entry{host, count, sizeof(T), &dev, [](void* slot, unsigned char* p) { *static_cast<T**>(slot) = reinterpret_cast<T*>(p); }, 0});
    }
    int reserve(DevBuf<unsigned char>& buf) {
        size_t bytes = 0;
        for (Entry& e : entries) {
            e.offset = bytes;
            bytes += (e.count * e.size + 255) / 256 * 256;  // (every place as aligned as an allocation of its own)
        }
        // (the buffer of an earlier host call is idle: it waited for its launches)
        if (int rc = buf.ensure(bytes)) return rc;
        for (Entry& e : entries) e.set(e.dev, buf.p + e.offset);
        return EZPZ_OK;
    }
    int copy_back(const DevBuf<unsigned char>& buf) const {
        for (const Entry& e : entries)
            if (e.count) HIP_TRY(hipMemcpy(e.host, buf.p + e.offset, e.count * e.size, hipMemcpyDeviceToHost));
        return EZPZ_OK;
    }
};

// A host form between its entry and its run: `c`'s x0 on the device, its stats and totals staged behind whatever `out` already
// holds; `run_on(d)` runs on the device pointers; the copies back once the stream has drained.
template <class Run>
int host_form(McPlan& P, const Call& c, Staged& out, Run&& run_on) {
    const size_t n = c.sys->counts.n_vars;
    Call d = c;
    out.add(c.stats, c.n_meas, d.stats);
    out.add(c.totals, 1, d.totals);
    int rc;
    if ((rc = P.x0_in.ensure(n)) != EZPZ_OK || (rc = out.reserve(P.host_out)) != EZPZ_OK) return rc;
    if (n) HIP_TRY(hipMemcpy(P.x0_in.p, c.x0, n * sizeof(double), hipMemcpyHostToDevice));
    d.x0 = P.x0_in.p;
    if ((rc = run_on(d)) != EZPZ_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c.stream));
    return out.copy_back(P.host_out);
}

// ---- the entries: plain, with contributors, with quantiles, with effects ----------------------------------------------------------
int check_kinds(const Call& c, const EzpzMcContribConfig* cc, Contrib* contrib, const EzpzMcQuantileConfig* qc, Quant* quant,
                const EzpzMcEffectConfig* ec = nullptr, Effects* effects = nullptr) {
    if (effects)
        if (int rc = check_effects(c.n_param, c.n_meas, c.samples, ec, *effects)) return rc;
    if (contrib)
        if (int rc = check_contrib(c.n_param, c.n_meas, c.samples, cc, *contrib)) return rc;
    if (quant)
        if (int rc = mcq::check(c.samples, c.n_meas, quant->probs, quant->n_q, qc, c.sys, quant->out, quant->z)) return rc;  // (the rows are the run's own)
    return EZPZ_OK;
}

int run_device(const Call& c, const Keep& keep, const EzpzMcContribConfig* cc, Contrib* contrib, const EzpzMcQuantileConfig* qc, Quant* quant,
               const EzpzMcEffectConfig* ec = nullptr, Effects* effects = nullptr) {
    return enter(c, [&](Request&) { return check_kinds(c, cc, contrib, qc, quant, ec, effects); }, [&](McPlan& P, Request& r) {
        return run(P, r, c, keep, contrib ? *contrib : Contrib{}, quant ? *quant : Quant{}, effects ? *effects : Effects{});
    });
}

// `contrib`, `quant` and `effects` hold host pointers here.
int run_host(const Call& c, const Keep& keep, const EzpzMcContribConfig* cc, Contrib* contrib, const EzpzMcQuantileConfig* qc, Quant* quant,
             const EzpzMcEffectConfig* ec = nullptr, Effects* effects = nullptr) {
    return enter(c, [&](Request&) { return check_kinds(c, cc, contrib, qc, quant, ec, effects); }, [&](McPlan& P, Request& r) {
        const size_t n_param = c.n_param, n_meas = c.n_meas, K = n_param + n_meas, km = n_param * n_meas;
        Staged out;
        uint64_t* hist_dev = nullptr;
        out.add(c.hist, n_meas * (r.hist_bins ? r.hist_bins + 2 : 0), hist_dev);
        Contrib dev;
        if (contrib) {
            dev.pivot_rel = contrib->pivot_rel;
            out.add(contrib->moments, mcm::entries_of((uint32_t)K), dev.moments);
            out.add(contrib->cov, K * K, dev.cov);
            out.add(contrib->beta, km, dev.beta);
            out.add(contrib->contrib, km, dev.contrib);
            out.add(contrib->r2, n_meas, dev.r2);
            out.add(contrib->info, 1, dev.info);
            out.add(contrib->dropped, 1, dev.dropped);
        }
        Quant qdev;
        if (quant && quant->n_q) {
            qdev = *quant;
            out.add(quant->out, n_meas * quant->n_q, qdev.out);
        }
        Effects edev;
        if (effects) {
            edev = *effects;  // (the edges stay the caller's host array; bins as checked)
            const size_t cells = n_param * effects->bins * n_meas;
            out.add(effects->sums, 2 * cells, edev.sums);
            out.add(effects->counts, cells, edev.counts);
            out.add(effects->cond_mean, cells, edev.cond_mean);
            out.add(effects->cond_var, cells, edev.cond_var);
            out.add(effects->eta2, km, edev.eta2);
            out.add(effects->first, km, edev.first);
            out.add(effects->bins_used, km, edev.bins_used);
        }
        return host_form(P, c, out, [&](Call& d) {
            d.hist = hist_dev;
            return run(P, r, d, keep, dev, qdev, edev);
        });
    });
}

// ---- the entries: factorial effects ------------------------------------------------------------------------------------------------
int factorial_device(const Call& c, const Keep& keep, Fact& fact) {
    return enter(c, [&](Request& r) { return check_factorial(c, r, fact); },
                 [&](McPlan& P, Request& r) { return run(P, r, c, keep, Contrib{}, Quant{}, Effects{}, fact); });
}

// `fact` holds host pointers here.
int factorial_host(const Call& c, const Keep& keep, Fact& fact) {
    return enter(c, [&](Request& r) { return check_factorial(c, r, fact); }, [&](McPlan& P, Request& r) {
        const size_t n_meas = c.n_meas, kc = fact.kc, N = (size_t)1 << kc;
        Staged out;
        uint64_t* hist_dev = nullptr;
        out.add(c.hist, n_meas * (r.hist_bins ? r.hist_bins + 2 : 0), hist_dev);
        Fact dev;
        dev.kc = fact.kc;
        out.add(fact.out.info, n_meas, dev.out.info);
        out.add(fact.out.main, n_meas * kc, dev.out.main);
        out.add(fact.out.pair, n_meas * kc * kc, dev.out.pair);
        out.add(fact.out.ss_order, n_meas * (kc + 1), dev.out.ss_order);
        out.add(fact.out.ss_total, n_meas * kc, dev.out.ss_total);
        out.add(fact.out.first, n_meas * kc, dev.out.first);
        out.add(fact.out.total, n_meas * kc, dev.out.total);
        if (fact.out.coef) out.add(fact.out.coef, n_meas * N, dev.out.coef);
        return host_form(P, c, out, [&](Call& d) {
            d.hist = hist_dev;
            return run(P, r, d, keep, Contrib{}, Quant{}, Effects{}, dev);
        });
    });
}

// ---- the entries: Sobol indices ----------------------------------------------------------------------------------------------------
int sobol_device(const Call& c, const EzpzSobolConfig* sc, SobolOut& out, const Keep& keep) {
    return enter(c, [&](Request& r) { return check_sobol(c, sc, r, out); }, [&](McPlan& P, Request& r) { return run_sobol(P, r, c, out, keep); });
}

// `out` holds host pointers here.
int sobol_host(const Call& c, const EzpzSobolConfig* sc, SobolOut& out, const Keep& keep) {
    return enter(c, [&](Request& r) { return check_sobol(c, sc, r, out); }, [&](McPlan& P, Request& r) {
        const size_t n_meas = c.n_meas, km = c.n_param * n_meas;
        Staged staged;
        SobolOut dev = out;
        staged.add(out.sums, n_meas * sobol::width_of((uint32_t)c.n_param), dev.sums);
        staged.add(out.n_complete, n_meas, dev.n_complete);
        staged.add(out.var, n_meas, dev.var);
        staged.add(out.first, km, dev.first);
        staged.add(out.total, km, dev.total);
        staged.add(out.first_var, km, dev.first_var);
        staged.add(out.total_var, km, dev.total_var);
        return host_form(P, c, staged, [&](Call& d) { return run_sobol(P, r, d, dev, keep); });
    });
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
    return mc::sample_host(seed, dist, nominal, n_param, first, count, params_out);
}

int ezpz_system_tolerance_mc_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                    const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo,
                                    const double* lim_hi, const double* hist_lo, const double* hist_hi, uint64_t samples,
                                    const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev,
                                    uint64_t* hist_dev, double* keep_params_dev, double* keep_m_dev, uint8_t* keep_flags_dev,
                                    uint8_t* keep_ok_dev, void* stream) {
    const Call c{sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats_dev, totals_dev, hist_dev, (hipStream_t)stream};
    return run_device(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, nullptr, nullptr, nullptr, nullptr);
}

int ezpz_system_tolerance_mc(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                             const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo, const double* lim_hi,
                             const double* hist_lo, const double* hist_hi, uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg,
                             EzpzMcStats* stats, EzpzMcTotals* totals, uint64_t* hist, double* keep_params, double* keep_m,
                             uint8_t* keep_flags, uint8_t* keep_ok) {
    const Call c{sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats, totals, hist, hipStreamPerThread};
    return run_host(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, nullptr, nullptr, nullptr, nullptr);
}

int ezpz_system_tolerance_mc_contrib_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                            const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                            const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                            uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats_dev,
                                            EzpzMcTotals* totals_dev, uint64_t* hist_dev, double* keep_params_dev, double* keep_m_dev,
                                            uint8_t* keep_flags_dev, uint8_t* keep_ok_dev, const EzpzMcContribConfig* cc, double* moments_dev,
                                            EzpzMcMomentsInfo* info_dev, double* cov_dev, double* beta_dev, double* contrib_dev,
                                            double* r2_dev, uint64_t* dropped_dev, void* stream) {
    const Call c{sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats_dev, totals_dev, hist_dev, (hipStream_t)stream};
    Contrib o;
    o.moments = moments_dev, o.info = info_dev, o.cov = cov_dev, o.beta = beta_dev, o.contrib = contrib_dev, o.r2 = r2_dev, o.dropped = dropped_dev;
    return run_device(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, cc, &o, nullptr, nullptr);
}

int ezpz_system_tolerance_mc_contrib(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                     const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo,
                                     const double* lim_hi, const double* hist_lo, const double* hist_hi, uint64_t samples,
                                     const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats, EzpzMcTotals* totals,
                                     uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags, uint8_t* keep_ok,
                                     const EzpzMcContribConfig* cc, double* moments, EzpzMcMomentsInfo* info, double* cov, double* beta,
                                     double* contrib, double* r2, uint64_t* dropped) {
    const Call c{sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats, totals, hist, hipStreamPerThread};
    Contrib o;
    o.moments = moments, o.info = info, o.cov = cov, o.beta = beta, o.contrib = contrib, o.r2 = r2, o.dropped = dropped;
    return run_host(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, cc, &o, nullptr, nullptr);
}

int ezpz_system_tolerance_mc_effects_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                            const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                            const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                            uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats_dev,
                                            EzpzMcTotals* totals_dev, uint64_t* hist_dev, double* keep_params_dev, double* keep_m_dev,
                                            uint8_t* keep_flags_dev, uint8_t* keep_ok_dev, const EzpzMcEffectConfig* ec,
                                            const double* edges, double* sums_dev, uint64_t* counts_dev, double* cond_mean_dev,
                                            double* cond_var_dev, double* eta2_dev, double* first_dev, uint32_t* bins_used_dev,
                                            void* stream) {
    const Call c{sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats_dev, totals_dev, hist_dev, (hipStream_t)stream};
    Effects o;
    o.edges = edges, o.sums = sums_dev, o.counts = counts_dev, o.cond_mean = cond_mean_dev, o.cond_var = cond_var_dev;
    o.eta2 = eta2_dev, o.first = first_dev, o.bins_used = bins_used_dev;
    return run_device(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, nullptr, nullptr, nullptr, nullptr, ec, &o);
}

int ezpz_system_tolerance_mc_effects(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                     const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo,
                                     const double* lim_hi, const double* hist_lo, const double* hist_hi, uint64_t samples,
                                     const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats, EzpzMcTotals* totals,
                                     uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags, uint8_t* keep_ok,
                                     const EzpzMcEffectConfig* ec, const double* edges, double* sums, uint64_t* counts,
                                     double* cond_mean, double* cond_var, double* eta2, double* first, uint32_t* bins_used) {
    const Call c{sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats, totals, hist, hipStreamPerThread};
    Effects o;
    o.edges = edges, o.sums = sums, o.counts = counts, o.cond_mean = cond_mean, o.cond_var = cond_var;
    o.eta2 = eta2, o.first = first, o.bins_used = bins_used;
    return run_host(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, nullptr, nullptr, nullptr, nullptr, ec, &o);
}

int ezpz_system_tolerance_mc_quantiles_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                              const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records,
                                              size_t n_meas, const double* lim_lo, const double* lim_hi, const double* hist_lo,
                                              const double* hist_hi, uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg,
                                              EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, uint64_t* hist_dev,
                                              double* keep_params_dev, double* keep_m_dev, uint8_t* keep_flags_dev,
                                              uint8_t* keep_ok_dev, const double* probs, size_t n_q, const EzpzMcQuantileConfig* qc,
                                              EzpzMcQuantile* out_dev, void* stream) {
    const Call c{sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats_dev, totals_dev, hist_dev, (hipStream_t)stream};
    Quant q;
    q.probs = probs, q.n_q = n_q, q.out = out_dev;
    return run_device(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, nullptr, nullptr, qc, &q);
}

int ezpz_system_tolerance_mc_quantiles(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param,
                                       const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                       const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                       uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats,
                                       EzpzMcTotals* totals, uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags,
                                       uint8_t* keep_ok, const double* probs, size_t n_q, const EzpzMcQuantileConfig* qc,
                                       EzpzMcQuantile* out) {
    const Call c{sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats, totals, hist, hipStreamPerThread};
    Quant q;
    q.probs = probs, q.n_q = n_q, q.out = out;
    return run_host(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, nullptr, nullptr, qc, &q);
}

int ezpz_system_tolerance_mc_factorial_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                              const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records,
                                              size_t n_meas, const double* lim_lo, const double* lim_hi, const double* hist_lo,
                                              const double* hist_hi, uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg,
                                              EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, uint64_t* hist_dev,
                                              double* keep_params_dev, double* keep_m_dev, uint8_t* keep_flags_dev,
                                              uint8_t* keep_ok_dev, EzpzMcFactorial* info_dev, double* main_dev, double* pair_dev,
                                              double* ss_order_dev, double* ss_total_dev, double* first_dev, double* total_dev,
                                              double* coef_dev, void* stream) {
    const Call c{sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats_dev, totals_dev, hist_dev, (hipStream_t)stream};
    Fact f;
    f.out.info = info_dev, f.out.main = main_dev, f.out.pair = pair_dev, f.out.ss_order = ss_order_dev, f.out.ss_total = ss_total_dev;
    f.out.first = first_dev, f.out.total = total_dev, f.out.coef = coef_dev;
    return factorial_device(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, f);
}

int ezpz_system_tolerance_mc_factorial(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param,
                                       const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                       const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                       uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats,
                                       EzpzMcTotals* totals, uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags,
                                       uint8_t* keep_ok, EzpzMcFactorial* info, double* main, double* pair, double* ss_order,
                                       double* ss_total, double* first, double* total, double* coef) {
    const Call c{sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats, totals, hist, hipStreamPerThread};
    Fact f;
    f.out.info = info, f.out.main = main, f.out.pair = pair, f.out.ss_order = ss_order, f.out.ss_total = ss_total;
    f.out.first = first, f.out.total = total, f.out.coef = coef;
    return factorial_host(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, f);
}

int ezpz_system_tolerance_sobol_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                       const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                       uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, const EzpzSobolConfig* sc,
                                       EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, double* sums_dev, uint64_t* n_complete_dev,
                                       double* var_dev, double* first_dev, double* total_dev, double* first_var_dev, double* total_var_dev,
                                       double* keep_f_dev, uint8_t* keep_flags_dev, uint8_t* keep_ok_dev, void* stream) {
    const Call c{sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, nullptr, nullptr, nullptr, nullptr, samples, mc_cfg, cfg,
                 stats_dev, totals_dev, nullptr, (hipStream_t)stream};
    SobolOut o;
    o.sums = sums_dev, o.n_complete = n_complete_dev, o.var = var_dev, o.first = first_dev, o.total = total_dev;
    o.first_var = first_var_dev, o.total_var = total_var_dev;
    return sobol_device(c, sc, o, Keep{nullptr, keep_f_dev, keep_flags_dev, keep_ok_dev, false});
}

int ezpz_system_tolerance_sobol(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                const double* nominal, const EzpzConstraint* records, size_t n_meas, uint64_t samples,
                                const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, const EzpzSobolConfig* sc, EzpzMcStats* stats,
                                EzpzMcTotals* totals, double* sums, uint64_t* n_complete, double* var, double* first, double* total,
                                double* first_var, double* total_var, double* keep_f, uint8_t* keep_flags, uint8_t* keep_ok) {
    const Call c{sys, x0, positions, n_param, dist, nominal, records, n_meas, nullptr, nullptr, nullptr, nullptr, samples, mc_cfg, cfg,
                 stats, totals, nullptr, hipStreamPerThread};
    SobolOut o;
    o.sums = sums, o.n_complete = n_complete, o.var = var, o.first = first, o.total = total, o.first_var = first_var, o.total_var = total_var;
    return sobol_host(c, sc, o, Keep{nullptr, keep_f, keep_flags, keep_ok, true});
}

}  // extern "C"
