// Monte-Carlo tolerance analysis (include/ezpz_amd.h: ezpz_mc_sample, ezpz_system_tolerance_mc and its _device form; DESIGN.md
// 3k): the host side of tolerance_mc.hip.hpp's kernels -- the check of a request, the plan a system keeps (the round's workspace,
// the sampler's and the limits' tables, the host forms' buffers) and the rounds.  Every kind of run is one pipeline with a tail of
// its own.  entry() checks the request and takes the plan; prepare() brings the plan's tables and buffers to what the run needs --
// Needs lists every buffer with its count once, and both "does anything grow" and "grow it" are that list -- and measures the
// nominal; sub_round() is sampler -> copies of x0 -> ezpz_system_solve_batch_params_device -> ezpz_system_measure_device, all on
// the caller's stream: the driven solve and the measurement are those entries themselves, with their routes, their locks and their
// ordering.  What a kind adds stands in its tail alone -- Plain, Contrib, Quant, Effects, Fact, Image, SobolOut: its checks, the one list of
// its outputs, its workspaces and what it enqueues -- and the run is a template on the tail that names none of them:
//   run()        one sub-round a round, the reduction behind it, then the tail's behind_round(); the rows kept on the device where
//                the tail reads them; the tail's behind_run() behind the last round
//   run_sobol()  (SobolOut alone) k' + 2 sub-rounds a round into the round's rows, the reduction behind A's, mc_sobol.hip's sums
//                behind the last one and its closing kernel behind the last round
// A host form is its run between the upload of x0 and the copies back of its staged outputs (host_stage.hpp).  A new kind is a tail, its two
// extern "C" entries and, where it has a workspace, a field of McPlan.
#include "driven_params.hpp"
#include "host_stage.hpp"
#include "mc_effects.hip.hpp"
#include "mc_factorial.hip.hpp"
#include "mc_moments.hip.hpp"
#include "mc_quantiles.hip.hpp"
#include "mc_sobol.hip.hpp"
#include "measure_tables.hpp"
#include "sketch_image.hip.hpp"
#include "tolerance_mc.hip.hpp"

using namespace ezpz;

namespace {

static_assert(sizeof(EzpzMcDist) == 24 && sizeof(EzpzMcStats) == 88 && sizeof(EzpzMcTotals) == 24 && sizeof(EzpzMcConfig) == 16,
              "the layouts include/ezpz_amd.h documents");

using mcb::kBlock;  // samples per block of the sums
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
    // the host forms' staging (host_stage.hpp): x0 and every output of the call
    DevBuf<unsigned char> host_stage;
    // the run with contributors: the moments' workspace
    mcb::Work moment_work;
    // the run with Sobol indices: the round's rows -- [k + 2][chunk][n_meas] values and flags, [k + 2][chunk] ok bytes
    // -- and the sums' workspace
    DevBuf<double> rows_f;
    DevBuf<uint8_t> rows_flags, rows_ok;
    mcb::Work sobol_work;
    // the run with quantiles: every sample's m, flags and ok -- samples x n_meas x 9 + samples bytes, the one
    // workspace here that grows with samples -- and the selection's workspace
    DevBuf<double> all_m;
    DevBuf<uint8_t> all_flags, all_ok;
    mcq::SelectWork select_work;
    // the run with effects: the cells' workspace, and the edges [k][bins - 1] with what the buffer holds
    mcb::Work effect_work;
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

// Every sample's m, flags and ok on the device, for a tail that reads them behind the last round: a caller's device keep-buffer
// where one is given -- the round's copies into it fill it -- else (NULL) the plan's all_m, all_flags, all_ok.
struct Rows {
    double* m = nullptr;
    uint8_t *flags = nullptr, *ok = nullptr;
};

// What a run needs of the plan's device buffers (the tables and the host forms' buffers apart): the round's, listed here, and the
// tail's, which the tail lists.  visit() is the one list of them.
struct Needs {
    uint64_t chunk, samples;
    size_t n_vars, n_param, n_meas;
    size_t rows;  // 1: run()'s m, flags and ok; k + 2: run_sobol()'s rows
    Rows kept;    // where the tail has the rows kept: the caller's buffers that stand in for the plan's

    // Every buffer with the count it has to hold.  grow == false: does any of them have to grow (1) or none (0); grow == true:
    // grow them (EZPZ_OK or the error).  A buffer cannot be in one answer and missing from the other.
    template <class Tail>
    int visit(McPlan& P, const Tail& tail, bool grow) const {
        const uint64_t blocks = chunk / kBlock;
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
        }
        if (tail.keeps_rows()) {
            if (!kept.m) buf(P.all_m, samples * n_meas);
            if (!kept.flags) buf(P.all_flags, samples * n_meas);
            if (!kept.ok) buf(P.all_ok, samples);
        }
        tail.needs(P, *this, work);
        return rc;
    }
};

// ---- the kinds: each a tail of the run --------------------------------------------------------------------------------------------
// A tail holds what its entry was given (its outputs: device pointers in a run, host pointers in a host form's entry) and owns what
// is the kind's: check() -- its argument errors, behind the run's; outputs() -- the ONE list of its outputs with their element
// counts, which is both a host form's staging and the rule "an output with elements must be given"; needs() -- its workspaces;
// keeps_rows() -- does it read every sample's rows behind the last round; upload() -- what it writes from the host before the
// launches; behind_round() and behind_run() -- what it enqueues behind a round's reduction and behind the last round.
struct Plain {
    int check(const Call&, Request&) { return EZPZ_OK; }
    template <class F>
    void outputs(size_t, size_t, F&&) {}
    template <class W>
    void needs(McPlan&, const Needs&, W&) const {}
    bool keeps_rows() const { return false; }
    int upload(McPlan&, const Call&) const { return EZPZ_OK; }
    int behind_round(McPlan&, const Call&, uint64_t, uint64_t) const { return EZPZ_OK; }
    int behind_run(McPlan&, const Call&, const Rows&) const { return EZPZ_OK; }
};

// is an output that has elements missing (the pointers are only compared with NULL; without samples nothing is written)
template <class Tail>
bool output_missing(Tail& tail, const Call& c) {
    bool missing = false;
    if (c.samples) tail.outputs(c.n_param, c.n_meas, [&](auto*& p, size_t count) { missing = missing || (count && !p); });
    return missing;
}

// Contributors (ezpz_system_tolerance_mc_contrib[_device]): mc_moments.hip's sums on every round's params, m, flags and
// ok, its closing kernel behind the last round.
struct Contrib : Plain {
    const EzpzMcContribConfig* cc = nullptr;
    double* moments = nullptr;
    EzpzMcMomentsInfo* info = nullptr;
    double *cov = nullptr, *beta = nullptr, *contrib = nullptr, *r2 = nullptr;
    uint64_t* dropped = nullptr;
    double pivot_rel = 0.0;  // as checked

    int check(const Call& c, Request&) {
        if (int rc = mcm::check_shape(c.n_param, c.n_meas)) return rc;
        if (int rc = mcm::check_config(cc, pivot_rel)) return rc;
        return output_missing(*this, c) ? EZPZ_ERR_INVALID_ARGUMENT : EZPZ_OK;
    }
    template <class F>
    void outputs(size_t k, size_t m, F&& f) {
        const size_t K = k + m;
        f(moments, mcm::entries_of((uint32_t)K)), f(cov, K * K), f(beta, k * m), f(contrib, k * m), f(r2, m), f(info, 1), f(dropped, 1);
    }
    template <class W>
    void needs(McPlan& P, const Needs& n, W& work) const {
        const uint64_t blocks = n.chunk / kBlock;
        work(P.moment_work, blocks * mcm::entries_of((uint32_t)(n.n_param + n.n_meas)), blocks);
    }
    int behind_round(McPlan& P, const Call& c, uint64_t first, uint64_t count) const {
        mcm::MomentArgs a{};
        a.params = P.params.p, a.m = P.m.p, a.flags = P.flags.p, a.ok = P.ok.p;
        a.nominal_p = P.tab.p + 4 * c.n_meas, a.nominal_m = P.nominal.p;
        a.first = first, a.count = count, a.samples = c.samples;
        a.k = (uint32_t)c.n_param, a.n_meas = (uint32_t)c.n_meas, a.first_round = first == 0;
        a.moments = moments, a.info = info;
        return mcm::enqueue_moments(P.moment_work, a, c.stream);
    }
    int behind_run(McPlan&, const Call& c, const Rows&) const {
        mcm::ContribArgs a{};
        a.moments = moments, a.info = info;
        a.k = (uint32_t)c.n_param, a.m = (uint32_t)c.n_meas;
        a.pivot_rel = pivot_rel;
        a.cov = cov, a.beta = beta, a.contrib = contrib, a.r2 = r2, a.dropped = dropped;
        return mcm::enqueue_contributors(a, c.stream);
    }
};

// Quantiles (ezpz_system_tolerance_mc_quantiles[_device]): every round's rows kept, mc_quantiles.hip's selection behind
// the last round.  probs: host memory.  n_q == 0: the plain run.
struct Quant : Plain {
    const EzpzMcQuantileConfig* qc = nullptr;
    const double* probs = nullptr;
    size_t n_q = 0;
    EzpzMcQuantile* out = nullptr;
    double z = 0.0;  // as checked

    int check(const Call& c, Request&) { return mcq::check(c.samples, c.n_meas, probs, n_q, qc, c.sys, out, z); }  // (the rows are the run's own)
    template <class F>
    void outputs(size_t, size_t m, F&& f) {
        f(out, m * n_q);
    }
    template <class W>
    void needs(McPlan& P, const Needs& n, W& work) const {
        if (n_q) work(P.select_work, (uint32_t)n.n_meas, (uint32_t)n_q);
    }
    bool keeps_rows() const { return n_q != 0; }
    int behind_run(McPlan& P, const Call& c, const Rows& rows) const {
        if (!n_q) return EZPZ_OK;
        return mcq::enqueue_select(P.select_work, rows.m, rows.flags, rows.ok, c.samples, (uint32_t)c.n_meas, probs, (uint32_t)n_q, z, out,
                                   c.sys->lim.cus, c.stream);
    }
};

// Main effects (ezpz_system_tolerance_mc_effects[_device]): mc_effects.hip's cells on every round's params, m, flags,
// ok and the run's edges, its closing kernel behind the last round.  edges: host memory, read by check().
struct Effects : Plain {
    const EzpzMcEffectConfig* ec = nullptr;
    const double* edges = nullptr;
    double* sums = nullptr;
    uint64_t* counts = nullptr;
    double *cond_mean = nullptr, *cond_var = nullptr, *eta2 = nullptr, *first = nullptr;
    uint32_t* bins_used = nullptr;
    uint32_t bins = 0;  // as checked

    int check(const Call& c, Request&) {
        EzpzMcEffectConfig conf;
        mce::default_config(&conf);
        if (ec) conf = *ec;
        if (int rc = mce::check_shape(c.n_param, c.n_meas, conf.bins)) return rc;
        bins = conf.bins;
        if ((c.samples && !edges) || output_missing(*this, c)) return EZPZ_ERR_INVALID_ARGUMENT;
        return edges ? mce::check_edges(edges, c.n_param, bins) : EZPZ_OK;
    }
    template <class F>
    void outputs(size_t k, size_t m, F&& f) {
        const size_t cells = k * bins * m;
        f(sums, 2 * cells), f(counts, cells), f(cond_mean, cells), f(cond_var, cells), f(eta2, k * m), f(first, k * m), f(bins_used, k * m);
    }
    template <class W>
    void needs(McPlan& P, const Needs& n, W& work) const {
        const uint64_t cells = n.chunk / kBlock * n.n_param * bins * n.n_meas;  // of every block
        work(P.effect_work, cells * 2, cells);
    }
    // the edges where the kernels read them: others than the buffer holds wait for the last run's launches first
    int upload(McPlan& P, const Call& c) const {
        const size_t count = c.n_param * (bins - 1);
        if (P.effect_edges.p && P.effect_edges_kept.size() == count &&
            std::equal(edges, edges + count, P.effect_edges_kept.begin(), [](double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }))
            return EZPZ_OK;
        release_thread_kernel(c.sys->device);
        int rc;
        if ((rc = P.order.before_overwrite()) != EZPZ_OK) return rc;
        P.effect_edges_kept.clear();
        if ((rc = P.effect_edges.ensure(count)) != EZPZ_OK) return rc;
        HIP_TRY(hipMemcpy(P.effect_edges.p, edges, count * sizeof(double), hipMemcpyHostToDevice));
        P.effect_edges_kept.assign(edges, edges + count);
        call_stamp(MC_TABLES_UPLOADED);
        return EZPZ_OK;
    }
    int behind_round(McPlan& P, const Call& c, uint64_t first_sample, uint64_t count) const {
        mce::EffectArgs a{};
        a.params = P.params.p, a.m = P.m.p, a.flags = P.flags.p, a.ok = P.ok.p;
        a.nominal_m = P.nominal.p;
        a.edges = P.effect_edges.p;
        a.count = count;
        a.k = (uint32_t)c.n_param, a.n_meas = (uint32_t)c.n_meas, a.bins = bins, a.first_round = first_sample == 0;
        a.sums = sums, a.counts = counts;
        return mce::enqueue_effects(P.effect_work, a, c.stream);
    }
    int behind_run(McPlan& P, const Call& c, const Rows&) const {
        mce::CloseArgs a{};
        a.sums = sums, a.counts = counts;
        a.nominal_m = P.nominal.p;
        a.k = (uint32_t)c.n_param, a.m = (uint32_t)c.n_meas, a.bins = bins;
        a.cond_mean = cond_mean, a.cond_var = cond_var, a.eta2 = eta2, a.first = first, a.bins_used = bins_used;
        return mce::enqueue_close(a, c.stream);
    }
};

// Factorial effects (ezpz_system_tolerance_mc_factorial[_device]): every round's rows kept as for the quantiles,
// mc_factorial.hip's transform behind the last round.  coef is optional: no elements where it is NULL.
struct Fact : Plain {
    mcf::FactorialOut out;
    uint32_t kc = 0;  // the CORNER dimensions, as checked

    int check(const Call& c, Request& r) {
        if (c.n_meas == 0 || c.n_meas > mcf::kMaxMeas) return EZPZ_ERR_INVALID_ARGUMENT;
        kc = 0;
        for (const mc::Dist& d : r.dists) {
            if (d.kind != EZPZ_MC_CORNER && d.kind != EZPZ_MC_FIXED) return EZPZ_ERR_INVALID_ARGUMENT;
            if (d.kind == EZPZ_MC_CORNER) ++kc;
        }
        if (kc == 0 || kc > mcf::kMaxCorners) return EZPZ_ERR_INVALID_ARGUMENT;
        if (c.samples && c.samples != 1ull << kc) return EZPZ_ERR_INVALID_ARGUMENT;
        return output_missing(*this, c) ? EZPZ_ERR_INVALID_ARGUMENT : EZPZ_OK;
    }
    template <class F>
    void outputs(size_t, size_t m, F&& f) {
        f(out.info, m), f(out.main, m * kc), f(out.pair, m * kc * kc), f(out.ss_order, m * (kc + 1)), f(out.ss_total, m * kc);
        f(out.first, m * kc), f(out.total, m * kc), f(out.coef, out.coef ? m << kc : 0);
    }
    template <class W>
    void needs(McPlan& P, const Needs& n, W& work) const {
        work(P.factorial_work, (uint32_t)n.n_meas, kc);
    }
    bool keeps_rows() const { return true; }
    int behind_run(McPlan& P, const Call& c, const Rows& rows) const {
        return mcf::enqueue_factorial(P.factorial_work, rows.m, rows.flags, rows.ok, P.nominal.p, kc, (uint32_t)c.n_meas, out, c.sys->lim.cus, c.stream);
    }
};

// The picture (ezpz_system_tolerance_mc_image[_device]): every round's solved variants -- the round's x_out with its ok
// bytes -- drawn by ezpz_sketch_image_device behind the round's reduction; the first round's call zeroes counts and info, the others
// add.  items and view: host memory.  The rasteriser's workspace is the process's, not the plan's.
struct Image : Plain {
    const EzpzDrawItem* items = nullptr;
    size_t n_items = 0;
    const EzpzImageView* view = nullptr;
    uint32_t n_layers = 0;
    uint32_t* counts = nullptr;
    EzpzImageInfo* info = nullptr;

    // (the drawing entry's own check, on a round's variants; without samples nothing is written and no output is asked for)
    int check(const Call& c, Request& r) {
        const void* given = this;
        return skimg::check_request(given, (size_t)std::min<uint64_t>(c.samples, r.chunk), c.sys->counts.n_vars, items, n_items, view, n_layers,
                                    c.samples ? (const void*)counts : given, c.samples ? (const void*)info : given);
    }
    template <class F>
    void outputs(size_t, size_t, F&& f) {
        f(counts, view ? (size_t)n_layers * view->width * view->height : 0), f(info, 1);
    }
    int behind_round(McPlan& P, const Call& c, uint64_t first, uint64_t count) const {
        return ezpz_sketch_image_device(P.x_out.p, P.ok.p, count, c.sys->counts.n_vars, items, n_items, view, n_layers, first != 0, counts, info, c.stream);
    }
};

// Sobol indices (ezpz_system_tolerance_sobol[_device]): the tail of run_sobol(), which enqueues mc_sobol.hip's sums
// and closing kernel itself.
struct SobolOut {
    const EzpzSobolConfig* sc = nullptr;
    double* sums = nullptr;
    uint64_t* n_complete = nullptr;
    double *var = nullptr, *first = nullptr, *total = nullptr, *first_var = nullptr, *total_var = nullptr;
    uint64_t seed_b = 0;      // as checked
    uint32_t fixed_mask = 0;  // the FIXED dimensions

    // ... and the run's chunk
    int check(const Call& c, Request& r) {
        const size_t n_param = c.n_param, n_meas = c.n_meas;
        if (int rc = sobol::check_shape(n_param, n_meas)) return rc;
        EzpzSobolConfig s;
        sobol::default_config(&s);
        if (sc) s = *sc;
        if (s.seed_b == r.seed) return EZPZ_ERR_INVALID_ARGUMENT;
        seed_b = s.seed_b;
        fixed_mask = 0;
        for (size_t j = 0; j < n_param; ++j) {
            if (r.dists[j].kind == EZPZ_MC_CORNER) return EZPZ_ERR_INVALID_ARGUMENT;
            // (a flagged dimension's matrix B would be matrix A XOR a constant: the two are not independent, and pick-freeze needs that)
            if (r.dists[j].sequence) return EZPZ_ERR_INVALID_ARGUMENT;
            if (r.dists[j].kind == EZPZ_MC_FIXED) fixed_mask |= 1u << j;
        }
        if (output_missing(*this, c)) return EZPZ_ERR_INVALID_ARGUMENT;
        if (!(c.mc_cfg && c.mc_cfg->chunk)) {  // the library's choice: the rows and the copies of x0 each below the round's bound
            const uint64_t per_sample = std::max<uint64_t>({(uint64_t)c.sys->counts.n_vars, (uint64_t)(n_param + 2) * n_meas, 1}) * sizeof(double);
            const uint64_t chunk = std::max<uint64_t>(std::min<uint64_t>(kChunkValueBytes / per_sample, kDefaultSampleChunk) / kBlock * kBlock, kBlock);
            r.chunk = std::min<uint64_t>(chunk, whole_blocks(c.samples));
        }
        return EZPZ_OK;
    }
    template <class F>
    void outputs(size_t k, size_t m, F&& f) {
        f(sums, m * sobol::width_of((uint32_t)k)), f(n_complete, m), f(var, m), f(first, k * m), f(total, k * m), f(first_var, k * m), f(total_var, k * m);
    }
    template <class W>
    void needs(McPlan& P, const Needs& n, W& work) const {
        const uint64_t blocks = n.chunk / kBlock;
        work(P.sobol_work, blocks * n.n_meas * sobol::width_of((uint32_t)n.n_param), blocks * n.n_meas);
    }
    bool keeps_rows() const { return false; }
};

// What the host writes before a run's launches, behind the last run's, and the nominal: nominal[i] = m(record i, x0), 0 where
// the guard fires.  `c` holds device pointers.
template <class Tail>
int prepare(McPlan& P, const Request& r, const Call& c, const Needs& need, const Tail& tail) {
    release_thread_kernel(c.sys->device);
    const size_t dist_bytes = r.dists.size() * sizeof(mc::Dist), tab_bytes = r.tab.size() * sizeof(double);
    int rc;
    std::vector<unsigned char> tables(dist_bytes + tab_bytes);
    if (dist_bytes) std::memcpy(tables.data(), r.dists.data(), dist_bytes);
    if (tab_bytes) std::memcpy(tables.data() + dist_bytes, r.tab.data(), tab_bytes);
    if (tables != P.tables_kept || !P.ticket.p || need.visit(P, tail, false)) {
        if ((rc = P.order.before_overwrite()) != EZPZ_OK) return rc;
        P.tables_kept.clear();
        if ((rc = P.dist.ensure(r.dists.size())) != EZPZ_OK || (rc = P.tab.ensure(r.tab.size())) != EZPZ_OK) return rc;
        if (dist_bytes) HIP_TRY(hipMemcpy(P.dist.p, r.dists.data(), dist_bytes, hipMemcpyHostToDevice));
        if (tab_bytes) HIP_TRY(hipMemcpy(P.tab.p, r.tab.data(), tab_bytes, hipMemcpyHostToDevice));
        if ((rc = need.visit(P, tail, true)) != EZPZ_OK) return rc;
        if (!P.ticket.p) {
            if ((rc = P.ticket.ensure(1)) != EZPZ_OK) return rc;
            HIP_TRY(hipMemset(P.ticket.p, 0, P.ticket.cap * sizeof(unsigned int)));
        }
        P.tables_kept = std::move(tables);
        call_stamp(MC_TABLES_UPLOADED);
    }
    if ((rc = P.order.order_behind(c.stream)) != EZPZ_OK) return rc;
    // (run() measures where there are records; run_sobol() always does: SobolOut::check has seen to n_meas >= 1)
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

// The run of every kind but Sobol's: a round is one sub-round, the reduction behind it and what the tail enqueues behind that; the
// tail's closing step goes behind the last round.  Device pointers throughout (but Keep's, see there): the plan's mutex is held, the
// system's device current, the request checked and samples > 0.
template <class Tail>
int run(McPlan& P, const Request& r, const Call& c, const Keep& keep, const Tail& tail) {
    const size_t n_param = c.n_param, n_meas = c.n_meas;
    const uint64_t samples = c.samples, chunk = r.chunk;
    const hipStream_t stream = c.stream;
    int rc;
    Rows rows;  // (a caller's device buffer is filled by the round's copies into it)
    if (!keep.host) rows.m = keep.m, rows.flags = keep.flags, rows.ok = keep.ok;
    const Needs need{chunk, samples, c.sys->counts.n_vars, n_param, n_meas, 1, rows};
    if ((rc = tail.upload(P, c)) != EZPZ_OK || (rc = prepare(P, r, c, need, tail)) != EZPZ_OK) return rc;
    if (r.hist_bins && n_meas) HIP_TRY(hipMemsetAsync(c.hist, 0, n_meas * (r.hist_bins + 2) * sizeof(uint64_t), stream));
    mc::ReduceArgs a = reduce_args(P, need, P.m.p, P.flags.p, P.ok.p, r.limits, r.hist_bins, c.stats, c.totals, c.hist);
    for (uint64_t first = 0; first < samples; first += chunk) {
        const uint64_t count = std::min<uint64_t>(chunk, samples - first);
        if ((rc = sub_round(P, r, c, nullptr, first, count, P.m.p, P.flags.p)) != EZPZ_OK || (rc = enqueue_reduce(a, first, count, stream)) != EZPZ_OK ||
            (rc = tail.behind_round(P, c, first, count)) != EZPZ_OK)
            return rc;
        if (tail.keeps_rows()) {
            if ((rc = copy_out(rows.m ? nullptr : P.all_m.p + first * n_meas, P.m.p, count * n_meas * sizeof(double), false, stream)) != EZPZ_OK ||
                (rc = copy_out(rows.flags ? nullptr : P.all_flags.p + first * n_meas, P.flags.p, count * n_meas, false, stream)) != EZPZ_OK ||
                (rc = copy_out(rows.ok ? nullptr : P.all_ok.p + first, P.ok.p, count, false, stream)) != EZPZ_OK)
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
    if (!rows.m) rows.m = P.all_m.p;
    if (!rows.flags) rows.flags = P.all_flags.p;
    if (!rows.ok) rows.ok = P.all_ok.p;
    if ((rc = tail.behind_run(P, c, rows)) != EZPZ_OK) return rc;
    call_stamp(MC_LAUNCHED);
    return P.order.record(stream);
}

// The run with Sobol indices, on the same plan, kernels and entries as run(): a round is k' + 2 sub-rounds into the round's rows,
// with the reduction behind A's, the ok bytes behind every other one, mc_sobol.hip's sums behind the last one and its closing kernel
// behind the last round.  Device pointers throughout (but Keep's): the plan's mutex is held, the system's device current, the
// request checked and samples > 0.
int run_sobol(McPlan& P, const Request& r, const Call& c, const Keep& keep, const SobolOut& out) {
    const size_t n_param = c.n_param, n_meas = c.n_meas, R = n_param + 2;
    const uint64_t samples = c.samples, chunk = r.chunk;
    const hipStream_t stream = c.stream;
    int rc;
    const Needs need{chunk, samples, c.sys->counts.n_vars, n_param, n_meas, R, Rows{}};
    if ((rc = prepare(P, r, c, need, out)) != EZPZ_OK) return rc;
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

// Every entry, in the order the argument errors take precedence: the run's checks, the tail's, nothing to do for no samples -- up to
// here no output and nothing of the plan is touched -- then the run on the plan with its mutex held and the system's device current
// (SobolOut's run is run_sobol()).  A host form (`c`, `keep` and `tail` hold host pointers) is that run between the upload of x0
// and the copies back, once the stream has drained, of its outputs: the histogram, the tail's list, stats and totals, staged side
// by side on the device.
template <class Tail>
int entry(const Call& c, const Keep& keep, Tail& tail, bool host) {
    Request r;
    if (int rc = check_run(c, r)) return rc;
    if (int rc = tail.check(c, r)) return rc;
    if (c.samples == 0) return EZPZ_OK;
    McPlan& P = plan_of(c.sys);
    std::lock_guard<std::mutex> lock(P.mu);
    EZPZ_ON_DEVICE(c.sys->device);
    auto run_on = [&](const Call& on, const Tail& t) {
        if constexpr (std::is_same_v<Tail, SobolOut>)
            return run_sobol(P, r, on, keep, t);
        else
            return run(P, r, on, keep, t);
    };
    if (!host) return run_on(c, tail);
    const size_t n = c.sys->counts.n_vars;
    Call d = c;
    Tail dev = tail;
    Staged io;
    io.in(c.x0, n, d.x0, Staged::kPlaced);  // (the measure entry wants its x whatever n is)
    io.out(c.hist, c.n_meas * (r.hist_bins ? r.hist_bins + 2 : 0), d.hist);
    dev.outputs(c.n_param, c.n_meas, [&](auto*& p, size_t count) { io.out(p, count, p); });
    io.out(c.stats, c.n_meas, d.stats);
    io.out(c.totals, 1, d.totals);
    int rc;
    if ((rc = io.reserve(P.host_stage)) != EZPZ_OK || (rc = io.upload(P.host_stage)) != EZPZ_OK) return rc;
    if ((rc = run_on(d, dev)) != EZPZ_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c.stream));
    return io.copy_back(P.host_stage);
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
    Plain plain;
    return entry(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, plain, false);
}

int ezpz_system_tolerance_mc(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                             const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo, const double* lim_hi,
                             const double* hist_lo, const double* hist_hi, uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg,
                             EzpzMcStats* stats, EzpzMcTotals* totals, uint64_t* hist, double* keep_params, double* keep_m,
                             uint8_t* keep_flags, uint8_t* keep_ok) {
    const Call c{sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats, totals, hist, hipStreamPerThread};
    Plain plain;
    return entry(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, plain, true);
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
    o.cc = cc, o.moments = moments_dev, o.info = info_dev, o.cov = cov_dev, o.beta = beta_dev, o.contrib = contrib_dev, o.r2 = r2_dev, o.dropped = dropped_dev;
    return entry(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, o, false);
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
    o.cc = cc, o.moments = moments, o.info = info, o.cov = cov, o.beta = beta, o.contrib = contrib, o.r2 = r2, o.dropped = dropped;
    return entry(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, o, true);
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
    o.ec = ec, o.edges = edges, o.sums = sums_dev, o.counts = counts_dev, o.cond_mean = cond_mean_dev, o.cond_var = cond_var_dev;
    o.eta2 = eta2_dev, o.first = first_dev, o.bins_used = bins_used_dev;
    return entry(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, o, false);
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
    o.ec = ec, o.edges = edges, o.sums = sums, o.counts = counts, o.cond_mean = cond_mean, o.cond_var = cond_var;
    o.eta2 = eta2, o.first = first, o.bins_used = bins_used;
    return entry(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, o, true);
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
    q.qc = qc, q.probs = probs, q.n_q = n_q, q.out = out_dev;
    return entry(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, q, false);
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
    q.qc = qc, q.probs = probs, q.n_q = n_q, q.out = out;
    return entry(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, q, true);
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
    return entry(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, f, false);
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
    return entry(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, f, true);
}

int ezpz_system_tolerance_mc_image_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                          const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                          const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                          uint64_t samples, const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats_dev,
                                          EzpzMcTotals* totals_dev, uint64_t* hist_dev, double* keep_params_dev, double* keep_m_dev,
                                          uint8_t* keep_flags_dev, uint8_t* keep_ok_dev, const EzpzDrawItem* items, size_t n_items,
                                          const EzpzImageView* view, uint32_t n_layers, uint32_t* counts_dev, EzpzImageInfo* info_dev,
                                          void* stream) {
    const Call c{sys, x0_dev, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats_dev, totals_dev, hist_dev, (hipStream_t)stream};
    Image o;
    o.items = items, o.n_items = n_items, o.view = view, o.n_layers = n_layers, o.counts = counts_dev, o.info = info_dev;
    return entry(c, Keep{keep_params_dev, keep_m_dev, keep_flags_dev, keep_ok_dev, false}, o, false);
}

int ezpz_system_tolerance_mc_image(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                   const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo,
                                   const double* lim_hi, const double* hist_lo, const double* hist_hi, uint64_t samples,
                                   const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, EzpzMcStats* stats, EzpzMcTotals* totals,
                                   uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags, uint8_t* keep_ok,
                                   const EzpzDrawItem* items, size_t n_items, const EzpzImageView* view, uint32_t n_layers,
                                   uint32_t* counts, EzpzImageInfo* info) {
    const Call c{sys, x0, positions, n_param, dist, nominal, records, n_meas, lim_lo, lim_hi, hist_lo, hist_hi, samples, mc_cfg, cfg,
                 stats, totals, hist, hipStreamPerThread};
    Image o;
    o.items = items, o.n_items = n_items, o.view = view, o.n_layers = n_layers, o.counts = counts, o.info = info;
    return entry(c, Keep{keep_params, keep_m, keep_flags, keep_ok, true}, o, true);
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
    o.sc = sc, o.sums = sums_dev, o.n_complete = n_complete_dev, o.var = var_dev, o.first = first_dev, o.total = total_dev;
    o.first_var = first_var_dev, o.total_var = total_var_dev;
    return entry(c, Keep{nullptr, keep_f_dev, keep_flags_dev, keep_ok_dev, false}, o, false);
}

int ezpz_system_tolerance_sobol(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                const double* nominal, const EzpzConstraint* records, size_t n_meas, uint64_t samples,
                                const EzpzMcConfig* mc_cfg, const EzpzConfig* cfg, const EzpzSobolConfig* sc, EzpzMcStats* stats,
                                EzpzMcTotals* totals, double* sums, uint64_t* n_complete, double* var, double* first, double* total,
                                double* first_var, double* total_var, double* keep_f, uint8_t* keep_flags, uint8_t* keep_ok) {
    const Call c{sys, x0, positions, n_param, dist, nominal, records, n_meas, nullptr, nullptr, nullptr, nullptr, samples, mc_cfg, cfg,
                 stats, totals, nullptr, hipStreamPerThread};
    SobolOut o;
    o.sc = sc, o.sums = sums, o.n_complete = n_complete, o.var = var, o.first = first, o.total = total, o.first_var = first_var, o.total_var = total_var;
    return entry(c, Keep{nullptr, keep_f, keep_flags, keep_ok, true}, o, true);
}

}  // extern "C"
