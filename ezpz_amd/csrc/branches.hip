// Solution branches (include/ezpz_amd.h: ezpz_branch_cluster, ezpz_system_solve_branches and their _device forms):
// the host side of branches.hip.hpp's kernels -- the check of a request, the plan (the round's workspace, the compared variables'
// and the sampler's tables, the host forms' staging) and the rounds.  A round of the run is the start kernel ->
// ezpz_system_solve_batch_device -> assign -> elect, all on the caller's stream: the solve is that entry itself, with its routes,
// its locks and its ordering.  The leader table lives in the caller's outputs between rounds.
#include "branches.hip.hpp"
#include "host_stage.hpp"

using namespace ezpz;

namespace {

static_assert(sizeof(EzpzBranchConfig) == 32 && sizeof(EzpzBranchInfo) == 32 && sizeof(EzpzBranch) == 56,
              "the layouts include/ezpz_amd.h documents");

constexpr uint64_t kBlock = 256;                     // a round is a multiple of this, as the Monte-Carlo entry's
constexpr uint64_t kDefaultChunk = 65536;            // samples per base and round where the caller leaves the choice ...
constexpr uint64_t kChunkValueBytes = 256ull << 20;  // ... while one of the round's two value arrays stays below this
constexpr uint64_t kFirstRound = 1024;               // round 0 meets an empty table and is all election: it is kept short
constexpr uint64_t kMaxRoundValues = 1ull << 40;     // more values in one round than any device holds: declined, not computed with

struct BranchPlan {
    std::mutex mu;  // a run holds it from its first upload to its last enqueue
    // The completion of the last run's launches: a run on another stream goes behind it, and whatever a run overwrites from the
    // host -- the tables, a buffer that has to grow -- waits for it first
    LaunchOrder order;
    std::vector<unsigned char> tables_kept;  // what `cmp` and `dist` hold
    DevBuf<uint32_t> cmp, pend;
    DevBuf<mc::Dist> dist;
    DevBuf<double> x_in, x_out;
    DevBuf<EzpzStatus> status;
    DevBuf<int32_t> label;
    DevBuf<unsigned char> host_stage;  // the host forms' staging (host_stage.hpp)
};

BranchPlan& plan_of(EzpzSystem* sys) {
    std::lock_guard<std::mutex> lock(sys->mu);
    if (!sys->branches) sys->branches = std::make_shared<BranchPlan>();
    return *static_cast<BranchPlan*>(sys->branches.get());
}

struct Request {
    std::vector<uint32_t> cmp;    // the compared variables, ascending
    std::vector<mc::Dist> dists;  // the run's sampler table (nominal unused: the start kernel takes it per base)
    uint64_t seed = 0, chunk = 0;
    uint32_t max_branches = 0;
    double eps_abs = 0.0, eps_rel = 0.0;
};

// The argument errors of the rule's part of a request, and its tables.  `values_per_sample`: what a round keeps per sample in its
// workspace (the run: n_vars; the clustering alone reads the caller's array: 0).
int check_rule(const uint8_t* compare, size_t n_vars, uint64_t batch, uint64_t samples, const EzpzBranchConfig* cfg, uint64_t values_per_sample,
               Request& r) {
    EzpzBranchConfig c;
    ezpz_default_branch_config(&c);
    if (cfg) c = *cfg;
    if (c.max_branches == 0 || c.max_branches > EZPZ_BRANCH_MAX) return EZPZ_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(c.eps_abs) || !std::isfinite(c.eps_rel) || c.eps_abs < 0.0 || c.eps_rel < 0.0) return EZPZ_ERR_INVALID_ARGUMENT;
    if (n_vars > 0xFFFFFFFEull) return EZPZ_ERR_INVALID_ARGUMENT;
    r.cmp.clear();
    for (size_t v = 0; v < n_vars; ++v)
        if (!compare || compare[v]) r.cmp.push_back((uint32_t)v);
    if (r.cmp.empty()) return EZPZ_ERR_INVALID_ARGUMENT;
    r.seed = c.seed;
    r.max_branches = c.max_branches;
    r.eps_abs = c.eps_abs;
    r.eps_rel = c.eps_rel;
    if (batch > 0xFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    const uint64_t per_sample = std::max<uint64_t>(batch, 1) * std::max<uint64_t>(values_per_sample, 1);  // (both below 2^32)
    uint64_t chunk = c.chunk;
    if (chunk == 0) {
        chunk = kDefaultChunk;
        while (chunk > kBlock && chunk > kChunkValueBytes / sizeof(double) / per_sample) chunk /= 2;
    }
    r.chunk = round_chunk(chunk, samples, kBlock);
    // a round's workspace is batch x chunk x n_vars values: no product below may wrap
    if (r.chunk > kMaxRoundValues / per_sample) return EZPZ_ERR_TOO_LARGE;
    return EZPZ_OK;
}

// The round that begins at `first`: round 0 is short (see kFirstRound), the others are the chunk.
uint64_t round_count(const Request& r, uint64_t first, uint64_t samples) {
    return std::min<uint64_t>(first == 0 ? std::min(r.chunk, kFirstRound) : r.chunk, samples - first);
}

uint32_t stride_grid(uint64_t items, int cus) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, (uint64_t)cus * 16));
}

// The tables and the clustering workspace of a run where the plan's are another run's or too small: behind the last run's launches.
// `solve_values`: batch * chunk * n_vars of the run (0: the clustering alone), `label_count`: the labels the workspace has to hold.
int prepare(BranchPlan& P, const Request& r, uint64_t batch, uint64_t solve_values, uint64_t solve_systems, uint64_t label_count) {
    std::vector<unsigned char> tables(r.cmp.size() * sizeof(uint32_t) + r.dists.size() * sizeof(mc::Dist));
    std::memcpy(tables.data(), r.cmp.data(), r.cmp.size() * sizeof(uint32_t));
    if (!r.dists.empty()) std::memcpy(tables.data() + r.cmp.size() * sizeof(uint32_t), r.dists.data(), r.dists.size() * sizeof(mc::Dist));
    const uint64_t pend_count = batch * r.chunk;
    const bool grows = pend_count > P.pend.cap || label_count > P.label.cap || solve_values > P.x_in.cap || solve_values > P.x_out.cap ||
                       solve_systems > P.status.cap;
    if (tables == P.tables_kept && !grows) return EZPZ_OK;
    int rc;
    if ((rc = P.order.before_overwrite()) != EZPZ_OK) return rc;
    P.tables_kept.clear();
    if ((rc = P.cmp.ensure(r.cmp.size())) != EZPZ_OK || (rc = P.dist.ensure(r.dists.size())) != EZPZ_OK ||
        (rc = P.pend.ensure(pend_count)) != EZPZ_OK || (rc = P.label.ensure(label_count)) != EZPZ_OK ||
        (rc = P.x_in.ensure(solve_values)) != EZPZ_OK || (rc = P.x_out.ensure(solve_values)) != EZPZ_OK ||
        (rc = P.status.ensure(solve_systems)) != EZPZ_OK)
        return rc;
    HIP_TRY(hipMemcpy(P.cmp.p, r.cmp.data(), r.cmp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!r.dists.empty()) HIP_TRY(hipMemcpy(P.dist.p, r.dists.data(), r.dists.size() * sizeof(mc::Dist), hipMemcpyHostToDevice));
    P.tables_kept = std::move(tables);
    call_stamp(BRANCH_TABLES_UPLOADED);
    return EZPZ_OK;
}

int clear_outputs(const Request& r, uint64_t batch, size_t n_vars, EzpzBranchInfo* info, EzpzBranch* branches, double* x_branch,
                  hipStream_t stream) {
    HIP_TRY(hipMemsetAsync(info, 0, batch * sizeof(EzpzBranchInfo), stream));
    HIP_TRY(hipMemsetAsync(branches, 0, batch * r.max_branches * sizeof(EzpzBranch), stream));
    HIP_TRY(hipMemsetAsync(x_branch, 0, batch * r.max_branches * n_vars * sizeof(double), stream));
    return EZPZ_OK;
}

template <int G>
void launch_assign(const branch::Round& a, uint32_t tile_leaders, int cus, hipStream_t stream) {
    const uint32_t span = 256 / G * branch::kSamplesPerGroup, spans = (a.count + span - 1) / span;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(a.batch * spans, (uint64_t)cus * 32));
    hipLaunchKernelGGL(branch::branch_assign_kernel<G>, dim3(grid), dim3(256), (size_t)tile_leaders * a.n_cmp * sizeof(double), stream, a,
                       tile_leaders, spans);
}

// The clustering of one round: assign (unless the round is the first: no leaders yet) and elect.
int enqueue_round(branch::Round& a, int cus, hipStream_t stream) {
    a.fresh = a.first == 0;
    if (!a.fresh) {
        // leaders per LDS tile; a row of compared values that does not fit a tile is read from global memory (0)
        const uint32_t tile_leaders = std::min<uint32_t>(a.max_branches, branch::kTileDoubles / a.n_cmp);
        if (a.n_cmp <= 8)
            launch_assign<8>(a, tile_leaders, cus, stream);
        else if (a.n_cmp <= 16)
            launch_assign<16>(a, tile_leaders, cus, stream);
        else if (a.n_cmp <= 32)
            launch_assign<32>(a, tile_leaders, cus, stream);
        else
            launch_assign<64>(a, tile_leaders, cus, stream);
    }
    hipLaunchKernelGGL(branch::branch_elect_kernel, dim3((uint32_t)std::min<uint64_t>(a.batch, (uint64_t)cus * 32)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

branch::Round round_args(BranchPlan& P, const Request& r, uint64_t batch, uint64_t samples, size_t n_vars, EzpzBranchInfo* info,
                         EzpzBranch* branches, double* x_branch) {
    branch::Round a{};
    a.cmp = P.cmp.p;
    a.n_cmp = (uint32_t)r.cmp.size();
    a.n_vars = (uint32_t)n_vars;
    a.batch = batch;
    a.samples = samples;
    a.max_branches = r.max_branches;
    a.eps_abs = r.eps_abs;
    a.eps_rel = r.eps_rel;
    a.pend = P.pend.p;
    a.info = info;
    a.branches = branches;
    a.x_branch = x_branch;
    return a;
}

// The clustering alone, device pointers throughout: the plan's mutex is held, the device current, the request checked, batch and
// samples > 0.
int cluster(BranchPlan& P, const Request& r, int cus, const double* x_dev, const uint8_t* ok_dev, uint64_t batch, uint64_t samples, size_t n_vars,
            EzpzBranchInfo* info, EzpzBranch* branches, double* x_branch, int32_t* keep_label, hipStream_t stream) {
    int rc;
    if ((rc = prepare(P, r, batch, 0, 0, keep_label ? 0 : batch * r.chunk)) != EZPZ_OK) return rc;
    if ((rc = P.order.order_behind(stream)) != EZPZ_OK) return rc;
    if ((rc = clear_outputs(r, batch, n_vars, info, branches, x_branch, stream)) != EZPZ_OK) return rc;
    branch::Round a = round_args(P, r, batch, samples, n_vars, info, branches, x_branch);
    a.x_stride = samples;
    a.origin = x_dev;  // sample 0 of the base
    a.origin_stride = samples * n_vars;
    for (uint64_t first = 0; first < samples;) {
        const uint64_t count = round_count(r, first, samples);
        a.x = x_dev + first * n_vars;
        a.ok = ok_dev ? ok_dev + first : nullptr;
        a.first = first;
        a.count = (uint32_t)count;
        a.label = keep_label ? keep_label + first : P.label.p;
        a.label_stride = keep_label ? samples : count;
        if ((rc = enqueue_round(a, cus, stream)) != EZPZ_OK) return rc;
        first += count;
    }
    call_stamp(BRANCH_LAUNCHED);
    return P.order.record(stream);
}

// Every argument error of a clustering call, before anything is enqueued or written.  The pointers are only compared with NULL.
int check_cluster(const void* x, size_t batch, uint64_t samples, size_t n_vars, const uint8_t* compare, const EzpzBranchConfig* cfg,
                  const void* info, const void* branches, const void* x_branch, Request& r) {
    if (int rc = check_rule(compare, n_vars, batch, samples, cfg, 0, r)) return rc;
    if (samples > 0xFFFFFFFFFFFFull || batch > 0xFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    if (batch && samples && (!x || !info || !branches || !x_branch)) return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

// Every argument error of a run.  `x0_host`: the host form's base rows, whose values the sampler's check reads (NULL: the device form).
int check_run(EzpzSystem* sys, const void* x0, const double* x0_host, const EzpzMcDist* dist, const uint8_t* compare, size_t batch,
              uint64_t samples, const EzpzBranchConfig* cfg, const void* info, const void* branches, const void* x_branch, Request& r) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    const size_t n = sys->counts.n_vars;
    if (int rc = check_rule(compare, n, batch, samples, cfg, n, r)) return rc;
    if (samples > 0xFFFFFFFFFFFFull || batch > 0xFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    // the sampler's errors, by the sampler's own check: on every base row where the host has them, else on a row of zeros
    if (!dist) return EZPZ_ERR_INVALID_ARGUMENT;
    if (x0_host) {
        for (size_t b = 0; b < batch; ++b)
            if (int rc = ezpz_mc_sample(0, dist, x0_host + b * n, n, 0, 0, nullptr)) return rc;
    }
    const std::vector<double> zeros(n, 0.0);
    if (int rc = ezpz_mc_sample(0, dist, zeros.data(), n, 0, 0, nullptr)) return rc;
    r.dists.resize(n);
    uint32_t corners = 0;
    for (size_t v = 0; v < n; ++v) {
        // (a flagged dimension has 2^32 samples: ezpz_mc_sample's error for first + count past them)
        if (mc::sequenced(dist[v]) && samples > 1ull << 32) return EZPZ_ERR_INVALID_ARGUMENT;
        r.dists[v] = mc::dist_of(dist[v], dist[v].kind == EZPZ_MC_CORNER ? corners++ : 0u, 0.0);
    }
    if (batch && samples && (!x0 || !info || !branches || !x_branch)) return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

// The run, device pointers throughout: the plan's mutex is held, the system's device current, the request checked, batch and
// samples > 0.
int run(EzpzSystem* sys, BranchPlan& P, const Request& r, const double* x0_dev, uint64_t batch, uint64_t samples, const EzpzConfig* cfg,
        EzpzBranchInfo* info, EzpzBranch* branches, double* x_branch, int32_t* keep_label, hipStream_t stream) {
    release_thread_kernel(sys->device);
    const size_t n = sys->counts.n_vars;
    const int cus = sys->lim.cus;
    int rc;
    if ((rc = prepare(P, r, batch, batch * r.chunk * n, batch * r.chunk, keep_label ? 0 : batch * r.chunk)) != EZPZ_OK) return rc;
    if ((rc = P.order.order_behind(stream)) != EZPZ_OK) return rc;
    if ((rc = clear_outputs(r, batch, n, info, branches, x_branch, stream)) != EZPZ_OK) return rc;
    branch::Round a = round_args(P, r, batch, samples, n, info, branches, x_branch);
    a.x = P.x_out.p;
    a.status = P.status.p;
    a.origin = x0_dev;
    a.origin_stride = n;
    for (uint64_t first = 0; first < samples;) {
        const uint64_t count = round_count(r, first, samples);
        hipLaunchKernelGGL(branch::branch_start_kernel, dim3(stride_grid(batch * count * n, cus)), dim3(256), 0, stream, P.dist.p, x0_dev, r.seed,
                           first, (uint32_t)count, batch, (uint32_t)n, P.x_in.p);
        HIP_TRY(hipGetLastError());
        if ((rc = ezpz_system_solve_batch_device(sys, P.x_in.p, batch * count, cfg, P.x_out.p, P.status.p, nullptr, nullptr, 0, stream)) != EZPZ_OK)
            return rc;
        a.x_stride = count;
        a.first = first;
        a.count = (uint32_t)count;
        a.label = keep_label ? keep_label + first : P.label.p;
        a.label_stride = keep_label ? samples : count;
        if ((rc = enqueue_round(a, cus, stream)) != EZPZ_OK) return rc;
        first += count;
    }
    call_stamp(BRANCH_LAUNCHED);
    return P.order.record(stream);
}

// The outputs of both host forms: their places on the list
struct HostOutputs {
    EzpzBranchInfo* info;
    EzpzBranch* branches;
    double* x_branch;
    int32_t* label;
    HostOutputs(Staged& io, const Request& r, uint64_t batch, uint64_t samples, size_t n_vars, EzpzBranchInfo* info_host, EzpzBranch* branches_host,
                double* x_branch_host, int32_t* keep_label) {
        io.out(info_host, batch, info);
        io.out(branches_host, batch * r.max_branches, branches);
        io.out(x_branch_host, batch * r.max_branches * n_vars, x_branch);
        io.out(keep_label, batch * samples, label);
    }
    HostOutputs(const HostOutputs&) = delete;  // (the list holds the members' addresses)
};

}  // namespace

extern "C" {

void ezpz_default_branch_config(EzpzBranchConfig* bcfg) {
    if (!bcfg) return;
    bcfg->seed = 0;
    bcfg->chunk = 0;
    bcfg->max_branches = 32;
    bcfg->eps_abs = 1e-5;
    bcfg->eps_rel = 1e-5;
}

int ezpz_branch_cluster_device(const double* x_dev, const uint8_t* ok_dev, const uint8_t* compare, size_t batch, uint64_t samples, size_t n_vars,
                               const EzpzBranchConfig* bcfg, EzpzBranchInfo* info_dev, EzpzBranch* branches_dev, double* x_branch_dev,
                               int32_t* keep_label_dev, void* stream) {
    Request r;
    if (int rc = check_cluster(x_dev, batch, samples, n_vars, compare, bcfg, info_dev, branches_dev, x_branch_dev, r)) return rc;
    if (samples == 0 || batch == 0) return EZPZ_OK;
    BranchPlan* P = nullptr;
    int device = -1;
    if (int rc = plan_of_device(P, device)) return device < 0 ? EZPZ_ERR_HIP : rc;  // (a failing hipGetDevice is the runtime's error here, as ever)
    std::lock_guard<std::mutex> lock(P->mu);
    return cluster(*P, r, device_limits(device).cus, x_dev, ok_dev, batch, samples, n_vars, info_dev, branches_dev, x_branch_dev, keep_label_dev,
                   (hipStream_t)stream);
}

int ezpz_branch_cluster(const double* x, const uint8_t* ok, const uint8_t* compare, size_t batch, uint64_t samples, size_t n_vars,
                        const EzpzBranchConfig* bcfg, EzpzBranchInfo* info, EzpzBranch* branches, double* x_branch, int32_t* keep_label) {
    Request r;
    if (int rc = check_cluster(x, batch, samples, n_vars, compare, bcfg, info, branches, x_branch, r)) return rc;
    if (samples == 0 || batch == 0) return EZPZ_OK;
    // ezpz_branch_cluster has no system: its workspace is the process's, one per device (system.hpp: plan_of_device)
    BranchPlan* P = nullptr;
    int device = -1;
    if (int rc = plan_of_device(P, device)) return rc;
    std::lock_guard<std::mutex> lock(P->mu);
    const double* x_dev;
    const uint8_t* ok_dev;
    Staged io;
    io.in(x, batch * samples * n_vars, x_dev);
    io.in(ok, batch * samples, ok_dev);
    HostOutputs o(io, r, batch, samples, n_vars, info, branches, x_branch, keep_label);
    int rc;
    if ((rc = io.reserve(P->host_stage)) != EZPZ_OK || (rc = io.upload(P->host_stage)) != EZPZ_OK) return rc;
    if ((rc = cluster(*P, r, device_limits(device).cus, x_dev, ok_dev, batch, samples, n_vars, o.info, o.branches, o.x_branch, o.label,
                      hipStreamPerThread)) != EZPZ_OK)
        return rc;
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    return io.copy_back(P->host_stage);
}

int ezpz_system_solve_branches_device(EzpzSystem* sys, const double* x0_dev, const EzpzMcDist* dist, const uint8_t* compare, size_t batch,
                                      uint64_t samples, const EzpzBranchConfig* bcfg, const EzpzConfig* cfg, EzpzBranchInfo* info_dev,
                                      EzpzBranch* branches_dev, double* x_branch_dev, int32_t* keep_label_dev, void* stream) {
    Request r;
    if (int rc = check_run(sys, x0_dev, nullptr, dist, compare, batch, samples, bcfg, info_dev, branches_dev, x_branch_dev, r)) return rc;
    if (samples == 0 || batch == 0) return EZPZ_OK;
    BranchPlan& P = plan_of(sys);
    std::lock_guard<std::mutex> lock(P.mu);
    EZPZ_ON_DEVICE(sys->device);
    return run(sys, P, r, x0_dev, batch, samples, cfg, info_dev, branches_dev, x_branch_dev, keep_label_dev, (hipStream_t)stream);
}

int ezpz_system_solve_branches(EzpzSystem* sys, const double* x0, const EzpzMcDist* dist, const uint8_t* compare, size_t batch, uint64_t samples,
                               const EzpzBranchConfig* bcfg, const EzpzConfig* cfg, EzpzBranchInfo* info, EzpzBranch* branches,
                               double* x_branch, int32_t* keep_label) {
    Request r;
    if (int rc = check_run(sys, x0, batch && samples ? x0 : nullptr, dist, compare, batch, samples, bcfg, info, branches, x_branch, r)) return rc;
    if (samples == 0 || batch == 0) return EZPZ_OK;
    BranchPlan& P = plan_of(sys);
    std::lock_guard<std::mutex> lock(P.mu);
    EZPZ_ON_DEVICE(sys->device);
    const size_t n = sys->counts.n_vars;
    const double* x0_dev;
    Staged io;
    io.in(x0, batch * n, x0_dev);
    HostOutputs o(io, r, batch, samples, n, info, branches, x_branch, keep_label);
    int rc;
    if ((rc = io.reserve(P.host_stage)) != EZPZ_OK || (rc = io.upload(P.host_stage)) != EZPZ_OK) return rc;
    if ((rc = run(sys, P, r, x0_dev, batch, samples, cfg, o.info, o.branches, o.x_branch, o.label, hipStreamPerThread)) != EZPZ_OK) return rc;
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    return io.copy_back(P.host_stage);
}

}  // extern "C"
