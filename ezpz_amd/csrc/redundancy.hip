// Redundancy analysis (include/ezpz_amd.h: ezpz_system_redundancy): the host side of redundancy.hip.hpp's kernel -- the row tables
// beside FreedomAnalysis' component tables, the LANE / TEAM launch and the two entry points of the C ABI.
#include "host_stage.hpp"

#include "redundancy.hip.hpp"

using namespace ezpz;

namespace {

struct RedundancyPlan {
    bool built = false;
    // [with conflict groups]: workspace doubles of the largest component in the LANE and in the TEAM layout
    uint32_t ws_lane[2] = {1, 1}, ws_team[2] = {1, 1};
    DevBuf<uint32_t> lists;  // comp_row0 | comp_rows | row_int | row_con | con_row0 | focus_of
    uint32_t o_rows = 0, o_row_int = 0, o_row_con = 0, o_con_row0 = 0, o_focus_of = 0;
    DevBuf<double> row_w;
    // what the launches of this entry share -- which is why they run one behind the other, whatever their streams (`focus.done`)
    KeptList focus;
    DevBuf<double> x_int, jv, r, gws;
    DevBuf<uint8_t> row_status;
    DevBuf<unsigned char> host_stage;  // the host entry's staging (host_stage.hpp)
};

RedundancyPlan& plan_of(EzpzSystem* sys) {
    if (!sys->redundancy) sys->redundancy = std::make_shared<RedundancyPlan>();
    return *static_cast<RedundancyPlan*>(sys->redundancy.get());
}

// Each component's caller rows (ascending = request order, as build_freedom numbers them), row -> constraint position, row weight.
int build_redundancy(EzpzSystem* sys, RedundancyPlan& R) {
    if (R.built) return EZPZ_OK;
    const auto& F = sys->freedom;
    const uint32_t m = sys->counts.n_rows, n_cs = (uint32_t)sys->host_cs.size();
    std::vector<uint32_t> con_row0(n_cs + 1, 0), row_con(std::max<uint32_t>(m, 1), 0), row_int(std::max<uint32_t>(m, 1), 0);
    std::vector<double> row_w(std::max<uint32_t>(m, 1), 1.0);
    for (uint32_t c = 0; c < n_cs; ++c) {
        const EzpzConstraint& k = sys->host_cs[c];
        if (k.kind >= 25) return EZPZ_ERR_INVALID_ARGUMENT;
        con_row0[c + 1] = con_row0[c] + kKinds[k.kind].n_rows;
        if (con_row0[c + 1] > m) return EZPZ_ERR_INVALID_ARGUMENT;
        for (uint32_t row = con_row0[c]; row < con_row0[c + 1]; ++row) {
            row_con[row] = c;
            row_w[row] = k.weight;
        }
    }
    if (con_row0[n_cs] != m || sys->host_row_of.size() != m) return EZPZ_ERR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < m; ++k) row_int[sys->host_row_of[k]] = k;
    std::vector<uint32_t> comp_row0(std::max<size_t>(F.host_comps.size(), 1), 0);
    uint32_t total = 0;
    for (size_t c = 0; c < F.host_comps.size(); ++c) {
        comp_row0[c] = total;
        total += F.host_comps[c].m;
    }
    std::vector<uint32_t> comp_rows(std::max<uint32_t>(total, 1), 0);
    for (size_t c = 0; c < F.host_comps.size(); ++c) {
        const FreedomComp& k = F.host_comps[c];
        for (uint32_t it = k.item0; it < k.item1; ++it)
            comp_rows[comp_row0[c] + F.host_items[2 * it + 1] % k.m] = sys->host_slot_row[F.host_items[2 * it]];
        for (int with_l = 0; with_l < 2; ++with_l) {
            const uint64_t lane = redundancy::component_ws(k.m, k.n, false, with_l), team = redundancy::component_ws(k.m, k.n, true, with_l);
            if (team > (1ull << 31)) return EZPZ_ERR_TOO_LARGE;
            R.ws_lane[with_l] = std::max(R.ws_lane[with_l], (uint32_t)lane);
            R.ws_team[with_l] = std::max(R.ws_team[with_l], (uint32_t)team);
        }
    }
    std::vector<uint32_t> lists(comp_row0);
    R.o_rows = (uint32_t)lists.size();
    lists.insert(lists.end(), comp_rows.begin(), comp_rows.end());
    R.o_row_int = (uint32_t)lists.size();
    lists.insert(lists.end(), row_int.begin(), row_int.end());
    R.o_row_con = (uint32_t)lists.size();
    lists.insert(lists.end(), row_con.begin(), row_con.end());
    R.o_con_row0 = (uint32_t)lists.size();
    lists.insert(lists.end(), con_row0.begin(), con_row0.end());
    R.o_focus_of = (uint32_t)lists.size();
    lists.insert(lists.end(), std::max<uint32_t>(n_cs, 1), kNoFocus);
    int rc;
    if ((rc = R.lists.ensure(lists.size())) != EZPZ_OK) return rc;
    if ((rc = R.row_w.ensure(row_w.size())) != EZPZ_OK) return rc;
    HIP_TRY(hipMemcpy(R.lists.p, lists.data(), lists.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(R.row_w.p, row_w.data(), row_w.size() * sizeof(double), hipMemcpyHostToDevice));
    R.built = true;
    return EZPZ_OK;
}

bool config_ok(const EzpzRedundancyConfig& c) {
    for (double t : {c.rank_tol, c.conflict_tol, c.group_tol})
        if (!(t >= 0.0) || !std::isfinite(t)) return false;
    return true;
}

// The argument errors of both entries: nothing is enqueued and no output touched when this fails.
int check_request(const EzpzSystem* sys, const double* x, size_t batch, const EzpzRedundancyConfig* cfg, const uint8_t* con_status,
                  const uint32_t* focus, size_t n_focus, const uint8_t* group) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    if (cfg && !config_ok(*cfg)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch && (!x || !con_status)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (n_focus) {
        if (!focus || !group) return EZPZ_ERR_INVALID_ARGUMENT;
        const size_t n_cs = sys->host_cs.size();
        std::vector<uint8_t> seen(n_cs, 0);
        for (size_t k = 0; k < n_focus; ++k) {
            if (focus[k] >= n_cs || seen[focus[k]]) return EZPZ_ERR_INVALID_ARGUMENT;
            seen[focus[k]] = 1;
        }
    }
    return EZPZ_OK;
}

// Everything on `stream`; `focus` is host memory.  The caller holds sys->mu (as FreedomAnalysis does: the component tables are shared with it) and has checked the request.
int redundancy_device(EzpzSystem* sys, const double* x_dev, size_t batch, const EzpzRedundancyConfig& cfg, uint8_t* con_status_dev,
                      uint8_t* row_status_dev, uint32_t* rank_dev, const uint32_t* focus, size_t n_focus, uint8_t* group_dev,
                      hipStream_t stream) {
    release_thread_kernel(sys->device);
    int rc = ensure_program(sys);
    if (rc != EZPZ_OK) return rc;
    const size_t n = sys->counts.n_vars, zj = sys->counts.zj, m = sys->counts.n_rows, n_cs = sys->host_cs.size();
    if (n == 0 || m == 0) return EZPZ_ERR_EMPTY_SYSTEM;
    if ((rc = build_freedom(sys)) != EZPZ_OK) return rc;
    RedundancyPlan& R = plan_of(sys);
    bool blocked = !R.built;
    if ((rc = build_redundancy(sys, R)) != EZPZ_OK) return rc;
    const auto& F = sys->freedom;
    const bool with_l = n_focus != 0;
    // the focus table changes only behind the last launch that read it
    if (!R.focus.same(focus, n_focus)) {
        if ((rc = R.focus.before_overwrite()) != EZPZ_OK) return rc;
        std::vector<uint32_t> focus_of(std::max<size_t>(n_cs, 1), kNoFocus);
        for (size_t k = 0; k < n_focus; ++k) focus_of[focus[k]] = (uint32_t)k;
        HIP_TRY(hipMemcpy(R.lists.p + R.o_focus_of, focus_of.data(), focus_of.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        R.focus.keep(focus, n_focus);
        blocked = true;
    }
    // placement: LANE while the largest component's private workspace is at most 64 doubles, else TEAM with the workspace in LDS
    // (up to 128 KiB) or in global memory (at most 1024 workgroups and 4 GiB)
    const bool lane = R.ws_lane[with_l] <= 64;
    const uint32_t ws = lane ? R.ws_lane[with_l] : R.ws_team[with_l];
    const uint32_t threads = lane ? 128 : F.max_n > 64 ? 1024 : 256;
    const uint32_t group_sz = !lane ? 1 : F.ncomp >= 128 ? 1 : 128 / std::max<uint32_t>(F.ncomp, 1);
    const size_t head = ((size_t)(group_sz + 1) / 2 + 16) * sizeof(double);
    size_t lds = head + (size_t)(lane ? threads : 1) * ws * sizeof(double);
    uint32_t grid = (uint32_t)std::min<size_t>((batch + group_sz - 1) / group_sz, 1u << 16);
    bool global_ws = false;
    if (!lane && lds > 128 * 1024) {
        global_ws = true;
        lds = head;
        const size_t per = (size_t)ws * sizeof(double);
        grid = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(batch, 1024), (4ull << 30) / per));
    }
    // Whatever can fail is done before the first launch (a growing buffer is replaced behind the last launch that used it).
    const size_t need_x = batch * n, need_jv = batch * std::max<size_t>(zj, 1), need_r = batch * m, need_gws = global_ws ? (size_t)grid * ws : 0;
    const size_t need_rows = row_status_dev ? 0 : batch * m;
    if (need_x > R.x_int.cap || need_jv > R.jv.cap || need_r > R.r.cap || need_gws > R.gws.cap || need_rows > R.row_status.cap) {
        if ((rc = R.focus.before_overwrite()) != EZPZ_OK) return rc;
        blocked = true;
    }
    if ((rc = R.x_int.ensure(need_x)) != EZPZ_OK) return rc;
    if ((rc = R.jv.ensure(need_jv)) != EZPZ_OK) return rc;
    if ((rc = R.r.ensure(need_r)) != EZPZ_OK) return rc;
    if ((rc = R.gws.ensure(need_gws)) != EZPZ_OK) return rc;
    if ((rc = R.row_status.ensure(need_rows)) != EZPZ_OK) return rc;
    static std::atomic<size_t> raised[2][16];  // (the attribute belongs to the kernel: raised once per device and size)
    if (raised[lane][sys->device & 15].load(std::memory_order_relaxed) < lds) {
        HIP_TRY(hipFuncSetAttribute(lane ? (const void*)redundancy_kernel<true> : (const void*)redundancy_kernel<false>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        raised[lane][sys->device & 15].store(lds, std::memory_order_relaxed);
    }
    if (blocked) call_stamp(REDUNDANCY_PREPARED);
    if ((rc = R.focus.order_behind(stream)) != EZPZ_OK) return rc;
    const uint32_t* var_of = reinterpret_cast<const uint32_t*>(sys->view.base + sys->view.o_var_of);
    const uint64_t total = (uint64_t)batch * n;
    hipLaunchKernelGGL(rd_gather_kernel, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 65536)), dim3(256), 0, stream, x_dev,
                       var_of, R.x_int.p, (uint32_t)n, total);
    launch_eval(sys, R.x_int.p, batch, R.r.p, R.jv.p, nullptr, (uint32_t)std::min<size_t>(batch, 8192), stream);
    RedundancyArgs a{};
    a.jv = R.jv.p;
    a.r = R.r.p;
    a.comps = F.comps.p;
    a.items = F.lists.p;
    a.comp_row0 = R.lists.p;
    a.comp_rows = R.lists.p + R.o_rows;
    a.row_int = R.lists.p + R.o_row_int;
    a.row_con = R.lists.p + R.o_row_con;
    a.con_row0 = R.lists.p + R.o_con_row0;
    a.row_w = R.row_w.p;
    a.focus_of = with_l ? R.lists.p + R.o_focus_of : nullptr;
    a.con_status = con_status_dev;
    a.row_status = row_status_dev ? row_status_dev : R.row_status.p;
    a.rank = rank_dev;
    a.group = with_l ? group_dev : nullptr;
    a.gws = global_ws ? R.gws.p : nullptr;
    a.batch = batch;
    a.n_rows = (uint32_t)m;
    a.n_cs = (uint32_t)n_cs;
    a.zj = (uint32_t)zj;
    a.ncomp = F.ncomp;
    a.n_focus = (uint32_t)n_focus;
    a.ws = ws;
    a.group_sz = group_sz;
    a.rank_tol = cfg.rank_tol;
    a.conflict_tol = cfg.conflict_tol;
    a.group_tol = cfg.group_tol;
    if (lane)
        hipLaunchKernelGGL(redundancy_kernel<true>, dim3(grid), dim3(threads), lds, stream, a);
    else
        hipLaunchKernelGGL(redundancy_kernel<false>, dim3(grid), dim3(threads), lds, stream, a);
    HIP_TRY(hipGetLastError());
    call_stamp(REDUNDANCY_LAUNCHED);
    call_stamp(lane ? REDUNDANCY_PLACED_LANE : global_ws ? REDUNDANCY_PLACED_TEAM_GLOBAL : REDUNDANCY_PLACED_TEAM_LDS);
    return R.focus.record(stream);
}

}  // namespace

extern "C" {

void ezpz_default_redundancy_config(EzpzRedundancyConfig* cfg) {
    if (!cfg) return;
    cfg->rank_tol = 1e-6;
    cfg->conflict_tol = 1e-4;
    cfg->group_tol = 1e-6;
}

int ezpz_system_redundancy_device(EzpzSystem* sys, const double* x_dev, size_t batch, const EzpzRedundancyConfig* cfg,
                                  uint8_t* con_status_dev, uint8_t* row_status_dev, uint32_t* rank_dev, const uint32_t* focus,
                                  size_t n_focus, uint8_t* group_dev, void* stream) {
    if (int rc = check_request(sys, x_dev, batch, cfg, con_status_dev, focus, n_focus, group_dev)) return rc;
    if (batch == 0) return EZPZ_OK;
    EzpzRedundancyConfig c;
    ezpz_default_redundancy_config(&c);
    if (cfg) c = *cfg;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    return redundancy_device(sys, x_dev, batch, c, con_status_dev, row_status_dev, rank_dev, focus, n_focus, group_dev, (hipStream_t)stream);
}

int ezpz_system_redundancy(EzpzSystem* sys, const double* x, size_t batch, const EzpzRedundancyConfig* cfg, uint8_t* con_status,
                           uint8_t* row_status, uint32_t* rank, const uint32_t* focus, size_t n_focus, uint8_t* group) {
    if (int rc = check_request(sys, x, batch, cfg, con_status, focus, n_focus, group)) return rc;
    if (batch == 0) return EZPZ_OK;
    EzpzRedundancyConfig c;
    ezpz_default_redundancy_config(&c);
    if (cfg) c = *cfg;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    const size_t n = sys->counts.n_vars, m = sys->counts.n_rows, n_cs = sys->host_cs.size();
    if (n == 0 || m == 0) return EZPZ_ERR_EMPTY_SYSTEM;
    RedundancyPlan& R = plan_of(sys);
    const double* x_dev;
    uint8_t *con_dev, *row_dev, *group_dev;
    uint32_t* rank_dev;
    Staged io;
    io.in(x, batch * n, x_dev);
    io.out(con_status, batch * n_cs, con_dev);
    io.out(row_status, batch * m, row_dev);
    io.out(rank, batch, rank_dev);
    io.out(group, batch * n_focus * n_cs, group_dev);
    int rc;
    if ((rc = io.reserve(R.host_stage)) != EZPZ_OK || (rc = io.upload(R.host_stage)) != EZPZ_OK) return rc;
    if ((rc = redundancy_device(sys, x_dev, batch, c, con_dev, row_dev, rank_dev, focus, n_focus, group_dev, nullptr)) != EZPZ_OK) return rc;
    return io.copy_back(R.host_stage);  // (blocking copies on the null stream: they wait for its launch)
}

}  // extern "C"
