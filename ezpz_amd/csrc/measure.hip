// Reference dimensions (include/ezpz_amd.h: ezpz_constraint_measure, ezpz_system_measure, _measure_response, _measure_vjp and
// their _device forms): the host side of measure.hip.hpp's kernels -- the plan a system keeps for the last call's
// record list (a KeptRecords, its packed table and CSR on the device, the gradient workspace, the host entries' staging), the
// ROW / DIRECT launch, and the entry points of the C ABI.  The check of a list and its tables are in measure_tables.hpp.
#include "host_stage.hpp"

#include "measure.hip.hpp"
#include "measure_tables.hpp"

using namespace ezpz;

namespace {

static_assert(kMeasRecWords == kMeasureRecWords, "the kernels read the table measure_pack_records writes");

struct MeasurePlan {
    // what the launches of these entries share -- which is why they run one behind the other, whatever their streams (`list.done`)
    KeptRecords list;
    DevBuf<uint32_t> table, csr;
    bool csr_valid = false;  // `csr` is the kept list's (built when a vjp first asks for it)
    DevBuf<double> gws;      // [batch][n_meas][8]: the gradients of a response's or a vjp's first launch
    DevBuf<unsigned char> host_stage;  // the host entries' staging (host_stage.hpp)
};

MeasurePlan& plan_of(EzpzSystem* sys) {
    if (!sys->measure) sys->measure = std::make_shared<MeasurePlan>();
    return *static_cast<MeasurePlan*>(sys->measure.get());
}

// EZPZ_MEASURE_ROUTE=row | direct: the placement whatever the threshold (read per call: a test or tools/measure_rate.py switches it)
enum ForcedRoute { ROUTE_AUTO, ROUTE_ROW, ROUTE_DIRECT };
ForcedRoute forced_route() {
    const char* e = std::getenv("EZPZ_MEASURE_ROUTE");
    if (e && !std::strcmp(e, "row")) return ROUTE_ROW;
    if (e && !std::strcmp(e, "direct")) return ROUTE_DIRECT;
    return ROUTE_AUTO;
}

// The tables of `words` on the device (the caller holds sys->mu).  Whatever overwrites something a launch may still read waits for
// the last launch first; a caller that repeats its list finds everything in place and only enqueues.
int prepare(MeasurePlan& P, std::vector<uint32_t>&& words, size_t n_vars, bool need_csr, size_t gws_doubles) {
    int rc;
    bool blocked = false;
    if (!P.list.same(words)) {
        if ((rc = P.list.before_overwrite()) != EZPZ_OK) return rc;
        P.list.valid = false;
        P.csr_valid = false;
        if ((rc = P.table.ensure(words.size())) != EZPZ_OK) return rc;
        HIP_TRY(hipMemcpy(P.table.p, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        P.list.keep(std::move(words));
        blocked = true;
    }
    if (need_csr && !P.csr_valid) {
        if ((rc = P.list.before_overwrite()) != EZPZ_OK) return rc;
        std::vector<uint32_t> csr;
        measure_build_csr(P.list.words, n_vars, csr);
        if ((rc = P.csr.ensure(csr.size())) != EZPZ_OK) return rc;
        HIP_TRY(hipMemcpy(P.csr.p, csr.data(), csr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        P.csr_valid = true;
        blocked = true;
    }
    if (gws_doubles > P.gws.cap) {
        if ((rc = P.list.before_overwrite()) != EZPZ_OK) return rc;
        if ((rc = P.gws.ensure(gws_doubles)) != EZPZ_OK) return rc;
        blocked = true;
    }
    if (blocked) call_stamp(MEASURE_TABLE_UPLOADED);
    return EZPZ_OK;
}

uint32_t stride_grid(uint64_t items, const EzpzSystem* sys, uint32_t per_cu) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, (uint64_t)sys->lim.cus * per_cu));
}

// m / flags / grad (each optional) of the kept list at x: ROW while a row fits the LDS and the policy says so, DIRECT otherwise.
int launch_measure(EzpzSystem* sys, MeasurePlan& P, const double* x_dev, size_t batch, double* m_dev, uint8_t* flags_dev,
                   double* grad_dev, hipStream_t stream) {
    MeasureArgs a{};
    a.x = x_dev;
    a.table = P.table.p;
    a.m = m_dev;
    a.flags = flags_dev;
    a.grad = grad_dev;
    a.batch = batch;
    a.n_vars = (uint32_t)sys->counts.n_vars;
    a.n_meas = (uint32_t)(P.list.words.size() / kMeasRecWords);
    a.grad16 = (reinterpret_cast<uintptr_t>(grad_dev) & 15) == 0;
    const ForcedRoute forced = forced_route();
    const uint32_t row_from = forced == ROUTE_ROW ? 0 : kMeasureRowMinVars;
    const uint32_t row_limit = forced == ROUTE_ROW ? kMeasureRowLdsMaxVars : forced == ROUTE_DIRECT ? 0 : kMeasureRowMaxVars;
    // (the ROW kernel pairs doubles by the parity of their index: x has to be 16-byte aligned)
    const bool row = a.n_vars >= row_from && a.n_vars <= row_limit && (reinterpret_cast<uintptr_t>(x_dev) & 15) == 0;
    if (row) {
        // systems per workgroup: what the LDS budget holds, no more than gives the lanes a measurement each and leaves the device
        // some four workgroups per CU
        const uint64_t fit = std::max<uint32_t>(kMeasureRowGroupDoubles / std::max<uint32_t>(a.n_vars, 1), 1);
        const uint64_t want = std::max<uint64_t>((256 + a.n_meas - 1) / a.n_meas, batch / ((uint64_t)sys->lim.cus * 4));
        a.group = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(fit, std::max<uint64_t>(want, 1)), std::min<uint64_t>(batch, 256));
        const size_t row_bytes = (((size_t)a.group * a.n_vars + 3) & ~(size_t)1) * sizeof(double);
        const size_t table_bytes = (size_t)a.n_meas * kMeasRecWords * sizeof(uint32_t);
        a.table_in_lds = table_bytes <= kMeasureTableLdsBytes && row_bytes + table_bytes <= 64 * 1024;
        const size_t lds = row_bytes + (a.table_in_lds ? table_bytes : 0);
        const uint64_t groups = (batch + a.group - 1) / a.group;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(groups, (uint64_t)sys->lim.cus * 16);
        hipLaunchKernelGGL(measure_row_kernel, dim3(grid), dim3(256), lds, stream, a);
    } else {
        hipLaunchKernelGGL(measure_direct_kernel, dim3(stride_grid((uint64_t)batch * a.n_meas, sys, 16)), dim3(256), 0, stream, a);
    }
    HIP_TRY(hipGetLastError());
    call_stamp(row ? MEASURE_PLACED_ROW : MEASURE_PLACED_DIRECT);
    return EZPZ_OK;
}

// ---- the argument errors: nothing is enqueued and no output touched when one of these fails ---------------------------------
int check_list(const EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, std::vector<uint32_t>& words) {
    if (!sys) return EZPZ_ERR_INVALID_ARGUMENT;
    return measure_pack_records(records, n_meas, sys->counts.n_vars, words);
}

int check_measure(const EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x, size_t batch, const double* m_out,
                  std::vector<uint32_t>& words) {
    if (int rc = check_list(sys, records, n_meas, words)) return rc;
    if (batch && n_meas && (!x || !m_out)) return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

int check_response(const EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x, const double* S, size_t n_param,
                   size_t batch, const double* tol, const double* D_out, const double* worst_out, const double* rss_out,
                   std::vector<uint32_t>& words) {
    if (int rc = check_list(sys, records, n_meas, words)) return rc;
    if ((worst_out != nullptr) != (rss_out != nullptr) || (worst_out && !tol)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch && n_meas && n_param && (!x || !S || !D_out)) return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

int check_vjp(const EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x, const double* grad_m, size_t batch,
              const double* grad_x_out, std::vector<uint32_t>& words) {
    if (int rc = check_list(sys, records, n_meas, words)) return rc;
    if (batch && n_meas && (!x || !grad_m || !grad_x_out)) return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

// ---- the device forms' bodies: everything on `stream`; the caller holds sys->mu, the system's device is current, the request is
// checked and not empty ----------------------------------------------------------------------------------------------------------
int measure_device(EzpzSystem* sys, std::vector<uint32_t>&& words, const double* x_dev, size_t batch, double* m_dev, uint8_t* flags_dev,
                   double* grad_dev, hipStream_t stream) {
    release_thread_kernel(sys->device);
    MeasurePlan& P = plan_of(sys);
    int rc;
    if ((rc = prepare(P, std::move(words), sys->counts.n_vars, false, 0)) != EZPZ_OK) return rc;
    if ((rc = P.list.order_behind(stream)) != EZPZ_OK) return rc;
    if ((rc = launch_measure(sys, P, x_dev, batch, m_dev, flags_dev, grad_dev, stream)) != EZPZ_OK) return rc;
    call_stamp(MEASURE_LAUNCHED);
    return P.list.record(stream);
}

int response_device(EzpzSystem* sys, std::vector<uint32_t>&& words, const double* x_dev, const double* S_dev, size_t n_param, size_t batch,
                    const double* tol_dev, double* D_dev, double* worst_dev, double* rss_dev, hipStream_t stream) {
    release_thread_kernel(sys->device);
    MeasurePlan& P = plan_of(sys);
    const size_t n_meas = words.size() / kMeasRecWords;
    int rc;
    if ((rc = prepare(P, std::move(words), sys->counts.n_vars, false, batch * n_meas * 8)) != EZPZ_OK) return rc;
    if ((rc = P.list.order_behind(stream)) != EZPZ_OK) return rc;
    if ((rc = launch_measure(sys, P, x_dev, batch, nullptr, nullptr, P.gws.p, stream)) != EZPZ_OK) return rc;
    ResponseArgs a{};
    a.table = P.table.p;
    a.grad = P.gws.p;
    a.S = S_dev;
    a.tol = tol_dev;
    a.D = D_dev;
    a.worst = worst_dev;
    a.rss = rss_dev;
    a.batch = batch;
    a.n_vars = (uint32_t)sys->counts.n_vars;
    a.n_meas = (uint32_t)n_meas;
    a.n_param = (uint32_t)n_param;
    hipLaunchKernelGGL(response_kernel, dim3(stride_grid((uint64_t)batch * n_meas * n_param, sys, 16)), dim3(256), 0, stream, a);
    if (worst_dev) hipLaunchKernelGGL(stackup_kernel, dim3(stride_grid((uint64_t)batch * n_meas, sys, 16)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    call_stamp(MEASURE_LAUNCHED);
    return P.list.record(stream);
}

int vjp_device(EzpzSystem* sys, std::vector<uint32_t>&& words, const double* x_dev, const double* grad_m_dev, size_t batch,
               double* grad_x_dev, hipStream_t stream) {
    release_thread_kernel(sys->device);
    MeasurePlan& P = plan_of(sys);
    const size_t n_meas = words.size() / kMeasRecWords, n = sys->counts.n_vars;
    int rc;
    if ((rc = prepare(P, std::move(words), n, true, batch * n_meas * 8)) != EZPZ_OK) return rc;
    if ((rc = P.list.order_behind(stream)) != EZPZ_OK) return rc;
    if ((rc = launch_measure(sys, P, x_dev, batch, nullptr, nullptr, P.gws.p, stream)) != EZPZ_OK) return rc;
    VjpArgs a{};
    a.grad = P.gws.p;
    a.grad_m = grad_m_dev;
    a.csr = P.csr.p;
    a.grad_x = grad_x_dev;
    a.batch = batch;
    a.n_vars = (uint32_t)n;
    a.n_meas = (uint32_t)n_meas;
    hipLaunchKernelGGL(vjp_sum_kernel, dim3(stride_grid((uint64_t)batch * n, sys, 16)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    call_stamp(MEASURE_LAUNCHED);
    return P.list.record(stream);
}

}  // namespace

extern "C" {

int ezpz_constraint_measure(const EzpzConstraint* c, const double* x, double* m_out, double grad_out[8], int* flags) {
    return constraint_measure_host(c, x, m_out, grad_out, flags);
}

int ezpz_system_measure_device(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x_dev, size_t batch,
                               double* m_out_dev, uint8_t* flags_out_dev, double* grad_out_dev, void* stream) {
    std::vector<uint32_t> words;
    if (int rc = check_measure(sys, records, n_meas, x_dev, batch, m_out_dev, words)) return rc;
    if (batch == 0 || n_meas == 0) return EZPZ_OK;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    return measure_device(sys, std::move(words), x_dev, batch, m_out_dev, flags_out_dev, grad_out_dev, (hipStream_t)stream);
}

int ezpz_system_measure(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x, size_t batch, double* m_out,
                        uint8_t* flags_out, double* grad_out) {
    std::vector<uint32_t> words;
    if (int rc = check_measure(sys, records, n_meas, x, batch, m_out, words)) return rc;
    if (batch == 0 || n_meas == 0) return EZPZ_OK;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    MeasurePlan& P = plan_of(sys);
    const size_t n = sys->counts.n_vars, out = batch * n_meas;
    const double* x_dev;
    double *m_dev, *grad_dev;
    uint8_t* flags_dev;
    Staged io;
    io.in(x, batch * n, x_dev);
    io.out(m_out, out, m_dev);
    io.out(flags_out, out, flags_dev);
    io.out(grad_out, out * 8, grad_dev);
    int rc;
    if ((rc = io.reserve(P.host_stage)) != EZPZ_OK || (rc = io.upload(P.host_stage)) != EZPZ_OK) return rc;
    if ((rc = measure_device(sys, std::move(words), x_dev, batch, m_dev, flags_dev, grad_dev, nullptr)) != EZPZ_OK) return rc;
    return io.copy_back(P.host_stage);  // (blocking copies on the null stream: they wait for its launches)
}

int ezpz_system_measure_response_device(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x_dev,
                                        const double* S_dev, size_t n_param, size_t batch, const double* tol_dev, double* D_out_dev,
                                        double* worst_out_dev, double* rss_out_dev, void* stream) {
    std::vector<uint32_t> words;
    if (int rc = check_response(sys, records, n_meas, x_dev, S_dev, n_param, batch, tol_dev, D_out_dev, worst_out_dev, rss_out_dev, words))
        return rc;
    if (batch == 0 || n_meas == 0 || n_param == 0) return EZPZ_OK;
    if (n_param > 0xFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    return response_device(sys, std::move(words), x_dev, S_dev, n_param, batch, tol_dev, D_out_dev, worst_out_dev, rss_out_dev,
                           (hipStream_t)stream);
}

int ezpz_system_measure_response(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x, const double* S,
                                 size_t n_param, size_t batch, const double* tol, double* D_out, double* worst_out, double* rss_out) {
    std::vector<uint32_t> words;
    if (int rc = check_response(sys, records, n_meas, x, S, n_param, batch, tol, D_out, worst_out, rss_out, words)) return rc;
    if (tol)
        for (size_t j = 0; j < n_param; ++j)
            if (!(tol[j] >= 0.0) || !std::isfinite(tol[j])) return EZPZ_ERR_INVALID_ARGUMENT;
    if (batch == 0 || n_meas == 0 || n_param == 0) return EZPZ_OK;
    if (n_param > 0xFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    MeasurePlan& P = plan_of(sys);
    const size_t n = sys->counts.n_vars, out = batch * n_meas;
    const double *x_dev, *S_dev, *tol_dev;
    double *D_dev, *worst_dev, *rss_dev;
    Staged io;
    io.in(x, batch * n, x_dev);
    io.in(S, batch * n_param * n, S_dev);
    io.in(tol, n_param, tol_dev);
    io.out(D_out, out * n_param, D_dev);
    io.out(worst_out, out, worst_dev);  // (both or neither: check_response)
    io.out(rss_out, out, rss_dev);
    int rc;
    if ((rc = io.reserve(P.host_stage)) != EZPZ_OK || (rc = io.upload(P.host_stage)) != EZPZ_OK) return rc;
    if ((rc = response_device(sys, std::move(words), x_dev, S_dev, n_param, batch, tol_dev, D_dev, worst_dev, rss_dev, nullptr)) != EZPZ_OK)
        return rc;
    return io.copy_back(P.host_stage);
}

int ezpz_system_measure_vjp_device(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x_dev,
                                   const double* grad_m_dev, size_t batch, double* grad_x_out_dev, void* stream) {
    std::vector<uint32_t> words;
    if (int rc = check_vjp(sys, records, n_meas, x_dev, grad_m_dev, batch, grad_x_out_dev, words)) return rc;
    if (batch == 0 || n_meas == 0) return EZPZ_OK;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    return vjp_device(sys, std::move(words), x_dev, grad_m_dev, batch, grad_x_out_dev, (hipStream_t)stream);
}

int ezpz_system_measure_vjp(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x, const double* grad_m,
                            size_t batch, double* grad_x_out) {
    std::vector<uint32_t> words;
    if (int rc = check_vjp(sys, records, n_meas, x, grad_m, batch, grad_x_out, words)) return rc;
    if (batch == 0 || n_meas == 0) return EZPZ_OK;
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    MeasurePlan& P = plan_of(sys);
    const size_t n = sys->counts.n_vars;
    const double *x_dev, *gm_dev;
    double* gx_dev;
    Staged io;
    io.in(x, batch * n, x_dev);
    io.in(grad_m, batch * n_meas, gm_dev);
    io.out(grad_x_out, batch * n, gx_dev);
    int rc;
    if ((rc = io.reserve(P.host_stage)) != EZPZ_OK || (rc = io.upload(P.host_stage)) != EZPZ_OK) return rc;
    if ((rc = vjp_device(sys, std::move(words), x_dev, gm_dev, batch, gx_dev, nullptr)) != EZPZ_OK) return rc;
    return io.copy_back(P.host_stage);
}

}  // extern "C"
