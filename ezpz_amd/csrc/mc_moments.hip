// Tolerance contributors (include/ezpz_amd.h: ezpz_mc_contributors, ezpz_mc_moments and its _device form): the host
// side of mc_moments.hip.hpp -- the checks, the closing step's host entry, the reduction's workspace and launches (shared with the
// run, ezpz_system_tolerance_mc_contrib in tolerance_mc.hip) and the reduction alone on a caller's samples, on a workspace the
// process owns per device.
#define EZPZ_MCM_KERNELS
#include "host_stage.hpp"
#include "mc_moments.hip.hpp"

using namespace ezpz;

namespace ezpz {
namespace mcm {

static_assert(sizeof(EzpzMcContribConfig) == 16 && sizeof(EzpzMcMomentsInfo) == 16, "the layouts include/ezpz_amd.h documents");

int enqueue_moments(mcb::Work& work, MomentArgs a, hipStream_t stream) {
    a.part = work.part.p;
    a.part_n = work.part_n.p;
    a.ticket = work.ticket.p;
    const uint32_t blocks = (uint32_t)((a.count + 255) / 256), K = a.k + a.n_meas;
    hipLaunchKernelGGL(mc_moments_kernel, dim3(blocks), dim3(256), (size_t)kTile * K * sizeof(double), stream, a);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

int enqueue_contributors(const ContribArgs& a, hipStream_t stream) {
    const size_t lds = ((size_t)a.k * a.k + a.k) * sizeof(double) + (a.k + 7) / 8 * 8;
    hipLaunchKernelGGL(mc_contrib_kernel, dim3(1), dim3(256), lds, stream, a);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

}  // namespace mcm
}  // namespace ezpz

namespace {

using namespace ezpz::mcm;

constexpr uint64_t kBlock = 256;

// ezpz_mc_moments has no system: its workspace is the process's (mcb::ProcessPlan), with the host form's staging beside the sums'
struct MomentWork : mcb::Work {
    DevBuf<unsigned char> host_stage;  // the nominals, the outputs, a round of the samples (host_stage.hpp)
};
using MomentPlan = mcb::ProcessPlan<MomentWork>;

// Every argument error of the reduction alone, before anything is enqueued or written; the pointers are only compared with NULL.
int check_moments(const void* params, const void* m, const void* nominal_p, const void* nominal_m, uint64_t samples, size_t n_param,
                  size_t n_meas, uint32_t chunk_in, const void* moments, const void* info, uint64_t& chunk) {
    if (int rc = check_shape(n_param, n_meas)) return rc;
    if (samples && (!moments || !info || (n_param && (!params || !nominal_p)) || (n_meas && (!m || !nominal_m)))) return EZPZ_ERR_INVALID_ARGUMENT;
    if (samples > 0xFFFFFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    chunk = round_chunk(chunk_in ? chunk_in : kDefaultSampleChunk, samples, kBlock);
    return EZPZ_OK;
}

MomentArgs args_of(const double* nominal_p, const double* nominal_m, uint64_t samples, size_t n_param, size_t n_meas, double* moments,
                   EzpzMcMomentsInfo* info) {
    MomentArgs a{};
    a.nominal_p = nominal_p;
    a.nominal_m = nominal_m;
    a.samples = samples;
    a.k = (uint32_t)n_param;
    a.n_meas = (uint32_t)n_meas;
    a.moments = moments;
    a.info = info;
    return a;
}

}  // namespace

extern "C" {

void ezpz_default_mc_contrib_config(EzpzMcContribConfig* cc) {
    if (cc) default_config(cc);
}

int ezpz_mc_contributors(const double* moments, uint64_t n_complete, size_t n_param, size_t n_meas, const EzpzMcContribConfig* cc,
                         double* cov, double* beta, double* contrib, double* r2, uint64_t* dropped) {
    return contributors_host(moments, n_complete, n_param, n_meas, cc, cov, beta, contrib, r2, dropped);
}

int ezpz_mc_moments_device(const double* params_dev, const double* m_dev, const uint8_t* flags_dev, const uint8_t* ok_dev,
                           const double* nominal_p_dev, const double* nominal_m_dev, uint64_t samples, size_t n_param, size_t n_meas,
                           uint32_t chunk_in, double* moments_dev, EzpzMcMomentsInfo* info_dev, void* stream_) {
    uint64_t chunk = 0;
    if (int rc = check_moments(params_dev, m_dev, nominal_p_dev, nominal_m_dev, samples, n_param, n_meas, chunk_in, moments_dev, info_dev, chunk))
        return rc;
    if (samples == 0) return EZPZ_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const uint64_t blocks = chunk / kBlock;
    return mcb::on_process_plan<MomentWork>(stream, MOMENTS_WORKSPACE_GROWN, MOMENTS_LAUNCHED, [&](MomentPlan& P) {
        MomentArgs a = args_of(nominal_p_dev, nominal_m_dev, samples, n_param, n_meas, moments_dev, info_dev);
        for (uint64_t first = 0; first < samples; first += chunk) {
            a.params = params_dev + first * n_param;
            a.m = m_dev + first * n_meas;
            a.flags = flags_dev ? flags_dev + first * n_meas : nullptr;
            a.ok = ok_dev ? ok_dev + first : nullptr;
            a.first = first;
            a.count = std::min<uint64_t>(chunk, samples - first);
            a.first_round = first == 0;
            if (int rc = enqueue_moments(P.work, a, stream)) return rc;
        }
        return (int)EZPZ_OK;
    }, blocks * entries_of((uint32_t)(n_param + n_meas)), blocks);
}

int ezpz_mc_moments(const double* params, const double* m, const uint8_t* flags, const uint8_t* ok, const double* nominal_p,
                    const double* nominal_m, uint64_t samples, size_t n_param, size_t n_meas, uint32_t chunk_in, double* moments,
                    EzpzMcMomentsInfo* info) {
    uint64_t chunk = 0;
    if (int rc = check_moments(params, m, nominal_p, nominal_m, samples, n_param, n_meas, chunk_in, moments, info, chunk)) return rc;
    if (samples == 0) return EZPZ_OK;
    MomentPlan* P = nullptr;
    int device = -1;
    if (int rc = plan_of_device(P, device)) return rc;
    std::lock_guard<std::mutex> lock(P->mu);
    const uint32_t K = (uint32_t)(n_param + n_meas);
    const hipStream_t stream = hipStreamPerThread;
    int rc;
    // (the buffers of an earlier host call are idle: it waited for its launches)
    MomentWork& W = P->work;
    const uint64_t blocks = chunk / kBlock;
    if (W.grows(blocks * entries_of(K), blocks)) {
        if ((rc = P->order.before_overwrite()) != EZPZ_OK || (rc = W.ensure(blocks * entries_of(K), blocks)) != EZPZ_OK) return rc;
        call_stamp(MOMENTS_WORKSPACE_GROWN);
    }
    if ((rc = P->order.order_behind(stream)) != EZPZ_OK) return rc;
    MomentArgs a = args_of(nullptr, nullptr, samples, n_param, n_meas, nullptr, nullptr);
    Staged io;
    for (uint64_t first = 0; first < samples; first += chunk) {
        const uint64_t count = std::min<uint64_t>(chunk, samples - first);
        if (first) HIP_TRY(hipStreamSynchronize(stream));  // (the last round has read the buffers)
        // The round's list.  What the whole call shares -- the nominals, and the outputs the rounds sum into -- stands in front of the
        // round's samples, so that every round finds it at the same place; round 0 uploads the nominals, the others keep their room.
        io = Staged{};
        first ? io.room(n_param, a.nominal_p) : io.in(nominal_p, n_param, a.nominal_p);
        first ? io.room(n_meas, a.nominal_m) : io.in(nominal_m, n_meas, a.nominal_m);
        io.out(moments, entries_of(K), a.moments);
        io.out(info, 1, a.info);
        io.in(params + first * n_param, count * n_param, a.params);
        io.in(m + first * n_meas, count * n_meas, a.m);
        io.in(flags ? flags + first * n_meas : nullptr, count * n_meas, a.flags);
        io.in(ok ? ok + first : nullptr, count, a.ok);
        if ((rc = io.reserve(W.host_stage)) != EZPZ_OK || (rc = io.upload(W.host_stage)) != EZPZ_OK) return rc;
        a.first = first;
        a.count = count;
        a.first_round = first == 0;
        if ((rc = enqueue_moments(W, a, stream)) != EZPZ_OK) return rc;
    }
    call_stamp(MOMENTS_LAUNCHED);
    if ((rc = P->order.record(stream)) != EZPZ_OK) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return io.copy_back(W.host_stage);
}

}  // extern "C"
