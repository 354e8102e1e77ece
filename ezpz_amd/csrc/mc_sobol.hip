// Sobol tolerance indices (include/ezpz_amd.h: ezpz_mc_sobol_indices, ezpz_mc_sobol_sums and its _device form): the
// host side of mc_sobol.hip.hpp -- the two host entries (plain C++, no device), the reduction's workspace and launches (shared with
// the run, ezpz_system_tolerance_sobol in tolerance_mc.hip) and the reduction alone on a caller's rows, on a workspace the process
// owns per device.
#define EZPZ_SOBOL_KERNELS
#include "mc_sobol.hip.hpp"

using namespace ezpz;

namespace ezpz {
namespace sobol {

static_assert(sizeof(EzpzSobolConfig) == 16, "the layout include/ezpz_amd.h documents");

int enqueue_sums(mcb::Work& work, SumArgs a, hipStream_t stream) {
    a.part = work.part.p;
    a.part_n = work.part_n.p;
    a.ticket = work.ticket.p;
    const uint32_t blocks = (uint32_t)((a.count + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(mc_sobol_kernel, dim3(blocks), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

int enqueue_ok(const EzpzStatus* status, uint64_t count, uint8_t* ok, hipStream_t stream) {
    hipLaunchKernelGGL(mc_sobol_ok_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, stream, status, count, ok);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

int enqueue_close(const CloseArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(mc_sobol_close_kernel, dim3(1), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

}  // namespace sobol
}  // namespace ezpz

using namespace ezpz::sobol;

namespace {
struct SumWork : mcb::Work {};  // (a type of its own: the process keeps a plan per type)
}

extern "C" {

void ezpz_default_sobol_config(EzpzSobolConfig* c) {
    if (c) default_config(c);
}

int ezpz_mc_sobol_indices(const double* sums, const uint64_t* n_complete, size_t n_param, size_t n_meas, double* var, double* first,
                          double* total, double* first_var, double* total_var) {
    return indices_host(sums, n_complete, n_param, n_meas, var, first, total, first_var, total_var);
}

int ezpz_mc_sobol_sums(const double* f, const uint8_t* flags, const uint8_t* ok, const double* nominal_m, uint32_t fixed_mask,
                       uint64_t samples, size_t n_param, size_t n_meas, uint32_t chunk, double* sums, uint64_t* n_complete) {
    (void)chunk;  // (the host form has no rounds; the sums' bits do not depend on them)
    return sums_host(f, flags, ok, nominal_m, fixed_mask, samples, n_param, n_meas, sums, n_complete);
}

int ezpz_mc_sobol_sums_device(const double* f_dev, const uint8_t* flags_dev, const uint8_t* ok_dev, const double* nominal_m_dev,
                              uint32_t fixed_mask, uint64_t samples, size_t n_param, size_t n_meas, uint32_t chunk_in, double* sums_dev,
                              uint64_t* n_complete_dev, void* stream_) {
    if (int rc = check_shape(n_param, n_meas)) return rc;
    if (int rc = check_mask(fixed_mask, n_param)) return rc;
    if (samples && (!sums_dev || !n_complete_dev || !f_dev || !nominal_m_dev)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (samples > 0xFFFFFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    if (samples == 0) return EZPZ_OK;
    const uint64_t chunk = round_chunk(chunk_in ? chunk_in : kDefaultSampleChunk, samples, kBlock);
    hipStream_t stream = (hipStream_t)stream_;
    const uint32_t k = (uint32_t)n_param, m = (uint32_t)n_meas;
    return mcb::on_process_plan<SumWork>(stream, SOBOL_WORKSPACE_GROWN, SOBOL_LAUNCHED, [&](mcb::ProcessPlan<SumWork>& P) {
        SumArgs a{};
        a.nominal_m = nominal_m_dev;
        a.stride_s = (uint64_t)(k + 2) * m, a.stride_r = m;
        a.ok_stride_s = k + 2, a.ok_stride_r = 1;
        a.k = k, a.m = m, a.fixed_mask = fixed_mask;
        a.sums = sums_dev;
        a.n_complete = n_complete_dev;
        for (uint64_t first = 0; first < samples; first += chunk) {
            a.f = f_dev + first * a.stride_s;
            a.flags = flags_dev ? flags_dev + first * a.stride_s : nullptr;
            a.ok = ok_dev ? ok_dev + first * a.ok_stride_s : nullptr;
            a.count = std::min<uint64_t>(chunk, samples - first);
            a.first_round = first == 0;
            if (int rc = enqueue_sums(P.work, a, stream)) return rc;
        }
        return (int)EZPZ_OK;
    }, chunk / kBlock * m * width_of(k), chunk / kBlock * m);
}

}  // extern "C"
