// Monte-Carlo main effects (include/ezpz_amd.h: ezpz_mc_effect_indices, ezpz_mc_effects and its _device form): the
// host side of mc_effects.hip.hpp -- the two host entries (plain C++, no device), the reduction's workspace and launches (shared with
// the run, ezpz_system_tolerance_mc_effects in tolerance_mc.hip) and the reduction alone on a caller's samples, on a workspace the
// process owns per device.
#define EZPZ_MCE_KERNELS
#include "mc_effects.hip.hpp"

#include <atomic>

using namespace ezpz;

namespace ezpz {
namespace mce {

static_assert(sizeof(EzpzMcEffectConfig) == 8, "the layout include/ezpz_amd.h documents");
static_assert(kMaxBins <= 256, "a bin is staged as a byte");

int enqueue_effects(mcb::Work& work, EffectArgs a, hipStream_t stream) {
    a.part = work.part.p;
    a.part_n = work.part_n.p;
    a.ticket = work.ticket.p;
    const uint32_t blocks = (uint32_t)((a.count + kBlock - 1) / kBlock);
    const size_t lds = effects_lds_bytes(a.k, a.n_meas);
    // (k = m = 32 stages 72 KiB; the attribute belongs to the kernel: raised once per device and size)
    static std::atomic<size_t> raised[16];
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (lds > 48 * 1024 && raised[device & 15].load(std::memory_order_relaxed) < lds) {
        HIP_TRY(hipFuncSetAttribute((const void*)mc_effects_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        raised[device & 15].store(lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(mc_effects_kernel, dim3(blocks), dim3(256), lds, stream, a);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

int enqueue_close(const CloseArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(mc_effects_close_kernel, dim3(1), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

}  // namespace mce
}  // namespace ezpz

using namespace ezpz::mce;

namespace {
struct EffectWork : mcb::Work {};  // (a type of its own: the process keeps a plan per type)
}

extern "C" {

void ezpz_default_mc_effect_config(EzpzMcEffectConfig* ec) {
    if (ec) default_config(ec);
}

int ezpz_mc_effect_indices(const double* sums, const uint64_t* counts, const double* nominal_m, size_t n_param, size_t n_meas, uint32_t bins,
                           double* cond_mean, double* cond_var, double* eta2, double* first, uint32_t* bins_used) {
    return indices_host(sums, counts, nominal_m, n_param, n_meas, bins, cond_mean, cond_var, eta2, first, bins_used);
}

int ezpz_mc_effects(const double* params, const double* m, const uint8_t* flags, const uint8_t* ok, const double* nominal_m,
                    const double* edges, uint64_t samples, size_t n_param, size_t n_meas, uint32_t bins, uint32_t chunk, double* sums,
                    uint64_t* counts) {
    (void)chunk;  // (the host form has no rounds; the sums' bits do not depend on them)
    return effects_host(params, m, flags, ok, nominal_m, edges, samples, n_param, n_meas, bins, sums, counts);
}

int ezpz_mc_effects_device(const double* params_dev, const double* m_dev, const uint8_t* flags_dev, const uint8_t* ok_dev,
                           const double* nominal_m_dev, const double* edges_dev, uint64_t samples, size_t n_param, size_t n_meas,
                           uint32_t bins, uint32_t chunk_in, double* sums_dev, uint64_t* counts_dev, void* stream_) {
    if (int rc = check_shape(n_param, n_meas, bins)) return rc;
    if (samples && (!params_dev || !m_dev || !nominal_m_dev || !edges_dev || !sums_dev || !counts_dev)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (samples > 0xFFFFFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    if (samples == 0) return EZPZ_OK;
    const uint64_t chunk = round_chunk(chunk_in ? chunk_in : kDefaultSampleChunk, samples, kBlock);
    hipStream_t stream = (hipStream_t)stream_;
    const uint32_t k = (uint32_t)n_param, m = (uint32_t)n_meas, cells = k * bins * m;
    return mcb::on_process_plan<EffectWork>(stream, EFFECTS_WORKSPACE_GROWN, EFFECTS_LAUNCHED, [&](mcb::ProcessPlan<EffectWork>& P) {
        EffectArgs a{};
        a.nominal_m = nominal_m_dev;
        a.edges = edges_dev;
        a.k = k, a.n_meas = m, a.bins = bins;
        a.sums = sums_dev;
        a.counts = counts_dev;
        for (uint64_t first = 0; first < samples; first += chunk) {
            a.params = params_dev + first * k;
            a.m = m_dev + first * m;
            a.flags = flags_dev ? flags_dev + first * m : nullptr;
            a.ok = ok_dev ? ok_dev + first : nullptr;
            a.count = std::min<uint64_t>(chunk, samples - first);
            a.first_round = first == 0;
            if (int rc = enqueue_effects(P.work, a, stream)) return rc;
        }
        return (int)EZPZ_OK;
    }, chunk / kBlock * cells * 2, chunk / kBlock * cells);
}

}  // extern "C"
