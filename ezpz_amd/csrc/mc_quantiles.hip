// Monte-Carlo quantiles (include/ezpz_amd.h: ezpz_mc_quantiles and its _device form): the host side of
// mc_quantiles.hip.hpp -- the host entry (plain C++, no device), the selection's workspace and launches (shared with the run,
// ezpz_system_tolerance_mc_quantiles in tolerance_mc.hip) and the selection alone on a caller's rows, on a workspace the process owns
// per device.
#define EZPZ_QUANTILES_KERNELS
#include "mc_block_sum.hip.hpp"
#include "mc_quantiles.hip.hpp"

using namespace ezpz;

namespace ezpz {
namespace mcq {

static_assert(sizeof(EzpzMcQuantile) == 80 && sizeof(EzpzMcQuantileConfig) == 16, "the layouts include/ezpz_amd.h documents");

int SelectWork::ensure(uint32_t n_meas, uint32_t n_q) {
    int rc;
    if ((rc = cnt.ensure((size_t)n_meas * 4 * n_q * 256)) != EZPZ_OK || (rc = sel_r.ensure(kMaxMeas * kMaxSel)) != EZPZ_OK ||
        (rc = sel_prefix.ensure(kMaxMeas * kMaxSel)) != EZPZ_OK || (rc = slot_prefix.ensure(kMaxMeas * kMaxSel)) != EZPZ_OK ||
        (rc = sel_of.ensure(kMaxMeas * kMaxSel)) != EZPZ_OK || (rc = n_slot.ensure(kMaxMeas)) != EZPZ_OK ||
        (rc = n_sel.ensure(kMaxMeas)) != EZPZ_OK || (rc = n_valid.ensure(kMaxMeas)) != EZPZ_OK)
        return rc;
    return EZPZ_OK;
}

int enqueue_select(SelectWork& work, const double* m, const uint8_t* flags, const uint8_t* ok, uint64_t samples, uint32_t n_meas,
                   const double* probs, uint32_t n_q, double z, EzpzMcQuantile* out, uint32_t cus, hipStream_t stream) {
    SelectArgs a{};
    a.m = m, a.flags = flags, a.ok = ok;
    a.samples = samples;
    a.n_meas = n_meas, a.n_q = n_q;
    for (uint32_t q = 0; q < n_q; ++q) a.probs[q] = probs[q];
    a.z = z;
    a.cnt = work.cnt.p;
    a.sel_prefix = work.sel_prefix.p, a.sel_r = work.sel_r.p, a.slot_prefix = work.slot_prefix.p;
    a.n_slot = work.n_slot.p, a.n_sel = work.n_sel.p, a.sel_of = work.sel_of.p, a.n_valid = work.n_valid.p;
    a.out = out;
    HIP_TRY(hipMemsetAsync(a.cnt, 0, (size_t)n_meas * 4 * n_q * 256 * sizeof(uint32_t), stream));
    const uint64_t turns = (samples + kRows - 1) / kRows;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(turns, (uint64_t)std::max<uint32_t>(cus, 1) * 2);
    for (uint32_t pass = 0; pass < 8; ++pass) {
        a.pass = pass;
        a.d_cap = d_cap_of(n_meas, n_q, pass);
        hipLaunchKernelGGL(mc_quantile_count_kernel, dim3(grid), dim3(256), lds_bytes_of(n_meas, n_q, pass), stream, a);
        hipLaunchKernelGGL(mc_quantile_narrow_kernel, dim3(n_meas), dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return EZPZ_OK;
}

}  // namespace mcq
}  // namespace ezpz

using namespace ezpz::mcq;

extern "C" {

void ezpz_default_mc_quantile_config(EzpzMcQuantileConfig* qc) {
    if (qc) default_config(qc);
}

int ezpz_mc_quantiles(const double* m, const uint8_t* flags, const uint8_t* ok, uint64_t samples, size_t n_meas, const double* probs,
                      size_t n_q, const EzpzMcQuantileConfig* qc, EzpzMcQuantile* out) {
    return quantiles_host(m, flags, ok, samples, n_meas, probs, n_q, qc, out);
}

int ezpz_mc_quantiles_device(const double* m_dev, const uint8_t* flags_dev, const uint8_t* ok_dev, uint64_t samples, size_t n_meas,
                             const double* probs, size_t n_q, const EzpzMcQuantileConfig* qc, EzpzMcQuantile* out_dev, void* stream_) {
    double z;
    if (int rc = check(samples, n_meas, probs, n_q, qc, m_dev, out_dev, z)) return rc;
    if (samples == 0 || n_q == 0) return EZPZ_OK;
    hipStream_t stream = (hipStream_t)stream_;
    return mcb::on_process_plan<SelectWork>(stream, QUANTILES_WORKSPACE_GROWN, QUANTILES_LAUNCHED, [&](mcb::ProcessPlan<SelectWork>& P) {
        uint32_t cus = 0;
        if (int rc = P.units(cus)) return rc;
        return enqueue_select(P.work, m_dev, flags_dev, ok_dev, samples, (uint32_t)n_meas, probs, (uint32_t)n_q, z, out_dev, cus, stream);
    }, (uint32_t)n_meas, (uint32_t)n_q);
}

}  // extern "C"
