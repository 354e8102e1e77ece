// Factorial effects of a corner run (include/ezpz_amd.h: ezpz_mc_factorial and its _device form): the host side of
// mc_factorial.hip.hpp -- the host entry (plain C++, no device), the reduction's workspace and launches (shared with the run,
// ezpz_system_tolerance_mc_factorial in tolerance_mc.hip) and the reduction alone on a caller's rows, on a workspace the process owns
// per device.
#define EZPZ_MCF_KERNELS
#include "mc_factorial.hip.hpp"

#include <cstddef>

using namespace ezpz;

namespace ezpz {
namespace mcf {

static_assert(sizeof(EzpzMcFactorial) == 56 && offsetof(EzpzMcFactorial, complete) == 8 && offsetof(EzpzMcFactorial, mean_dev) == 24,
              "the layout include/ezpz_amd.h documents");

namespace {
size_t part_count(uint32_t n_meas, uint32_t kc) { return (size_t)n_meas * ((((size_t)1 << kc) + kBlock - 1) / kBlock) * (2 * kc + 1); }
}  // namespace

bool FactorialWork::grows(uint32_t n_meas, uint32_t kc) const {
    return ((size_t)n_meas << kc) > w.cap || part_count(n_meas, kc) > part.cap || !cnt.p;
}

int FactorialWork::ensure(uint32_t n_meas, uint32_t kc) {
    int rc;
    if ((rc = w.ensure((size_t)n_meas << kc)) != EZPZ_OK || (rc = part.ensure(part_count(n_meas, kc))) != EZPZ_OK ||
        (rc = cnt.ensure(kMaxMeas)) != EZPZ_OK)
        return rc;
    return EZPZ_OK;
}

int enqueue_factorial(FactorialWork& work, const double* m, const uint8_t* flags, const uint8_t* ok, const double* nominal_m, uint32_t kc,
                      uint32_t n_meas, const FactorialOut& out, uint32_t cus, hipStream_t stream) {
    const uint32_t N = 1u << kc, ta = std::min(kc, kTa);
    FactorialArgs a{};
    a.m = m, a.flags = flags, a.ok = ok, a.nominal_m = nominal_m;
    a.kc = kc, a.n_meas = n_meas;
    a.blocks = (N + kBlock - 1) / kBlock;
    a.scale = 1.0 / (double)N;
    a.w = work.w.p, a.cnt = work.cnt.p, a.part = work.part.p;
    a.info = out.info;
    a.main = out.main, a.pair = out.pair, a.ss_order = out.ss_order, a.ss_total = out.ss_total, a.first = out.first, a.total = out.total;
    a.coef = out.coef;
    HIP_TRY(hipMemsetAsync(a.cnt, 0, kMaxMeas * sizeof(uint32_t), stream));
    // four workgroups of 33 KiB of LDS fit a compute unit; eight a unit at most, each taking its tiles in turns
    const uint32_t wide = std::max<uint32_t>(cus, 1) * 8;
    hipLaunchKernelGGL(mc_factorial_gather_kernel, dim3(std::min(N >> ta, wide)), dim3(256), 0, stream, a);
    for (uint32_t l0 = ta; l0 < kc; l0 += kG) {
        a.level0 = l0;
        a.levels = std::min(kG, kc - l0);
        const uint64_t tiles = (uint64_t)(N >> (a.levels + 5)) * n_meas;
        hipLaunchKernelGGL(mc_factorial_strided_kernel, dim3((uint32_t)std::min<uint64_t>(tiles, wide)), dim3(256), 0, stream, a);
    }
    hipLaunchKernelGGL(mc_factorial_walk_kernel, dim3((a.blocks + 3) / 4, n_meas), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(mc_factorial_close_kernel, dim3(n_meas), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EZPZ_OK;
}

}  // namespace mcf
}  // namespace ezpz

using namespace ezpz::mcf;

extern "C" {

int ezpz_mc_factorial(const double* m, const uint8_t* flags, const uint8_t* ok, const double* nominal_m, uint32_t n_corner, size_t n_meas,
                      EzpzMcFactorial* info, double* main, double* pair, double* ss_order, double* ss_total, double* first, double* total,
                      double* coef) {
    return factorial_host(m, flags, ok, nominal_m, n_corner, n_meas, info, main, pair, ss_order, ss_total, first, total, coef);
}

int ezpz_mc_factorial_device(const double* m_dev, const uint8_t* flags_dev, const uint8_t* ok_dev, const double* nominal_m_dev,
                             uint32_t n_corner, size_t n_meas, EzpzMcFactorial* info_dev, double* main_dev, double* pair_dev,
                             double* ss_order_dev, double* ss_total_dev, double* first_dev, double* total_dev, double* coef_dev,
                             void* stream_) {
    if (int rc = check(n_corner, n_meas, m_dev, nominal_m_dev, info_dev, main_dev, pair_dev, ss_order_dev, ss_total_dev, first_dev, total_dev))
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    return mcb::on_process_plan<FactorialWork>(stream, FACTORIAL_WORKSPACE_GROWN, FACTORIAL_LAUNCHED, [&](mcb::ProcessPlan<FactorialWork>& P) {
        uint32_t cus = 0;
        if (int rc = P.units(cus)) return rc;
        FactorialOut out;
        out.info = info_dev;
        out.main = main_dev, out.pair = pair_dev, out.ss_order = ss_order_dev, out.ss_total = ss_total_dev, out.first = first_dev;
        out.total = total_dev, out.coef = coef_dev;
        return enqueue_factorial(P.work, m_dev, flags_dev, ok_dev, nominal_m_dev, n_corner, (uint32_t)n_meas, out, cus, stream);
    }, (uint32_t)n_meas, n_corner);
}

}  // extern "C"
