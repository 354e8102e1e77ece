// Launch of the FRONTAL shape (front_kernel.hip.hpp; plan: fronts.cpp): one workgroup per system, or G workgroups per system
// that must all be resident (they wait for each other's chunks), as many systems in flight as the device holds.
#include "front_launch.hip.hpp"

using namespace ezpz;

namespace ezpz {

template <bool LIN>
static int front_launch_kernel(EzpzSystem& s, FrontArgs& fa, hipStream_t stream) {
    const FrontPlan& plan = *s.fronts;
    auto kernel = front_solve_kernel<LIN>;
    if (s.front_capacity == 0) {  // once per system: these runtime calls cost more than a small solve
        int per_cu = 0;
        if (int rc = front_per_cu(s, kernel, plan.lds_bytes, per_cu)) return rc;
        s.front_capacity = (uint64_t)s.lim.cus * (uint64_t)std::max(per_cu, 1);
    }
    return front_launch_on(s, kernel, fa, s.front_capacity, plan.lds_bytes, fa.batch, fa.batch, stream);
}

static int front_launch_with(EzpzSystem& s, SolveArgs& args, hipStream_t stream, const FrontProbe& probe) {
    if (!s.dev_fronts) return EZPZ_ERR_INVALID_ARGUMENT;
    FrontArgs fa = front_args_for(s, args, probe);
    return s.fronts->linear_only ? front_launch_kernel<true>(s, fa, stream) : front_launch_kernel<false>(s, fa, stream);
}

int front_launch(EzpzSystem& s, SolveArgs& args, hipStream_t stream) { return front_launch_with(s, args, stream, FrontProbe{}); }

// The null-space probes of FreedomAnalysis (FrontArgs::probe_m): `m` probes of `batch` systems at the values x_dev ([batch][n_vars],
// caller order), answers to y_dev ([batch][m][n_vars]); w_dev: the probes' vectors ([batch][m][n_vars]), or null = pseudo-random entries, uniform in [-1, 1).
int front_launch_probe(EzpzSystem& s, const double* x_dev, size_t batch, double* y_dev, uint32_t m, hipStream_t stream, const double* w_dev,
                       double lambda_scale) {
    if (!s.fronts || !s.dev_fronts || !m) return EZPZ_ERR_INVALID_ARGUMENT;
    SolveArgs args{};
    args.x0 = x_dev;
    args.batch = batch * m;  // (a work item is one probe of one system: front_kernel.hip.hpp)
    args.max_iterations = 0;
    args.residual_tolerance = 0.0;
    args.step_tolerance = 0.0;
    args.initial_lambda = 0.0;
    // (like launch(): what a launch creates on first use -- the occupancy figure, the scratch of several workgroups -- under the lock)
    std::lock_guard<std::mutex> launch_lock(s.launch_mu);
    FrontProbe probe;
    probe.m = m;
    probe.out = y_dev;
    probe.in = w_dev;
    probe.scale = lambda_scale;
    return front_launch_with(s, args, stream, probe);
}

}  // namespace ezpz
