"""Systems/s of ezpz_system_param_sensitivity_device (device-resident buffers, one process) against the only alternative the
library offered before it: k + 1 calls of ezpz_system_solve_batch_params_device on the same systems (finite differences; that
entry's kernels are untouched by the sensitivity work, so this build times them as the parent's).  16384 systems of
massive500, sketch150 and a small kind-by-kind case; k = every parametrised constraint, capped at 32 for sketch150 (S is
batch x k x n doubles).  Per side: warm-up, then the median of `--repeats` runs between two events.

    python tools/sensitivity_rate.py > profiles/sensitivity_rate.txt
    rocprofv3 --kernel-trace --stats -- python tools/sensitivity_rate.py --repeats 1      (the new kernels' share)
"""
import argparse
import os
import sys

import torch  # noqa: E402  (before the library: tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import ezpz_amd as E  # noqa: E402
from ezpz_amd import synthetic  # noqa: E402
from ezpz_amd._lib import STATUS_DTYPE  # noqa: E402


def seconds(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(out))


def measure(name, recs, guesses, jitter, batch, cap, args):
    n = len(guesses)
    s = E.System(recs, n)
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    if cap and len(pos) > cap:
        pos = pos[np.linspace(0, len(pos) - 1, cap).astype(int)]
    k = len(pos)
    rng = np.random.default_rng(0)
    x0 = torch.from_numpy(guesses[None, :] + rng.uniform(-jitter, jitter, (batch, n))).cuda()
    par = torch.from_numpy(np.repeat(recs["param"][pos][None, :], batch, axis=0)).cuda()
    x = torch.empty_like(x0)
    st = torch.zeros(batch * STATUS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    solve = lambda: s.solve_batch_params_device(x0.data_ptr(), pos, par.data_ptr(), batch, x.data_ptr(), st.data_ptr(), stream=stream)
    solve()
    torch.cuda.synchronize()
    xs = x.clone()
    S = torch.empty((batch, k, n), dtype=torch.float64, device="cuda")
    status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    sens = lambda: s.param_sensitivity_device(xs.data_ptr(), pos, par.data_ptr(), batch, S.data_ptr(), status.data_ptr(), stream=stream)

    def finite_differences():
        for _ in range(k + 1):
            solve()

    t_new, t_old = seconds(sens, args.repeats), seconds(finite_differences, args.repeats)
    plan = s.param_sensitivity_plan(pos)
    print(f"{name}: {n} variables, {len(recs)} constraints, k = {k}, batch {batch}, failed {int(status.sum())}, plan {plan}")
    print(f"    param_sensitivity_device            {t_new * 1e3:10.3f} ms  ({batch / t_new / 1e6:.3f} M systems/s)")
    print(f"    {k + 1:3d} x solve_batch_params_device    {t_old * 1e3:10.3f} ms  ({batch / t_old / 1e6:.3f} M systems/s)   ratio {t_old / t_new:.1f}x")
    return t_old / t_new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16384)
    args = ap.parse_args()
    from test_gpu_params import CASES

    ratios = []
    _, recs, g, jitter, _ = synthetic.make_workload("massive500")
    ratios.append(measure("massive500", np.ascontiguousarray(recs), g, jitter, args.batch, 64, args))
    _, recs, g, jitter, _ = synthetic.make_workload("sketch150")
    ratios.append(measure("sketch150", np.ascontiguousarray(recs), g, jitter, args.batch, 32, args))
    recs, g, _ = CASES["lines_at_angle_deg"]
    ratios.append(measure("kind by kind (lines_at_angle_deg)", recs, g, 0.02, args.batch, 0, args))
    print("the new entry loses nowhere" if min(ratios) >= 1.0 else "THE NEW ENTRY LOSES SOMEWHERE", [round(r, 2) for r in ratios])
    return 0 if min(ratios) >= 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
