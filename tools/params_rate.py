"""Solves/s of ezpz_system_solve_batch_params_device with every parametrised constraint driven, against the plain entry on the
same system and the same route, device-resident buffers, one process.  Two systems: massive_parallel_system on the component
interpreter (before any compilation: EZPZ_JIT=0 keeps the plain entry there) and one connected sketch of ~300 variables on the
list-walk teams (EZPZ_TEAM_AUTO_LISTS).  Per rate: warm-up, then the median of `--repeats` timed runs of `--calls` launches
each between two events; the extra compulsory bytes per system (8 * n_param) beside the rates.

    EZPZ_JIT=0 python tools/params_rate.py > profiles/params_rate.txt
"""
import argparse
import os
import sys

os.environ.setdefault("EZPZ_JIT", "0")
import torch  # noqa: E402  (before the library: tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402

import ezpz_amd as E  # noqa: E402
from ezpz_amd._lib import STATUS_DTYPE  # noqa: E402


def rate(fn, batch, calls, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(batch * calls / (a.elapsed_time(b) * 1e-3))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def measure(name, recs, guesses, team, batch, jitter, args):
    n = len(guesses)
    s = E.System(recs, n, team_size=team)
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    rng = np.random.default_rng(0)
    x0 = torch.from_numpy(guesses[None, :] + rng.uniform(-jitter, jitter, (batch, n))).cuda()
    par = torch.from_numpy(np.repeat(recs["param"][pos][None, :], batch, axis=0)).cuda()  # (the system's own values: the same solves)
    xo = torch.empty_like(x0)
    st = torch.zeros(batch * STATUS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    plain = lambda: s.solve_batch_device(x0.data_ptr(), batch, xo.data_ptr(), st.data_ptr(), stream=stream)
    driven = lambda: s.solve_batch_params_device(x0.data_ptr(), pos, par.data_ptr(), batch, xo.data_ptr(), st.data_ptr(), stream=stream)
    plain()
    torch.cuda.synchronize()
    ref = xo.clone()
    driven()
    torch.cuda.synchronize()
    same = bool(torch.equal(ref, xo))
    info = s.info()
    rp, rd = rate(plain, batch, args.calls, args.repeats), rate(driven, batch, args.calls, args.repeats)
    print(f"{name}: {n} variables, {len(recs)} constraints, n_param {len(pos)} (+{8 * len(pos)} B per system beside {16 * n} B of values), "
          f"team_mode {info['team_mode']}, batch {batch}, same bits {same}")
    print(f"    plain entry   {rp[0] / 1e6:9.3f} M solves/s (min {rp[1] / 1e6:.3f}, max {rp[2] / 1e6:.3f})")
    print(f"    driven entry  {rd[0] / 1e6:9.3f} M solves/s (min {rd[1] / 1e6:.3f}, max {rd[2] / 1e6:.3f})   ratio {rd[0] / rp[0]:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import gen
    from oracle import oracle as O
    from oracle import textual as T

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref = T.load(open(os.path.join(root, "tests", "golden", "test_cases", "massive_parallel_system", "problem.md")).read())
    measure("massive_parallel_system on the interpreter", O.stack(ref.constraints), ref.guesses, 0, 16384, 0.25, args)
    recs, g = gen.connected_sketch(150, 3)
    measure("connected sketch on the list-walk teams", recs, g, E.TEAM_AUTO_LISTS, 16384, 0.02, args)


if __name__ == "__main__":
    main()
