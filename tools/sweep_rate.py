"""Rate of a dimension sweep in one launch (ezpz_system_sweep_params_device) against the chain of solve_batch_params_device calls
it is defined as, printed as the text of profiles/sweep_rate.txt.

Device resident: starts, parameters and results stay on the device; both forms are enqueued on one stream and the host clock runs
from the first enqueue to the stream's synchronise, so the chain's time includes the gaps between its launches -- that is what a
caller of the chain waits for.  Both forms go through the C entries (ctypes) with the list, the configuration and the pointers
made before the clock starts; the time the chain's calls take to return is reported beside its total.  Per (shape, batch, steps): WARMUP untimed runs of each form, then REPEATS timed runs, the two
forms alternating; the figures are the median and the spread (min .. max) of the repeats.  Equal bits (values and statuses) of
the two forms are asserted before anything is timed.

Shapes: a connected 300-variable sketch on one barrier workgroup per sweep, a chain of 40 points on sub-wavefront teams,
massive_parallel_system on the component interpreter -- and the two other routes, 64 independent blocks on the wavefront-
partitioned workgroup and a sketch of 70 points on the record walk; up to 8 of each system's parametrised constraints are
driven along a random walk.

    python tools/sweep_rate.py > profiles/sweep_rate.txt
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch  # (before the library: torch brings its own HIP runtime and must be the first to load one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ezpz_amd as E  # noqa: E402
from ezpz_amd._lib import STATUS_DTYPE  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import textual as T  # noqa: E402

WARMUP, REPEATS = 2, 7
BATCHES, STEPS = (1, 64, 4096), (16, 240)
MAX_DRIVEN = 8
MAX_BYTES = 12 << 30  # of results per form: a larger case is reported as not measured


def systems():
    from gen import connected_sketch
    from sweep_common import chain, record_walk_sketch

    recs, g = connected_sketch(150, 11)
    crecs, cg = chain(40)
    block = T.load(T.gen_big_problem(64))
    rrecs, rg = record_walk_sketch()
    path = os.path.join(ROOT, "tests", "golden", "test_cases", "massive_parallel_system", "problem.md")
    ref = T.load(open(path).read())
    return [("sketch, 300 variables", E.System(recs, len(g), team_size=256), recs, np.asarray(g, dtype=float)),
            ("chain of 40 points", E.System(crecs, len(cg), team_size=64), crecs, cg),
            ("massive_parallel_system", E.System(O.stack(ref.constraints), ref.num_vars), O.stack(ref.constraints), ref.guesses),
            ("64 blocks, partitioned", E.System(O.stack(block.constraints), block.num_vars, team_size=E.TEAM_AUTO_LISTS),
             O.stack(block.constraints), block.guesses),
            ("sketch of 70 points", E.System(rrecs, len(rg), team_size=E.TEAM_LATENCY_RECORDS), rrecs, rg)]


def measure(system, recs, g, batch, steps, stream):
    n = len(g)
    rng = np.random.default_rng(batch * 1000 + steps)
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    pos = pos[np.linspace(0, len(pos) - 1, min(MAX_DRIVEN, len(pos))).astype(int)]
    walk = np.cumsum(rng.uniform(-0.004, 0.004, (steps, batch, len(pos))), axis=0)
    params = np.ascontiguousarray(recs["param"][pos][None, None, :] + walk)
    x0 = g[None, :] + rng.uniform(-0.01, 0.01, (batch, n))
    with torch.cuda.stream(stream):
        pd, xin = torch.from_numpy(params).cuda(), torch.from_numpy(x0).cuda()
        out = [(torch.zeros((steps, batch, n), dtype=torch.float64, device="cuda"),
                torch.zeros((steps, batch, STATUS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")) for _ in range(2)]
    h = stream.cuda_stream
    k_bytes, x_bytes, s_bytes = batch * len(pos) * 8, batch * n * 8, batch * STATUS_DTYPE.itemsize
    # (both forms through the C entries, with the list, the configuration and every pointer made before the clock starts: the
    # chain's host side is then `steps` foreign calls and nothing else)
    L, cfg = E.lib(), C.byref(E.Config()._c())
    pp, (xs, ss), (xc, sc) = pos.ctypes.data, (t.data_ptr() for t in out[0]), (t.data_ptr() for t in out[1])
    links = [(xin.data_ptr() if k == 0 else xc + (k - 1) * x_bytes, pd.data_ptr() + k * k_bytes, xc + k * x_bytes, sc + k * s_bytes)
             for k in range(steps)]

    def sweep():
        rc = L.ezpz_system_sweep_params_device(system._h, xin.data_ptr(), pp, len(pos), pd.data_ptr(), steps, batch, cfg, xs, ss,
                                               None, None, 0, h)
        assert rc == 0, rc

    def chain_of_launches():
        for src, par, dst, st in links:
            rc = L.ezpz_system_solve_batch_params_device(system._h, src, pp, len(pos), par, batch, cfg, dst, st, None, None, 0, h)
            assert rc == 0, rc

    def timed(f):
        """(seconds from the first enqueue to the end of the synchronise, seconds of that spent enqueuing)"""
        stream.synchronize()
        t0 = time.perf_counter()
        f()
        t1 = time.perf_counter()
        stream.synchronize()
        return time.perf_counter() - t0, t1 - t0

    for _ in range(WARMUP):
        timed(sweep), timed(chain_of_launches)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), "the sweep and the chain differ"
    conv = out[0][1].cpu().numpy().view(STATUS_DTYPE)["converged"].mean()
    ts, tc = [], []
    for _ in range(REPEATS):
        ts.append(timed(sweep)), tc.append(timed(chain_of_launches))
    return np.asarray(ts), np.asarray(tc), float(conv), len(pos)


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/sweep_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("sweep in one launch against the chain of solve_batch_params_device calls; device resident, one stream, host clock from")
    print("the first enqueue to the stream's synchronise; %d warm-up runs, then %d timed runs of each form, alternating; median" % (WARMUP, REPEATS))
    print("(min .. max) of the timed runs in milliseconds; rate = batch * steps / median; equal bits asserted.  Both forms are called")
    print("through the C entries with every argument made beforehand; 'enqueue' is the part of the chain's time its `steps` calls take")
    print("to return (median, and its share of the run): while they enqueue the device already works, so the share is host time that")
    print("bounds the chain from below, not time added to the device's.  'beyond the spread': the sweep's slowest run is faster than")
    print("the chain's fastest ('SLOWER beyond the spread': its fastest is slower than the chain's slowest).")
    print("device:", torch.cuda.get_device_name(0))
    for name, system, recs, g in systems():
        plan = None
        for batch in BATCHES:
            for steps in STEPS:
                if steps * batch * len(g) * 8 > MAX_BYTES:
                    print(f"{name:26s} batch {batch:5d} steps {steps:4d}  not measured (results of one form exceed {MAX_BYTES >> 30} GiB)")
                    continue
                ts, tc, conv, k = measure(system, recs, g, batch, steps, stream)
                if plan is None:
                    pos = [i for i in range(len(recs)) if E.constraint_has_param(recs[i])][:1]
                    plan = system.sweep_params_plan(pos)
                    print(f"-- {name}: route {plan['route_name']}, in_kernel {plan['in_kernel']}, {k} driven parameters")
                ms, mc = np.median(ts[:, 0]), np.median(tc[:, 0])
                verdict = ("beyond the spread" if ts[:, 0].max() < tc[:, 0].min() else
                           "SLOWER beyond the spread" if ts[:, 0].min() > tc[:, 0].max() else "WITHIN the spread")
                print(f"{name:26s} batch {batch:5d} steps {steps:4d}  sweep {ms * 1e3:9.3f} ({ts[:, 0].min() * 1e3:.3f} .. {ts[:, 0].max() * 1e3:.3f})"
                      f"  chain {mc * 1e3:9.3f} ({tc[:, 0].min() * 1e3:.3f} .. {tc[:, 0].max() * 1e3:.3f}; enqueue {np.median(tc[:, 1]) * 1e3:.3f} ="
                      f" {100 * np.median(tc[:, 1] / tc[:, 0]):.0f} %)"
                      f"  {batch * steps / ms:12.0f} vs {batch * steps / mc:12.0f} steps/s  x{mc / ms:5.2f}"
                      f"  {verdict}  converged {conv:.3f}")
                sys.stdout.flush()


if __name__ == "__main__":
    main()
