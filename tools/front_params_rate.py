"""Driven dimensions and sweeps on the frontal shape (ezpz_system_set_params_route), printed as the text of
profiles/front_params_rate.txt.  On connected sketches of 300, 2000 and 5000 variables (tests/gen.py: connected_sketch) created
with EZPZ_TEAM_FRONTS:

  (a) ezpz_system_solve_batch_params_device with the route set against the same call with the route unset on the same system
      (the list-walk teams; after every change of route one untimed call first, which uploads the route's table);
  (b) the params entry on the fronts, driving the system's own values, against the plain entry on the fronts: what the overlay costs;
  (c) a sweep of 240 steps in one launch (where the route's table says in_kernel) against the chain of params calls.

Device resident, one stream, host clock from the first enqueue to the end of the stream's synchronise; WARMUP untimed runs of each
form, then REPEATS timed runs, the two forms alternating; median (min .. max) of the timed runs in milliseconds.  Every parametrised
constraint is driven, +-1e-3 around the system's own values (sweeps: a random walk of +-4e-3 per step from them).

    python tools/front_params_rate.py > profiles/front_params_rate.txt
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

WARMUP, REPEATS = 2, 7
SKETCHES = (150, 1000, 2500)  # points: 300, 2000, 5000 variables
BATCHES = (1, 16)
STEPS = 240


def timed(stream, f):
    stream.synchronize()
    t0 = time.perf_counter()
    f()
    stream.synchronize()
    return time.perf_counter() - t0


def alternate(stream, first, second, before_first=None, before_second=None):
    """WARMUP + REPEATS alternating runs of two forms; before_*: untimed, before every run of that form."""
    a, b = [], []
    for r in range(WARMUP + REPEATS):
        for f, before, out in ((first, before_first, a), (second, before_second, b)):
            if before:
                before()
                stream.synchronize()
            t = timed(stream, f)
            if r >= WARMUP:
                out.append(t)
    return np.asarray(a), np.asarray(b)


def line(what, name_a, ta, name_b, tb):
    verdict = ("beyond the spread" if ta.max() < tb.min() else "SLOWER beyond the spread" if ta.min() > tb.max() else "WITHIN the spread")
    print(f"  {what:34s} {name_a} {np.median(ta) * 1e3:9.3f} ({ta.min() * 1e3:.3f} .. {ta.max() * 1e3:.3f})   {name_b} {np.median(tb) * 1e3:9.3f}"
          f" ({tb.min() * 1e3:.3f} .. {tb.max() * 1e3:.3f})   x{np.median(tb) / np.median(ta):6.2f}  {verdict}")
    sys.stdout.flush()


def main():
    from gen import connected_sketch

    if E.device_count() < 1:
        raise SystemExit("tools/front_params_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    L, cfg = E.lib(), C.byref(E.Config()._c())
    print(__doc__.split("\n\n")[0].replace("\n", " "))
    print("x = second form's median / first form's median; 'beyond the spread': the first form's slowest run is faster than the second's")
    print("fastest ('SLOWER beyond the spread': its fastest is slower than the second's slowest).  %d warm-up and %d timed runs." % (WARMUP, REPEATS))
    print("device:", torch.cuda.get_device_name(0))
    for npts in SKETCHES:
        recs, g = connected_sketch(npts, 1000 + npts)
        n = len(g)
        s = E.System(recs, n, team_size=E.TEAM_FRONTS)
        info = s.info()
        assert info["team_mode"] == 5 and info["front_max_batch"] == 0xFFFFFFFF, info
        pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
        k = len(pos)
        s.set_params_route("fronts")
        plan = s.sweep_params_plan(pos)
        print(f"-- connected sketch, {n} variables, {len(recs)} constraints, {k} driven: {info['grid_workgroups']} workgroups per system;"
              f" sweep plan: route {plan['route_name']}, in_kernel {plan['in_kernel']}, params_in_lds {plan['params_in_lds']}, lds_bytes {plan['lds_bytes']}")
        for batch in BATCHES:
            rng = np.random.default_rng(batch * 1000 + npts)
            x0 = g[None, :] + rng.uniform(-0.01, 0.01, (batch, n))
            params = recs["param"][pos][None, :] + rng.uniform(-1e-3, 1e-3, (batch, k))
            own = np.repeat(recs["param"][pos][None, :], batch, axis=0)
            with torch.cuda.stream(stream):
                xin, pd, od = torch.from_numpy(x0).cuda(), torch.from_numpy(params).cuda(), torch.from_numpy(own).cuda()
                xo = [torch.zeros((batch, n), dtype=torch.float64, device="cuda") for _ in range(2)]
                st = [torch.zeros((batch, STATUS_DTYPE.itemsize), dtype=torch.uint8, device="cuda") for _ in range(2)]
            pp = pos.ctypes.data

            def params_call(values, o):
                def f():
                    rc = L.ezpz_system_solve_batch_params_device(s._h, xin.data_ptr(), pp, k, values.data_ptr(), batch, cfg, xo[o].data_ptr(),
                                                                 st[o].data_ptr(), None, None, 0, h)
                    assert rc == 0, rc
                return f

            def plain_call():
                rc = L.ezpz_system_solve_batch_device(s._h, xin.data_ptr(), batch, cfg, xo[1].data_ptr(), st[1].data_ptr(), None, None, 0, h)
                assert rc == 0, rc

            # (a) the route set against the route unset
            s.set_params_route("default")
            rc = L.ezpz_system_solve_batch_params_device(s._h, xin.data_ptr(), pp, k, pd.data_ptr(), batch, cfg, xo[1].data_ptr(),
                                                         st[1].data_ptr(), None, None, 0, h)
            stream.synchronize()
            if rc != 0:
                print(f"  (a) batch {batch:3d}: the route unset declines the call ({E.NonLinearSystemError(rc)}): nothing to compare with")
                s.set_params_route("fronts")
            else:
                def to(route, o):
                    def f():
                        s.set_params_route(route)
                        params_call(pd, o)()
                    return f
                ta, tb = alternate(stream, params_call(pd, 0), params_call(pd, 1), to("fronts", 0), to("default", 1))
                conv = [t.cpu().numpy().view(STATUS_DTYPE)["converged"].mean() for t in st]
                line(f"(a) batch {batch:3d} params entry:", "fronts", ta, "route unset", tb)
                print(f"      converged {conv[0]:.3f} (fronts) {conv[1]:.3f} (route unset)")
                s.set_params_route("fronts")
            # (b) the overlay's cost: own values driven against the plain entry
            params_call(od, 0)(), plain_call()
            stream.synchronize()
            assert torch.equal(xo[0], xo[1]) and torch.equal(st[0], st[1]), "own values driven differ from the plain entry"
            ta, tb = alternate(stream, params_call(od, 0), plain_call)
            line(f"(b) batch {batch:3d} own values driven:", "params", ta, "plain", tb)
            # (c) a sweep of STEPS steps against the chain
            walk = np.cumsum(rng.uniform(-0.004, 0.004, (STEPS, batch, k)), axis=0)
            with torch.cuda.stream(stream):
                wd = torch.from_numpy(np.ascontiguousarray(recs["param"][pos][None, None, :] + walk)).cuda()
                out = [(torch.zeros((STEPS, batch, n), dtype=torch.float64, device="cuda"),
                        torch.zeros((STEPS, batch, STATUS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")) for _ in range(2)]
            k_bytes, x_bytes, s_bytes = batch * k * 8, batch * n * 8, batch * STATUS_DTYPE.itemsize
            (xs, ss), (xc, sc) = (t.data_ptr() for t in out[0]), (t.data_ptr() for t in out[1])
            links = [(xin.data_ptr() if j == 0 else xc + (j - 1) * x_bytes, wd.data_ptr() + j * k_bytes, xc + j * x_bytes, sc + j * s_bytes)
                     for j in range(STEPS)]

            def sweep():
                rc = L.ezpz_system_sweep_params_device(s._h, xin.data_ptr(), pp, k, wd.data_ptr(), STEPS, batch, cfg, xs, ss, None, None, 0, h)
                assert rc == 0, rc

            def chain_of_launches():
                for src, par, dst, sta in links:
                    rc = L.ezpz_system_solve_batch_params_device(s._h, src, pp, k, par, batch, cfg, dst, sta, None, None, 0, h)
                    assert rc == 0, rc

            sweep(), chain_of_launches()
            stream.synchronize()
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), "the sweep and the chain differ"
            conv = out[0][1].cpu().numpy().view(STATUS_DTYPE)["converged"].mean()
            ta, tb = alternate(stream, sweep, chain_of_launches)
            line(f"(c) batch {batch:3d} sweep of {STEPS} steps:", "sweep", ta, "chain", tb)
            print(f"      in_kernel {plan['in_kernel']}, converged {conv:.3f}, {batch * STEPS / np.median(ta):.0f} vs {batch * STEPS / np.median(tb):.0f} steps/s")


if __name__ == "__main__":
    main()
