"""Dimension sensitivities on the frontal shape (ezpz_system_set_sensitivity_route), printed as the text of
profiles/front_sens_rate.txt.  On connected sketches of 300, 2000 and 5000 variables (tests/gen.py: connected_sketch) created
with EZPZ_TEAM_FRONTS, one system per call, device resident:

  (a) ezpz_system_param_sensitivity_device on the fronts for k = 1, 16, 256 and all listed constraints against what exists
      above the default route's limit without it: k + 1 driven solves on the fronts route (ezpz_system_solve_batch_params_device,
      the k + 1 parameter rows as ONE call of k + 1 systems -- the cheapest way to run them; k + 1 > 257: 257 timed, scaled);
  (b) the route against the default route (sens_block_kernel) where that serves: 300 variables with all constraints listed, and
      hub512 (1024 variables, the 12 listed constraints of tests/sensitivity_ref.py);
  (c) the chunking: EZPZ_SENS_FRONTS_RHS_PER_ITEM = 1 (a factorisation per right-hand side), 2, 4, 8, 16, 64 and one item for the
      whole list, each against the default rule, all constraints listed.

Host clock from the first enqueue to the end of the stream's synchronise; WARMUP untimed runs of each form, then REPEATS timed
runs, the two forms alternating; median (min .. max) of the timed runs in milliseconds.

    python tools/front_sens_rate.py > profiles/front_sens_rate.txt
"""
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
KS = (1, 16, 256, 0)  # 0: all
SOLVES_TIMED_AT_MOST = 257
LAM = 1e-9
ENV = "EZPZ_SENS_FRONTS_RHS_PER_ITEM"


def timed(stream, f):
    stream.synchronize()
    t0 = time.perf_counter()
    f()
    stream.synchronize()
    return time.perf_counter() - t0


def alternate(stream, first, second):
    a, b = [], []
    for r in range(WARMUP + REPEATS):
        for f, out in ((first, a), (second, b)):
            t = timed(stream, f)
            if r >= WARMUP:
                out.append(t)
    return np.asarray(a), np.asarray(b)


def line(what, name_a, ta, name_b, tb, scale_b=1.0):
    tb = tb * scale_b
    verdict = ("beyond the spread" if ta.max() < tb.min() else "SLOWER beyond the spread" if ta.min() > tb.max() else "WITHIN the spread")
    print(f"  {what:40s} {name_a} {np.median(ta) * 1e3:9.3f} ({ta.min() * 1e3:.3f} .. {ta.max() * 1e3:.3f})   {name_b} {np.median(tb) * 1e3:9.3f}"
          f" ({tb.min() * 1e3:.3f} .. {tb.max() * 1e3:.3f})   x{np.median(tb) / np.median(ta):7.2f}  {verdict}")
    sys.stdout.flush()


def sens_call(s, stream, x, pos, S, st, env=None):
    def f():
        if env is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = str(env)
        s.param_sensitivity_device(x.data_ptr(), pos, 0, 1, S.data_ptr(), st.data_ptr(), lam=LAM, stream=stream.cuda_stream)
    return f


def main():
    from gen import connected_sketch

    import sensitivity_ref as R

    if E.device_count() < 1:
        raise SystemExit("tools/front_sens_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print(__doc__.split("\n\n")[0].replace("\n", " "))
    print("x = second form's median / first form's median; 'beyond the spread': the first form's slowest run is faster than the second's")
    print("fastest ('SLOWER beyond the spread': its fastest is slower than the second's slowest).  %d warm-up and %d timed runs." % (WARMUP, REPEATS))
    print("device:", torch.cuda.get_device_name(0))
    cfg = E.Config()
    for npts in SKETCHES:
        recs, g = connected_sketch(npts, 1000 + npts)
        n = len(g)
        s = E.System(recs, n, team_size=E.TEAM_FRONTS)
        info = s.info()
        assert info["team_mode"] == 5 and info["front_max_batch"] == 0xFFFFFFFF, info
        s.set_params_route("fronts")
        s.set_sensitivity_route("fronts")
        driven = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
        x_host, st0, _ = s.solve_batch_params(g[None, :], driven, recs["param"][driven][None, :], cfg)
        print(f"-- connected sketch, {n} variables, {len(recs)} constraints, {len(driven)} with a parameter: {info['grid_workgroups']} workgroups per system"
              f" (values: the solve's answer, converged {int(st0['converged'][0])})")
        with torch.cuda.stream(stream):
            x = torch.from_numpy(x_host).cuda()
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
        for kk in KS:
            pos = driven if kk == 0 else driven[np.linspace(0, len(driven) - 1, kk).astype(int)]
            k = len(pos)
            os.environ.pop(ENV, None)
            plan = s.param_sensitivity_plan(pos)
            with torch.cuda.stream(stream):
                S = torch.zeros((1, k, n), dtype=torch.float64, device="cuda")
                m = min(k + 1, SOLVES_TIMED_AT_MOST)
                rows = torch.from_numpy(np.repeat(recs["param"][pos][None, :], m, axis=0) + 1e-6 * np.eye(m, k, -1)).cuda()
                xin = torch.from_numpy(np.repeat(x_host, m, axis=0)).cuda()
                xo = torch.zeros((m, n), dtype=torch.float64, device="cuda")
                sto = torch.zeros((m, STATUS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")

            def solves():
                s.solve_batch_params_device(xin.data_ptr(), pos, rows.data_ptr(), m, xo.data_ptr(), sto.data_ptr(), stream=stream.cuda_stream)

            ta, tb = alternate(stream, sens_call(s, stream, x, pos, S, st), solves)
            assert int(st.cpu()[0]) == 0
            note = "" if m == k + 1 else f" ({m} timed, x{(k + 1) / m:.1f})"
            line(f"(a) k = {k:5d}: route vs {k + 1} driven solves{note}", "fronts", ta, "solves", tb, (k + 1) / m)
            print(f"      rhs_per_item {plan['rhs_per_item']}, items_per_system {plan['items_per_system']}, {k / np.median(ta):.0f} rows/s")
        # (c) the chunking, all listed
        pos = driven
        k = len(pos)
        with torch.cuda.stream(stream):
            S = torch.zeros((1, k, n), dtype=torch.float64, device="cuda")
            S2 = torch.zeros((1, k, n), dtype=torch.float64, device="cuda")
        for per in (1, 2, 4, 8, 16, 64, k):
            ta, tb = alternate(stream, sens_call(s, stream, x, pos, S, st), sens_call(s, stream, x, pos, S2, st, env=per))
            assert torch.equal(S, S2), "the chunking changed the bits"
            line(f"(c) k = {k:5d}: default vs {per} per item", "default", ta, f"{per:5d}/item", tb)
        os.environ.pop(ENV, None)
        # (b) against the default route where it serves
        if n <= 1024:
            ref = torch.zeros_like(S)

            def to(route, out):
                def f():
                    s.set_sensitivity_route(route)
                    s.param_sensitivity_device(x.data_ptr(), pos, 0, 1, out.data_ptr(), st.data_ptr(), lam=LAM, stream=stream.cuda_stream)
                return f

            ta, tb = alternate(stream, to("fronts", S), to("default", ref))
            err = float((S - ref).abs().max() / max(1.0, float(ref.abs().max())))
            line(f"(b) {n} variables, {k} listed:", "fronts", ta, "default", tb)
            print(f"      largest difference between the routes {err:.3e} (relative to the largest entry)")
            s.set_sensitivity_route("fronts")
    # (b) hub512
    recs, g = R.hub_sketch(512)
    pos = np.asarray([3, 4, 5, 100, 101, 511, 512, 800, 801, 1000, 1020, 1023], dtype=np.uint32)
    s = E.System(recs, len(g), team_size=E.TEAM_FRONTS)
    info = s.info()
    if info["team_mode"] == 5 and info["front_max_batch"] == 0xFFFFFFFF:
        with torch.cuda.stream(stream):
            x = torch.from_numpy(g[None, :].copy()).cuda()
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            S, ref = (torch.zeros((1, len(pos), len(g)), dtype=torch.float64, device="cuda") for _ in range(2))

        def to(route, out):
            def f():
                s.set_sensitivity_route(route)
                s.param_sensitivity_device(x.data_ptr(), pos, 0, 1, out.data_ptr(), st.data_ptr(), lam=LAM, stream=stream.cuda_stream)
            return f

        print(f"-- hub512, {len(g)} variables, {len(pos)} listed: {info['grid_workgroups']} workgroups per system")
        ta, tb = alternate(stream, to("fronts", S), to("default", ref))
        err = float((S - ref).abs().max() / max(1.0, float(ref.abs().max())))
        line("(b) hub512, 12 listed:", "fronts", ta, "default", tb)
        print(f"      largest difference between the routes {err:.3e} (relative to the largest entry)")
    else:
        print("-- hub512: the frontal shape does not serve this system (a front of more than 63 rows): nothing to compare")


if __name__ == "__main__":
    main()
