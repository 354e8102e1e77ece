"""Reference dimensions (ezpz_system_measure_device and its siblings) in systems per second, printed as the text of
profiles/measure_rate.txt.  Every workload on both placements of the measure kernel (csrc/measure.hip.hpp), forced through
EZPZ_MEASURE_ROUTE -- ROW stages a system's row in LDS, DIRECT gathers it from global memory:

  block system  65 536 x the 2000-variable block system (massive500), 500 Distance records (one per line)
  small sketch  4096 x a 48-variable connected sketch (sketch24), one record of each of the 13 measurable kinds
  sketch150     64 x the 300-variable sketch, 39 records: measure, the response to 16 driving dimensions with the stack-up, the vjp
  threshold     rows of 1024 .. 7168 variables (the most ROW can hold), 256 Distance records, the same number of values per call:
                where DIRECT overtakes ROW is where csrc/policy.hpp: kMeasureRowMaxVars belongs
  reuse         lists that gather every variable 4 .. 90 times over, on rows of 48 and of 1024 variables: whether ROW's side of
                the threshold moves with it, and where short rows stop paying for the staging (kMeasureRowMinVars)

A measure call reads every row once and writes m: bytes moved = batch * (n_vars + n_meas) * 8, printed as GB/s beside what
tools/row_copy_bench.hip reaches on the same box in the same job (a copy of 16 KB rows, read + written).  Everything device
resident.  Host clock from the first enqueue to the end of the stream's synchronise; WARMUP untimed runs of each form, then REPEATS
timed runs, the forms alternating; median (min .. max) of the timed runs.

    python tools/measure_rate.py > profiles/measure_rate.txt
"""
import hashlib
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch  # (before the library: torch brings its own HIP runtime and must be the first to load one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ezpz_amd as E  # noqa: E402
from ezpz_amd import synthetic  # noqa: E402
from ezpz_amd.api import (ARC_ANGLE, ARC_LENGTH, ARC_RADIUS, CIRCLE_RADIUS, DISTANCE, FIXED, HORIZONTAL_DISTANCE,  # noqa: E402
                          HORIZONTAL_POINT_LINE_DISTANCE, LINES_AT_ANGLE, POINT_LINE_DISTANCE, POINTS_AT_ANGLE, VERTICAL_DISTANCE,
                          VERTICAL_POINT_LINE_DISTANCE, _rec, stack_records)

WARMUP, REPEATS = 2, 7
SUMMARY = []  # (workload, n_vars, ROW's time over DIRECT's for measure)
KINDS = ((FIXED, 1), (CIRCLE_RADIUS, 3), (VERTICAL_DISTANCE, 4), (HORIZONTAL_DISTANCE, 4), (DISTANCE, 4), (ARC_RADIUS, 6),
         (POINT_LINE_DISTANCE, 6), (VERTICAL_POINT_LINE_DISTANCE, 6), (HORIZONTAL_POINT_LINE_DISTANCE, 6), (LINES_AT_ANGLE, 8),
         (ARC_ANGLE, 6), (POINTS_AT_ANGLE, 6), (ARC_LENGTH, 6))
ANGLE_OTHER_RAD = 3


def timed(stream, f):
    stream.synchronize()
    t0 = time.perf_counter()
    f()
    stream.synchronize()
    return time.perf_counter() - t0


def all_kinds(rng, n_vars, copies=1):
    recs = []
    for _ in range(copies):
        for kind, n_ids in KINDS:
            r = _rec(kind, [int(v) for v in rng.permutation(n_vars)[:n_ids]], 0.0)
            r["tag"] = ANGLE_OTHER_RAD
            recs.append(r)
    return stack_records(recs)


def run(stream, title, forms, batch, moved=None):
    """forms: name -> callable; every form under both placements, alternating."""
    times = {(k, route): [] for k in forms for route in ("row", "direct")}
    for r in range(WARMUP + REPEATS):
        for (k, route) in times:
            os.environ["EZPZ_MEASURE_ROUTE"] = route
            t = timed(stream, forms[k])
            if r >= WARMUP:
                times[(k, route)].append(t)
    os.environ.pop("EZPZ_MEASURE_ROUTE", None)
    print(f"-- {title}")
    for (k, route), t in times.items():
        t = np.asarray(t)
        gbs = f"   {moved / np.median(t) / 1e9:8.1f} GB/s" if moved and k == "measure" else ""
        print(f"  {k:22s} {route.upper():6s} {np.median(t) * 1e3:10.3f} ms ({t.min() * 1e3:.3f} .. {t.max() * 1e3:.3f})   {batch / np.median(t):14.0f} systems/s{gbs}")
    sys.stdout.flush()
    med = {key: float(np.median(t)) for key, t in times.items()}
    if SUMMARY and len(SUMMARY[-1]) == 2:
        SUMMARY[-1] += (med[("measure", "row")] / med[("measure", "direct")],)
    return med


def workload(stream, title, sysobj, recs, batch, x, n_param=0):
    n, k = sysobj.n_vars, len(recs)
    with torch.cuda.stream(stream):
        m = torch.zeros((batch, k), dtype=torch.float64, device="cuda")
    forms = {"measure": lambda: sysobj.measure_device(x.data_ptr(), recs, batch, m.data_ptr(), stream=stream.cuda_stream)}
    if n_param:
        with torch.cuda.stream(stream):
            gen = torch.Generator(device="cuda").manual_seed(3)
            S = torch.rand((batch, n_param, n), dtype=torch.float64, device="cuda", generator=gen) - 0.5
            tol = torch.full((n_param,), 0.01, dtype=torch.float64, device="cuda")
            gm = torch.ones((batch, k), dtype=torch.float64, device="cuda")
            D = torch.zeros((batch, k, n_param), dtype=torch.float64, device="cuda")
            w, q, gx = torch.zeros_like(m), torch.zeros_like(m), torch.zeros((batch, n), dtype=torch.float64, device="cuda")
        forms["response + stack-up"] = lambda: sysobj.measure_response_device(x.data_ptr(), recs, S.data_ptr(), n_param, batch, D.data_ptr(),
                                                                              tol.data_ptr(), w.data_ptr(), q.data_ptr(), stream=stream.cuda_stream)
        forms["vjp"] = lambda: sysobj.measure_vjp_device(x.data_ptr(), recs, gm.data_ptr(), batch, gx.data_ptr(), stream=stream.cuda_stream)
    moved = batch * (n + k) * 8
    SUMMARY.append((title, n))
    return run(stream, f"{title}: {batch} systems of {n} variables, {k} records; measure moves {moved / 1e6:.1f} MB", forms, batch, moved)


def row_copy_roof():
    """tools/row_copy_bench.hip on this box (built beside it when the binary is not there); its lines as they come."""
    binary = os.path.join(ROOT, "tools", "row_copy_bench.bin")
    if not os.path.exists(binary):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", binary, os.path.join(ROOT, "tools", "row_copy_bench.hip")])
    return subprocess.run([binary], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120).stdout.strip()


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/measure_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print(__doc__.split("\n\n")[0].replace("\n", " "))
    print("%d warm-up and %d timed runs per form." % (WARMUP, REPEATS))
    src = open(os.path.join(ROOT, "ezpz_amd", "csrc", "measure.hip.hpp"), "rb").read()
    print("device:", torch.cuda.get_device_name(0), "| HIP", torch.version.hip, "| measure.hip.hpp sha256", hashlib.sha256(src).hexdigest()[:16])
    rng = np.random.default_rng(1)
    gen = torch.Generator(device="cuda").manual_seed(17)

    def values(batch, n):
        with torch.cuda.stream(stream):
            return torch.rand((batch, n), dtype=torch.float64, device="cuda", generator=gen) * 8.0 - 2.0

    _, recs, g, _, _ = synthetic.make_workload("massive500")
    n = len(g)
    lines = stack_records([_rec(DISTANCE, [4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3], 0.0) for k in range(n // 4)])
    x = values(65536, n)
    workload(stream, "block system", E.System(recs, n), lines, 65536, x)
    del x
    _, recs, g, _, _ = synthetic.make_workload("sketch24")
    workload(stream, "small sketch, all 13 kinds", E.System(recs, len(g)), all_kinds(rng, len(g)), 4096, values(4096, len(g)))
    _, recs, g, _, _ = synthetic.make_workload("sketch150")
    workload(stream, "sketch150", E.System(recs, len(g)), all_kinds(rng, len(g), 3), 64, values(64, len(g)), n_param=16)
    print("-- threshold: 256 Distance records on rows of n variables, 2^25 values per call")
    crossing = None
    for n in (1024, 2048, 3072, 4096, 5120, 6144, 7168):
        s = E.System(stack_records([_rec(FIXED, [v], 0.0) for v in range(n)]), n)
        recs = stack_records([_rec(DISTANCE, [int(v) for v in rng.permutation(n)[:4]], 0.0) for _ in range(256)])
        batch = (1 << 25) // n
        t = workload(stream, f"n = {n}", s, recs, batch, values(batch, n))
        if crossing is None and t[("measure", "direct")] < t[("measure", "row")]:
            crossing = n
    print("-- DIRECT first overtakes ROW at n =", crossing, "(None: nowhere up to what ROW can hold)")
    print("-- reuse: the same rows gathered more often -- 4096 x sketch24 with 13 * c records, 8192 x 1024 variables with r Distance records")
    _, recs, g, _, _ = synthetic.make_workload("sketch24")
    s24, x24 = E.System(recs, len(g)), values(4096, len(g))
    for copies in (4, 16, 64):
        lst = all_kinds(rng, len(g), copies)
        workload(stream, f"sketch24, {sum(k[1] for k in KINDS) * copies / len(g):.1f} gathers per variable", s24, lst, 4096, x24)
    s1k = E.System(stack_records([_rec(FIXED, [v], 0.0) for v in range(1024)]), 1024)
    x1k = values(8192, 1024)
    for count in (1024, 2048, 4096, 8192):
        lst = stack_records([_rec(DISTANCE, [int(v) for v in rng.permutation(1024)[:4]], 0.0) for _ in range(count)])
        workload(stream, f"1024 variables, {4 * count / 1024:.0f} gathers per variable", s1k, lst, 8192, x1k)
    print("-- tools/row_copy_bench.hip on the same box:")
    print(row_copy_roof())
    print("-- summary: measure, ROW's time over DIRECT's (below 1: ROW ahead), by variables per row")
    for title, n, ratio in sorted(SUMMARY, key=lambda w: w[1]):
        print(f"  {n:6d} variables  {ratio:6.3f}  {title}")
    policy = open(os.path.join(ROOT, "ezpz_amd", "csrc", "policy.hpp")).read()
    print("-- csrc/policy.hpp at this run:", ", ".join(re.findall(r"kMeasureRow(?:Min|Max)Vars = \d+", policy)),
          "(ROW between the two, DIRECT outside; the reasons are beside the constants and in DESIGN.md 3i)")


if __name__ == "__main__":
    main()
