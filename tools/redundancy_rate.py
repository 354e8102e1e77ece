"""Redundancy analysis (ezpz_system_redundancy_device) in systems per second, printed as the text of
profiles/redundancy_rate.txt.  Three workloads, one per placement of the kernel (csrc/redundancy.hip.hpp), each beside
ezpz_system_freedom_batch_device on the same systems and values for scale (the column-space analysis of the same matrix: a
pivoted QR, a null-space basis and its orthonormalisation per component -- more work per entry, so a yardstick, not a rival):

  LANE          65 536 x the 2000 x 2000 block system (massive500 with a repeated record on every 5th line and one that cannot
                hold on every 7th: tests/redundancy_ref.py: blocks), values drawn on the device
  TEAM, LDS     4096 x a 48-variable connected sketch with six appended records (redundancy_ref.sketch(24, ...))
  TEAM, global  64 x the 300-variable connected sketch with the same insertions

Everything device resident.  Host clock from the first enqueue to the end of the stream's synchronise, so a figure includes the
gather and evaluation launches both entries start with; WARMUP untimed runs of each form, then REPEATS timed runs, the forms
alternating; median (min .. max) of the timed runs.

    python tools/redundancy_rate.py > profiles/redundancy_rate.txt
"""
import hashlib
import os
import sys
import time

import numpy as np
import torch  # (before the library: torch brings its own HIP runtime and must be the first to load one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ezpz_amd as E  # noqa: E402

WARMUP, REPEATS = 2, 7


def timed(stream, f):
    stream.synchronize()
    t0 = time.perf_counter()
    f()
    stream.synchronize()
    return time.perf_counter() - t0


def workload(stream, title, case, batch, x):
    s = E.System(case["recs"], case["n_vars"])
    info = s.info()
    n, n_cs, m = case["n_vars"], len(case["recs"]), info["n_rows"]
    focus = case["focus"][:4]
    with torch.cuda.stream(stream):
        con = torch.zeros((batch, n_cs), dtype=torch.uint8, device="cuda")
        rank = torch.zeros(batch, dtype=torch.int32, device="cuda")
        group = torch.zeros((batch, len(focus), n_cs), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((batch, n), dtype=torch.uint8, device="cuda")
        count = torch.zeros(batch, dtype=torch.int32, device="cuda")
    forms = {
        "redundancy": lambda: s.redundancy_device(x.data_ptr(), batch, con.data_ptr(), 0, rank.data_ptr(), stream=stream.cuda_stream),
        "redundancy + %d groups" % len(focus): lambda: s.redundancy_device(x.data_ptr(), batch, con.data_ptr(), 0, rank.data_ptr(), focus,
                                                                         group.data_ptr(), stream=stream.cuda_stream),
        "freedom": lambda: s.freedom_batch_device(x.data_ptr(), batch, mask.data_ptr(), 0, count.data_ptr(), stream=stream.cuda_stream),
    }
    times = {k: [] for k in forms}
    for r in range(WARMUP + REPEATS):
        for k, f in forms.items():
            t = timed(stream, f)
            if r >= WARMUP:
                times[k].append(t)
    st = con.cpu().numpy()
    print(f"-- {title}: {batch} systems of {n} variables, {m} rows, {n_cs} constraints; per system {int((st[0] == 2).sum())} redundant, "
          f"{int((st[0] == 3).sum())} conflicting, rank {int(rank.cpu()[0])}, {int(count.cpu()[0])} underconstrained variables")
    for k, t in times.items():
        t = np.asarray(t)
        print(f"  {k:24s} {np.median(t) * 1e3:10.3f} ms ({t.min() * 1e3:.3f} .. {t.max() * 1e3:.3f})   {batch / np.median(t):14.0f} systems/s")
    sys.stdout.flush()


def main():
    import redundancy_ref as R

    if E.device_count() < 1:
        raise SystemExit("tools/redundancy_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print(__doc__.split("\n\n")[0].replace("\n", " "))
    print("%d warm-up and %d timed runs per form." % (WARMUP, REPEATS))
    src = open(os.path.join(ROOT, "ezpz_amd", "csrc", "redundancy.hip.hpp"), "rb").read()
    print("device:", torch.cuda.get_device_name(0), "| HIP", torch.version.hip, "| redundancy.hip.hpp sha256", hashlib.sha256(src).hexdigest()[:16])
    case = R.blocks(batch=1, lines=500)
    batch = 65536
    with torch.cuda.stream(stream):
        gen = torch.Generator(device="cuda").manual_seed(17)
        x = torch.rand((batch, case["n_vars"]), dtype=torch.float64, device="cuda", generator=gen) * 8.0 - 2.0
    workload(stream, "LANE, block system", case, batch, x)
    del x
    for title, npts, seed, batch in (("TEAM, workspace in LDS", 24, 5, 4096), ("TEAM, workspace in global memory", 150, 7, 64)):
        case = R.sketch(npts, seed, 0, 1)
        with torch.cuda.stream(stream):
            x = torch.from_numpy(np.repeat(case["x"][:1], batch, axis=0)).cuda()
        workload(stream, title, case, batch, x)


if __name__ == "__main__":
    main()
