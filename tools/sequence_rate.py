"""What the low-discrepancy draws (EZPZ_MC_SEQUENCE) cost and buy on the device, printed as the text of
profiles/sequence_rate.txt.  Four parts, each from child processes of this tool (the sampler's variant is read once per process):

  kernels   the sampler kernel alone, 65 536 samples x 8 dimensions: its average duration in a `rocprofv3 --kernel-trace --stats`
            trace of a child that does nothing but RUNS runs of an 8-variable all-Fixed system -- plain draws (mc_sample_kernel),
            flagged UNIFORM and flagged NORMAL (cut at 3 sigma) by the walk with its table in LDS, the walk on constant memory
            (EZPZ_MC_SEQUENCE_KERNEL=const) and the direct evaluation (=direct).  Kernel time, from the trace; nothing else here is.
  runs      1 048 576 samples on the systems of tools/mc_rate.py (8 driven dimensions, normal, cut at 3 sigma; 8 reference
            dimensions; rounds of 65 536), plain against flagged, stats and totals read back.  Host clock around work that ends in a
            synchronise; WARMUP untimed runs of each form, then REPEATS timed runs, the forms alternating; median (min .. max).
  parent    with --parent-lib: the same plain runs on another build of the library (the parent commit's), its children alternating
            with this build's.  `draw()` gained branches; an unflagged list launches the kernel it launched before.
  accuracy  through real solves: the point at (1, 0) of tests/test_gpu_sobol.py, x = 1 + u, y = v, u uniform on +-0.25 and v on
            +-0.35; the RMS error over 16 seeds of mean and std of its distance from the origin at 1024, 4096 and 16 384 samples,
            plain against flagged, the truth from 2^20 flagged samples of another seed.
No ratio is fixed in advance.

    python tools/sequence_rate.py [--parent-lib PATH] [--scratch DIR] > profiles/sequence_rate.txt
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, REPEATS, RUNS = 1, 5, 20
KERNEL_SAMPLES, KERNEL_DIMS = 65536, 8
RUN_SAMPLES = 1048576
SEED = 1
LISTS = ("plain uniform", "plain normal", "flagged uniform", "flagged normal")
VARIANTS = (("walk, table in LDS", ""), ("walk, constant memory", "const"), ("direct evaluation", "direct"))


def _imports():
    import numpy as np
    import torch  # (before the library: torch brings its own HIP runtime and must be the first to load one)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ezpz_amd as E
    return np, torch, E


def _list(E, name, k, sigma=None, trunc=3.0):
    flagged = name.startswith("flagged")
    kw = dict(sequence=True) if flagged else {}
    if name.endswith("uniform"):
        return [E.McDist.uniform(-0.01, 0.01, **kw)] * k
    return [E.McDist.normal(0.01 if sigma is None else float(s), trunc, **kw) for s in ([0.01] * k if sigma is None else sigma)]


def child_kernels(name):
    """RUNS runs of 65 536 samples x 8 dimensions on an all-Fixed system: under the profiler."""
    np, torch, E = _imports()
    from oracle import oracle as O
    k = KERNEL_DIMS
    x0 = np.arange(k, dtype=np.float64)
    system = E.System(O.stack([O.fixed(v, float(x0[v])) for v in range(k)]), k)
    for _ in range(RUNS + 1):
        system.tolerance_mc(x0, list(range(k)), _list(E, name, k), O.stack([O.fixed(0, 0.0)]), KERNEL_SAMPLES, seed=SEED, chunk=KERNEL_SAMPLES)


def child_runs(flagged_too):
    """{system: {form: [seconds]}} as one JSON line."""
    np, torch, E = _imports()
    from ezpz_amd._lib import MC_STATS_DTYPE, MC_TOTALS_DTYPE
    from mc_rate import CHUNK, SIGMA, TRUNC, driven, measurements, systems, timed
    stream, out = torch.cuda.Stream(), {}
    for name, system, recs, g in systems():
        pos, records = driven(recs), measurements(len(g))
        m = len(records)
        solved, st, _ = system.solve_batch(g[None, :])
        assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
        sigma = SIGMA * np.maximum(1.0, np.abs(recs["param"][pos].astype(np.float64)))
        with torch.cuda.stream(stream):
            x0 = torch.from_numpy(solved[0]).cuda()
            stats = torch.zeros(m * MC_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            totals = torch.zeros(MC_TOTALS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        result = {}

        def form(which):
            dists = _list(E, which + " normal", len(pos), sigma, TRUNC)

            def run():
                with torch.cuda.stream(stream):
                    system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, RUN_SAMPLES, stats.data_ptr(), totals.data_ptr(), seed=SEED,
                                               chunk=CHUNK, stream=stream.cuda_stream)
                    result[which] = np.frombuffer(stats.cpu().numpy().tobytes(), MC_STATS_DTYPE), np.frombuffer(totals.cpu().numpy().tobytes(), MC_TOTALS_DTYPE)
            return run

        forms = {"plain": form("plain")}
        if flagged_too:
            forms["flagged"] = form("flagged")
        for _ in range(WARMUP):
            for fn in forms.values():
                timed(fn)
        ts = {which: [] for which in forms}
        for _ in range(REPEATS):
            for which, fn in forms.items():
                ts[which].append(timed(fn))
        out[name] = dict(times=ts, ok={w: int(r[1]["n_ok"][0]) for w, r in result.items()},
                         mean={w: float(r[0]["mean"][0]) for w, r in result.items()}, std={w: float(np.sqrt(r[0]["var"][0])) for w, r in result.items()})
    print("RESULT " + json.dumps(dict(device=torch.cuda.get_device_name(0), systems=out)))


def child_accuracy():
    np, torch, E = _imports()
    from oracle import oracle as O
    system = E.System(O.stack([O.fixed(0, 1.0), O.fixed(1, 0.0), O.fixed(2, 0.5), O.fixed(3, 0.0), O.fixed(4, 0.0)]), 5)
    x0, pos = np.array([1.0, 0.0, 0.5, 0.0, 0.0]), [0, 1, 2]
    records = O.stack([O.distance((3, 4), (0, 1), 0.0)])

    def run(flagged, samples, seed):
        kw = dict(sequence=True) if flagged else {}
        dists = [E.McDist.uniform(-0.25, 0.25, **kw), E.McDist.uniform(-0.35, 0.35, **kw), E.McDist.uniform(-0.2, 0.2, **kw)]
        res = system.tolerance_mc(x0, pos, dists, records, samples, seed=seed)
        assert res.n_ok == samples
        return float(res.mean[0]), float(res.std[0])

    truth = run(True, 1 << 20, 0xABCDEF)
    rows = []
    for samples in (1024, 4096, 16384):
        err = {}
        for flagged in (False, True):
            got = np.array([run(flagged, samples, 1000 + s) for s in range(16)])
            err[flagged] = np.sqrt(np.mean((got - np.array(truth)[None, :]) ** 2, axis=0))
        rows.append(dict(samples=samples, plain=err[False].tolist(), flagged=err[True].tolist()))
    print("RESULT " + json.dumps(dict(truth=truth, rows=rows)))


def spawn(args, env=None, profile_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", profile_dir, "--"] + cmd
    p = subprocess.run(cmd, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("child %s failed with %d" % (" ".join(args), p.returncode))
    for ln in p.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    return None


def sampler_row(profile_dir):
    """(kernel name, calls, average ns, min ns, max ns) of the sampler kernel in the trace's statistics."""
    for path in glob.glob(os.path.join(profile_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "mc_sample" in row["Name"]:
                return row["Name"].split("(")[0].replace("ezpz::mc::", "").replace("void ", ""), int(row["Calls"]), float(row["AverageNs"]), float(row["MinNs"]), float(row["MaxNs"])
    raise SystemExit("no sampler kernel in the trace under " + profile_dir)


def fmt(ts, samples):
    import numpy as np
    ts = np.asarray(ts)
    return "%10.3f ms (%.3f .. %.3f)  %12.0f samples/s" % (np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3, samples / np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("kernels", "runs", "runs-plain", "accuracy"))
    ap.add_argument("--list", default=LISTS[0])
    ap.add_argument("--parent-lib")
    ap.add_argument("--scratch")
    a = ap.parse_args()
    if a.child == "kernels":
        return child_kernels(a.list)
    if a.child in ("runs", "runs-plain"):
        return child_runs(a.child == "runs")
    if a.child == "accuracy":
        return child_accuracy()
    import numpy as np
    scratch = a.scratch or tempfile.mkdtemp(prefix="sequence_rate_")
    first = spawn(["--child", "runs"])
    print("Low-discrepancy draws of the Monte-Carlo entries (EZPZ_MC_SEQUENCE) on", first["device"])
    print("-- the sampler kernel alone: %d samples x %d dimensions, average kernel time over %d launches (min .. max) in a rocprofv3 kernel trace"
          % (KERNEL_SAMPLES, KERNEL_DIMS, RUNS + 1))
    n = 0
    for name in LISTS:
        for label, env in (VARIANTS if name.startswith("flagged") else VARIANTS[:1]):
            d = os.path.join(scratch, "trace%d" % n)
            n += 1
            spawn(["--child", "kernels", "--list", name], env={"EZPZ_MC_SEQUENCE_KERNEL": env} if env else None, profile_dir=d)
            kernel, calls, avg, lo, hi = sampler_row(d)
            print("   %-16s %-22s %9.2f us (%.2f .. %.2f)  %7.2f G draws/s   %s, %d launches"
                  % (name, label if name.startswith("flagged") else "", avg / 1e3, lo / 1e3, hi / 1e3, KERNEL_SAMPLES * KERNEL_DIMS / avg, kernel, calls))
            sys.stdout.flush()
    print("-- runs of %d samples, 8 driven dimensions (normal, cut at 3 sigma), 8 reference dimensions, rounds of 65536; host clock around work that"
          % RUN_SAMPLES)
    print("   ends in a synchronise; %d warm-up run(s) of each form, then %d timed runs, the forms alternating; median (min .. max)" % (WARMUP, REPEATS))
    for name, r in first["systems"].items():
        print("   " + name)
        for which in ("plain", "flagged"):
            print("      %-8s %s   ok %d, first reference dimension: mean %.9g std %.6g"
                  % (which, fmt(r["times"][which], RUN_SAMPLES), r["ok"][which], r["mean"][which], r["std"][which]))
        print("      flagged / plain = %.3f" % (np.median(r["times"]["flagged"]) / np.median(r["times"]["plain"])))
    if a.parent_lib:
        print("-- the plain runs again, this build and the parent commit's build in alternating processes (%d timed runs each)" % REPEATS)
        for turn in range(2):
            for label, env in (("this build", None), ("parent", {"EZPZ_AMD_LIB": os.path.abspath(a.parent_lib), "EZPZ_AMD_NO_BUILD": "1"})):
                r = spawn(["--child", "runs-plain"], env=env)
                for name, s in r["systems"].items():
                    print("   %-10s turn %d  %s   %s" % (label, turn, fmt(s["times"]["plain"], RUN_SAMPLES), name))
                sys.stdout.flush()
    acc = spawn(["--child", "accuracy"])
    print("-- through real solves: the distance from the origin of the point at (1, 0), x = 1 + u, y = v, u uniform on +-0.25, v on +-0.35;")
    print("   truth from 2^20 flagged samples of another seed: mean %.12g std %.12g; RMS error over 16 seeds" % tuple(acc["truth"]))
    print("   samples    mean: plain      flagged    ratio     std: plain      flagged    ratio")
    for row in acc["rows"]:
        p, f = row["plain"], row["flagged"]
        print("   %7d    %12.3e %12.3e %6.1f x    %12.3e %12.3e %6.1f x" % (row["samples"], p[0], f[0], p[0] / f[0], p[1], f[1], p[1] / f[1]))


if __name__ == "__main__":
    main()
