"""The rate of the factorial effects (ezpz_system_tolerance_mc_factorial_device, ezpz_mc_factorial_device), printed as
the text of profiles/factorial_rate.txt: what the transform adds to a corner run, the run against the route that existed before, and
the transform alone.

The systems are those of tools/mc_rate.py; the driven dimensions are their parametrised constraints, evenly spread, as many as they
have up to 16, every one a CORNER of +-1e-3 x max(1, |value|); 8 reference dimensions; rounds of 65536.  Per case:
  factorial    ezpz_system_tolerance_mc_factorial_device: the corner run, every round's m, flags and ok copied into the plan's
               workspace, the transform behind the last round; stats, totals and the eight outputs but coef read back
  plain        ezpz_system_tolerance_mc_device on the same corners, stats and totals read back: this code is the parent commit's,
               unchanged, so the difference is what the factorial effects add
  host route   what the parent commit offers for the same numbers, end to end: System.tolerance_mc(keep=True) -- the rows to the
               host -- then a numpy Walsh-Hadamard transform per record and the sums by numpy
Then the transform alone, ezpz_mc_factorial_device on random rows of 8 records at kc of 12, 16 and 20, without and with coef, its
records read back.  The GB/s figure counts the bytes the kernels are built to move -- the rows once (N x (n_meas x 9 + 1)), the work
array written once by the gather, read and written once per strided launch, read once by the walk, and coef written where asked --
over the time, to put beside the row copy of profiles/row_stream_roof.txt (5.79 TB/s for rows streamed once by a kernel shaped for it).
No ratio is fixed in advance.

Host clock around work that ends in a synchronise; WARMUP untimed runs of each form, then REPEATS timed runs, the forms alternating;
median (min .. max).

    python tools/factorial_rate.py > profiles/factorial_rate.txt
"""
import os
import sys

import numpy as np
import torch  # (before the library: torch brings its own HIP runtime and must be the first to load one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ezpz_amd as E  # noqa: E402
from ezpz_amd._lib import MC_FACTORIAL_DTYPE, MC_STATS_DTYPE, MC_TOTALS_DTYPE  # noqa: E402
from mc_rate import CHUNK, SIGMA, measurements, systems, timed  # noqa: E402

WARMUP, REPEATS = 1, 5
MAX_CORNERS = 16
SEED = 1
ALONE_KC, ALONE_MEAS = (12, 16, 20), 8
NAMES = ("info", "main", "pair", "ss_order", "ss_total", "first", "total", "coef")


def line(what, ts, samples, extra=""):
    ts = np.asarray(ts)
    print("   %-11s %10.3f ms (%.3f .. %.3f)  %12.0f corners/s%s" % (what, np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3,
                                                                  samples / np.median(ts), extra))
    sys.stdout.flush()


def out_bytes(kc, m):
    return [m * MC_FACTORIAL_DTYPE.itemsize, m * kc * 8, m * kc * kc * 8, m * (kc + 1) * 8, m * kc * 8, m * kc * 8, m * kc * 8, (m << kc) * 8]


def numpy_factorial(rows, nominal):
    """(main [n_meas, kc], var [n_meas]) by a numpy Walsh-Hadamard transform per record: the route that existed before."""
    N, n_meas = rows.shape
    kc = N.bit_length() - 1
    w = np.ascontiguousarray((rows - nominal).T)
    for level in range(kc):
        h = 1 << level
        v = w.reshape(n_meas, N // (2 * h), 2, h)
        lo, hi = v[:, :, 0, :].copy(), v[:, :, 1, :].copy()
        v[:, :, 0, :] = lo + hi
        v[:, :, 1, :] = hi - lo
    coef = w / N
    return coef[:, [1 << c for c in range(kc)]], (coef[:, 1:] ** 2).sum(axis=1)


def driven_corners(recs):
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    return np.ascontiguousarray(pos[np.linspace(0, len(pos) - 1, min(MAX_CORNERS, len(pos))).astype(int)])


def case(name, system, recs, g, stream):
    pos, records = driven_corners(recs), measurements(len(g))
    kc, m = len(pos), len(records)
    samples = 1 << kc
    solved, st, _ = system.solve_batch(g[None, :])
    assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
    own = recs["param"][pos].astype(np.float64)
    dists = [E.McDist.corner(-float(s), float(s)) for s in SIGMA * np.maximum(1.0, np.abs(own))]
    h = stream.cuda_stream
    with torch.cuda.stream(stream):
        x0 = torch.from_numpy(solved[0]).cuda()
        u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")  # noqa: E731
        stats, totals = u8(m * MC_STATS_DTYPE.itemsize), u8(MC_TOTALS_DTYPE.itemsize)
        outs = [u8(n) for n in out_bytes(kc, m)[:7]]
    ptrs = {"factorial_%s_ptr" % n: o.data_ptr() for n, o in zip(NAMES, outs)}
    result = {}

    def run():
        with torch.cuda.stream(stream):
            system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), seed=SEED, chunk=CHUNK,
                                       stream=h, factorial=True, **ptrs)
            result["run"] = [t.cpu().numpy() for t in [stats, totals] + outs]

    def plain():
        with torch.cuda.stream(stream):
            system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), seed=SEED, chunk=CHUNK,
                                       stream=h)
            result["plain"] = [t.cpu().numpy() for t in (stats, totals)]

    def host_route():
        res = system.tolerance_mc(solved[0], pos, dists, records, samples, seed=SEED, chunk=CHUNK, keep=True)
        result["host"] = numpy_factorial(res.m, res.stats["nominal"])

    forms = [run, plain, host_route]
    for _ in range(WARMUP):
        for fn in forms:
            timed(fn)
    ts = [[] for _ in forms]
    for _ in range(REPEATS):
        for i, fn in enumerate(forms):
            ts[i].append(timed(fn))
    info = result["run"][2].view(MC_FACTORIAL_DTYPE)
    main = result["run"][3].view(np.float64).reshape(m, kc)
    first, total = (result["run"][at].view(np.float64).reshape(m, kc) for at in (7, 8))
    assert result["run"][0].tobytes() == result["plain"][0].tobytes(), "the run's stats are not the plain run's"
    host_main, host_var = result["host"]
    t_run, t_plain, t_host = (np.median(v) for v in ts)
    rounds = (samples + CHUNK - 1) // CHUNK
    print("-- %s; %d CORNER dimensions (+-%g x max(1, |value|)) = %d corners, %d reference dimensions, %d round(s) of %d"
          % (name, kc, SIGMA, samples, m, rounds, CHUNK))
    print("   ok %d of %d; complete records %d of %d; workspace %.1f MiB of rows + %.1f MiB of work array"
          % (result["run"][1].view(MC_TOTALS_DTYPE)["n_ok"][0], samples, int(info["complete"].sum()), m, samples * (m * 9 + 1) / 2 ** 20,
             samples * m * 8 / 2 ** 20))
    line("factorial", ts[0], samples)
    line("plain", ts[1], samples, "   the factorial effects add %.3f ms = %.1f%% of the plain run" % ((t_run - t_plain) * 1e3, 100.0 * (t_run - t_plain) / t_plain))
    with np.errstate(invalid="ignore"):
        print_worst = (np.nanmax(np.abs(main - host_main)), np.nanmax(np.abs(info["var"] - host_var)))
    line("host route", ts[2], samples, "   factorial x%.1f; max |main - numpy's| = %.1e, max |var - numpy's| = %.1e" % ((t_host / t_run,) + print_worst))
    for i in range(m):
        print("   [%d] var % .3e  sum(first) %.6f  max(total - first) %.6f  corner_hi %#x  m_hi % .6f  max % .6f" %
              (i, info["var"][i], first[i].sum(), (total[i] - first[i]).max(), info["corner_hi"][i], info["m_hi"][i],
               result["run"][0].view(MC_STATS_DTYPE)["max"][i]))
    sys.stdout.flush()


def alone(kc, with_coef, stream):
    m, N = ALONE_MEAS, 1 << kc
    rng = np.random.default_rng(kc)
    h = stream.cuda_stream
    with torch.cuda.stream(stream):
        rows = torch.from_numpy(rng.normal(size=(N, m))).cuda()
        flags = torch.zeros((N, m), dtype=torch.uint8, device="cuda")
        ok = torch.ones(N, dtype=torch.uint8, device="cuda")
        nominal = torch.zeros(m, dtype=torch.float64, device="cuda")
        outs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in out_bytes(kc, m)]
    args = [rows.data_ptr(), flags.data_ptr(), ok.data_ptr(), nominal.data_ptr(), kc, m] + [o.data_ptr() for o in outs[:7]] + [outs[7].data_ptr() if with_coef else None]

    def call():
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_mc_factorial_device(*args, h)
            assert rc == 0, rc
            outs[0].cpu()

    for _ in range(WARMUP + 1):
        timed(call)
    ts = np.asarray([timed(call) for _ in range(REPEATS)])
    strided = 0 if kc <= 7 else (kc - 7 + 6) // 7
    moved = N * (m * 9 + 1) + N * m * 8 * (1 + 2 * strided + 1 + (1 if with_coef else 0))
    print("   kc %2d, %d records, %s coef: %9.3f ms (%.3f .. %.3f)   %d strided launch(es); %.1f MiB moved = %.1f GB/s" %
          (kc, m, "with   " if with_coef else "without", np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3, strided, moved / 2 ** 20,
           moved / np.median(ts) / 1e9))
    sys.stdout.flush()


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/factorial_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("Factorial effects (ezpz_system_tolerance_mc_factorial_device) on", torch.cuda.get_device_name(0))
    print("host clock around work that ends in a synchronise; %d warm-up run(s) of each form, then %d timed runs, the forms alternating;"
          % (WARMUP, REPEATS))
    print("median (min .. max).  host route = tolerance_mc(keep=True), the rows to the host, a numpy Walsh-Hadamard: what the parent commit offers.")
    for name, system, recs, g in systems():
        case(name, system, recs, g, stream)
    print("-- the transform alone (ezpz_mc_factorial_device), random rows, its records read back")
    for kc in ALONE_KC:
        for with_coef in (False, True):
            alone(kc, with_coef, stream)


if __name__ == "__main__":
    main()
