"""The rate of the Sobol tolerance indices (ezpz_system_tolerance_sobol_device), printed as the text of
profiles/sobol_rate.txt: the run against what the library offered for the same numbers before, the share of a run that is not the
solves, and the reduction alone.

The systems and settings are those of tools/mc_rate.py (8 driven dimensions, normal, cut at 3 sigma; 8 reference dimensions; rounds
of 65536).  Per case:
  sobol        ezpz_system_tolerance_sobol_device: k + 2 sub-rounds a round, the sums' kernel, the closing kernel; stats, totals,
               sums, n_complete, var and the four index arrays read back
  host route   what the parent commit offers for the same numbers: the pick-freeze matrices built on the host with mc_sample, k + 2
               calls of solve_batch_params and measure with the answers brought back, numpy for the sums and the indices
  solves       k + 2 plain ezpz_system_solve_batch_params_device calls on params of the same shape, in the same rounds: what is
               left of `sobol` is the sampler, the copies of x0, the measurements, the reductions and the launches between them
  sums         ezpz_mc_sobol_sums_device alone on the kept rows of a run, and on synthetic rows at (k, m) = (32, 32)
No ratio is fixed in advance.  The host route draws NORMAL deviations with the host's log and cos: the same amount of work, not the
same bits; its indices are printed beside the run's.

Host clock around work that ends in a synchronise; WARMUP untimed runs of each form, then REPEATS timed runs, the forms alternating;
median (min .. max).

    python tools/sobol_rate.py > profiles/sobol_rate.txt
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
from ezpz_amd._lib import MC_STATS_DTYPE, MC_TOTALS_DTYPE, STATUS_DTYPE  # noqa: E402
from mc_rate import CHUNK, SIGMA, TRUNC, driven, measurements, systems, timed  # noqa: E402

WARMUP, REPEATS = 1, 5
SAMPLES = (65536, 1048576)
SEED, SEED_B = 1, 1 ^ 0x9E3779B97F4A7C15


def line(what, ts, samples, extra=""):
    ts = np.asarray(ts)
    print("   %-11s %10.3f ms (%.3f .. %.3f)  %12.0f samples/s%s" % (what, np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3,
                                                                  samples / np.median(ts), extra))
    sys.stdout.flush()


def numpy_indices(f, flags, ok, nominal):
    """first and total [m, k] of the rows by numpy: the complete-case rule per record, plain sums."""
    k, m = f.shape[1] - 2, f.shape[2]
    first, total = np.zeros((m, k)), np.zeros((m, k))
    for i in range(m):
        live = (ok != 0).all(axis=1) & ~((flags[:, :, i] & 1) != 0).any(axis=1) & np.isfinite(f[:, :, i]).all(axis=1)
        d = f[live][:, :, i] - nominal[i]
        dA, dB = d[:, 0], d[:, 1]
        var = np.concatenate([dA, dB]).var(ddof=1)
        for j in range(k):
            t = d[:, 2 + j] - dA
            with np.errstate(all="ignore"):
                first[i, j], total[i, j] = (dB * t).mean() / var, (t * t).mean() / 2.0 / var
    return first, total


def case(name, system, recs, g, samples, stream):
    pos, records = driven(recs), measurements(len(g))
    n, k, m = len(g), len(pos), len(records)
    solved, st, _ = system.solve_batch(g[None, :])
    assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
    own = recs["param"][pos].astype(np.float64)
    dists = [E.McDist.normal(float(s), TRUNC) for s in SIGMA * np.maximum(1.0, np.abs(own))]
    h = stream.cuda_stream
    with torch.cuda.stream(stream):
        x0 = torch.from_numpy(solved[0]).cuda()
        stats = torch.zeros(m * MC_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        totals = torch.zeros(MC_TOTALS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
        sums, var, first, total, first_var, total_var = f64(m, 4 + 4 * k), f64(m), f64(m, k), f64(m, k), f64(m, k), f64(m, k)
        n_complete = torch.zeros(m, dtype=torch.int64, device="cuda")
        kf, kflags, kok = f64(samples, k + 2, m), u8(samples, k + 2, m), u8(samples, k + 2)
        nominal_m = torch.from_numpy(system.measure(solved, records)[0]).cuda()
        sums_alone, n_alone = f64(m, 4 + 4 * k), torch.zeros(m, dtype=torch.int64, device="cuda")
        # the plain solves: one round's buffers, params of the run's shape
        rows = min(samples, CHUNK)
        params = torch.from_numpy(E.mc_sample(SEED, dists, own, 0, rows)).cuda()
        x_in, x_out = x0.repeat(rows, 1).contiguous(), f64(rows, n)
        status = u8(rows * STATUS_DTYPE.itemsize)
    result = {}

    def run(keep=False):
        kept = dict(keep_f_ptr=kf.data_ptr(), keep_flags_ptr=kflags.data_ptr(), keep_ok_ptr=kok.data_ptr()) if keep else {}
        with torch.cuda.stream(stream):
            system.tolerance_sobol_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), sums.data_ptr(),
                                          n_complete.data_ptr(), var.data_ptr(), first.data_ptr(), total.data_ptr(), first_var.data_ptr(),
                                          total_var.data_ptr(), seed=SEED, seed_b=SEED_B, chunk=CHUNK, stream=h, **kept)
            result["sobol"] = [t.cpu().numpy() for t in (stats, totals, sums, n_complete, var, first, total, first_var, total_var)]

    def solves():
        with torch.cuda.stream(stream):
            for first_sample in range(0, samples, CHUNK):
                count = min(CHUNK, samples - first_sample)
                for _ in range(k + 2):
                    system.solve_batch_params_device(x_in.data_ptr(), pos, params.data_ptr(), count, x_out.data_ptr(), status.data_ptr(), stream=h)

    def sums_only():
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_mc_sobol_sums_device(kf.data_ptr(), kflags.data_ptr(), kok.data_ptr(), nominal_m.data_ptr(), 0, samples, k, m, CHUNK,
                                                   sums_alone.data_ptr(), n_alone.data_ptr(), h)
            assert rc == 0, rc
            result["sums"] = sums_alone.cpu().numpy(), n_alone.cpu().numpy()

    def host_route():
        PA, PB = E.mc_sample(SEED, dists, own, 0, samples), E.mc_sample(SEED_B, dists, own, 0, samples)
        start = np.tile(solved[0], (samples, 1))
        f, flags, ok = np.zeros((samples, k + 2, m)), np.zeros((samples, k + 2, m), np.uint8), np.zeros((samples, k + 2), np.uint8)
        for r in range(k + 2):
            P = PA if r == 0 else PB if r == 1 else np.concatenate([PA[:, :r - 2], PB[:, r - 2:r - 1], PA[:, r - 1:]], axis=1)
            x, st, _ = system.solve_batch_params(start, pos, P)
            f[:, r], flags[:, r] = system.measure(x, records, want_flags=True)
            ok[:, r] = (st["converged"] != 0) & (st["n_unsatisfied"] == 0)
        result["host"] = numpy_indices(f, flags, ok, nominal_m.cpu().numpy())

    timed(lambda: run(keep=True))  # (the kept rows the sums alone run on; also a warm-up)
    forms = [run, solves, sums_only, host_route]
    for _ in range(WARMUP):
        for fn in forms:
            timed(fn)
    ts = [[] for _ in forms]
    for _ in range(REPEATS):
        for i, fn in enumerate(forms):
            ts[i].append(timed(fn))
    s = result["sobol"]
    assert s[2].tobytes() == result["sums"][0].tobytes(), "the run's sums are not the reduction alone on its kept rows"
    t_run, t_solves, t_sums, t_host = (np.median(v) for v in ts)
    rounds = (samples + CHUNK - 1) // CHUNK
    print("-- %s; %d samples, %d driven (normal, sigma %g x max(1, |value|), cut at %g sigma), %d reference dimensions, %d solves a sample, "
          "%d round(s) of %d" % (name, samples, k, SIGMA, TRUNC, m, k + 2, rounds, CHUNK))
    print("   ok (matrix A) %d of %d; complete per record %s" % (s[1].view(MC_TOTALS_DTYPE)["n_ok"][0], samples, s[3].tolist()))
    line("sobol", ts[0], samples)
    line("solves", ts[1], samples, "   the run less the solves: %.3f ms = %.1f%% of the run, %.1f us a round" %
         ((t_run - t_solves) * 1e3, 100.0 * (t_run - t_solves) / t_run, (t_run - t_solves) * 1e6 / rounds))
    line("sums", ts[2], samples, "   alone on the kept rows, its results read back")
    line("host route", ts[3], samples, "   sobol x%.1f" % (t_host / t_run))
    hf, ht = result["host"]
    with np.errstate(invalid="ignore"):
        se = np.sqrt(s[7])
    live = np.isfinite(s[5]).all(axis=1)
    print("   against the host route (its own NORMAL draws): max |first - host| = %.3e, max |total - host| = %.3e; largest standard error %.3e"
          % (np.max(np.abs(s[5][live] - hf[live])), np.max(np.abs(s[6][live] - ht[live])), np.nanmax(se[live]) if live.any() else float("nan")))
    for i in range(m):
        print("   [%d] var %.3e  first %s" % (i, s[4][i], " ".join("% .4f" % v for v in s[5][i])))
        print("       %s  total %s" % (" " * 13, " ".join("% .4f" % v for v in s[6][i])))
    sys.stdout.flush()


def sums_wide(stream, samples=65536, k=32, m=32):
    rng = np.random.default_rng(3)
    with torch.cuda.stream(stream):
        f = torch.from_numpy(rng.normal(size=(samples, k + 2, m))).cuda()
        nominal = torch.zeros(m, dtype=torch.float64, device="cuda")
        sums, n = torch.zeros((m, 4 + 4 * k), dtype=torch.float64, device="cuda"), torch.zeros(m, dtype=torch.int64, device="cuda")

    def go():
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_mc_sobol_sums_device(f.data_ptr(), None, None, nominal.data_ptr(), 0, samples, k, m, 0, sums.data_ptr(), n.data_ptr(),
                                                   stream.cuda_stream)
            assert rc == 0, rc
            sums.cpu()

    timed(go)
    ts = [timed(go) for _ in range(REPEATS)]
    print("-- the reduction alone at (k, m) = (%d, %d): %d samples of synthetic rows (%.0f MiB), %d sums, rounds of the library's choice"
          % (k, m, samples, samples * (k + 2) * m * 8 / 2 ** 20, m * (4 + 4 * k)))
    line("sums", ts, samples, "   %.1f GB/s of rows" % (samples * (k + 2) * m * 8 / np.median(ts) / 1e9))


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/sobol_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("Sobol tolerance indices (ezpz_system_tolerance_sobol_device) on", torch.cuda.get_device_name(0))
    print("host clock around work that ends in a synchronise; %d warm-up run(s) of each form, then %d timed runs, the forms alternating;"
          % (WARMUP, REPEATS))
    print("median (min .. max).  host route = mc_sample, k + 2 x (solve_batch_params, measure), numpy: what the parent commit offers.")
    for name, system, recs, g in systems():
        for samples in SAMPLES:
            case(name, system, recs, g, samples, stream)
    sums_wide(stream)


if __name__ == "__main__":
    main()
