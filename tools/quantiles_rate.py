"""The rate of the Monte-Carlo quantiles (ezpz_system_tolerance_mc_quantiles_device, ezpz_mc_quantiles_device),
printed as the text of profiles/quantiles_rate.txt: what the quantiles add to a run, the run against the route that existed before,
and the selection alone.

The systems and settings are those of tools/mc_rate.py and tools/sobol_rate.py (8 driven dimensions, normal, cut at 3 sigma; 8
reference dimensions; rounds of 65536); 5 probabilities -- 0.00135, 0.025, 0.5, 0.975, 0.99865 -- with z = 3.  Per case:
  quantiles    ezpz_system_tolerance_mc_quantiles_device: the run, every round's m, flags and ok copied into the plan's workspace, the
               selection behind the last round; stats, totals and the records read back
  plain        ezpz_system_tolerance_mc_device at the same samples, stats and totals read back: this code is the parent commit's,
               unchanged, so the difference is what the quantiles add
  host route   what the parent commit offers for the same numbers, end to end: System.tolerance_mc(keep=True) -- the rows to the
               host -- then numpy.partition per record at the same ranks
  select       ezpz_mc_quantiles_device alone on the kept rows of a run, its records read back.  Every one of its 8 digit passes
               reads every row: samples x (n_meas x 9 + 1) bytes; the GB/s figure is that times 8 over the time, to put beside the
               row copy of profiles/row_stream_roof.txt (5.79 TB/s for rows streamed once by a kernel shaped for it)
No ratio is fixed in advance.

Host clock around work that ends in a synchronise; WARMUP untimed runs of each form, then REPEATS timed runs, the forms alternating;
median (min .. max).

    python tools/quantiles_rate.py > profiles/quantiles_rate.txt
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
from ezpz_amd._lib import CMcQuantileConfig, MC_QUANTILE_DTYPE, MC_STATS_DTYPE, MC_TOTALS_DTYPE  # noqa: E402
from mc_rate import CHUNK, SIGMA, TRUNC, driven, measurements, systems, timed  # noqa: E402

import ctypes as C  # noqa: E402

WARMUP, REPEATS = 1, 5
SAMPLES = (65536, 1048576)
SEED = 1
PROBS, Z = [0.00135, 0.025, 0.5, 0.975, 0.99865], 3.0


def line(what, ts, samples, extra=""):
    ts = np.asarray(ts)
    print("   %-11s %10.3f ms (%.3f .. %.3f)  %12.0f samples/s%s" % (what, np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3,
                                                                  samples / np.median(ts), extra))
    sys.stdout.flush()


def numpy_quantiles(m, flags, ok, records):
    """value [n_meas, n_q] by numpy.partition at the ranks of `records`: the valid values per record, the order statistics at rank,
    rank + 1, rank_lo and rank_hi, the interpolation."""
    out = np.zeros(records.shape)
    for i in range(m.shape[1]):
        v = m[(ok != 0) & ((flags[:, i] & 1) == 0) & np.isfinite(m[:, i]), i]
        r = records[i]
        n = len(v)
        if n == 0:
            out[i] = np.nan
            continue
        hi = np.minimum(r["rank"] + 1, n - 1)
        ranks = np.unique(np.concatenate([r["rank"], hi, r["rank_lo"], r["rank_hi"]]).astype(np.int64))
        part = np.partition(v, ranks)
        lo_v, hi_v = part[r["rank"].astype(np.int64)], part[hi.astype(np.int64)]
        out[i] = np.where(r["frac"] == 0.0, lo_v, lo_v + r["frac"] * (hi_v - lo_v))
    return out


def case(name, system, recs, g, samples, stream):
    pos, records = driven(recs), measurements(len(g))
    k, m, n_q = len(pos), len(records), len(PROBS)
    solved, st, _ = system.solve_batch(g[None, :])
    assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
    own = recs["param"][pos].astype(np.float64)
    dists = [E.McDist.normal(float(s), TRUNC) for s in SIGMA * np.maximum(1.0, np.abs(own))]
    h = stream.cuda_stream
    probs = np.asarray(PROBS)
    qc = CMcQuantileConfig(Z, 0)
    with torch.cuda.stream(stream):
        x0 = torch.from_numpy(solved[0]).cuda()
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
        stats, totals = u8(m * MC_STATS_DTYPE.itemsize), u8(MC_TOTALS_DTYPE.itemsize)
        quant, quant_alone = u8(m * n_q * MC_QUANTILE_DTYPE.itemsize), u8(m * n_q * MC_QUANTILE_DTYPE.itemsize)
        km, kflags, kok = torch.zeros((samples, m), dtype=torch.float64, device="cuda"), u8(samples, m), u8(samples)
    result = {}

    def run(keep=False):
        kept = dict(keep_m_ptr=km.data_ptr(), keep_flags_ptr=kflags.data_ptr(), keep_ok_ptr=kok.data_ptr()) if keep else {}
        with torch.cuda.stream(stream):
            system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), seed=SEED, chunk=CHUNK,
                                       stream=h, quantiles=PROBS, quantile_z=Z, quantiles_ptr=quant.data_ptr(), **kept)
            result["run"] = [t.cpu().numpy() for t in (stats, totals, quant)]

    def plain():
        with torch.cuda.stream(stream):
            system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), seed=SEED, chunk=CHUNK,
                                       stream=h)
            result["plain"] = [t.cpu().numpy() for t in (stats, totals)]

    def select():
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_mc_quantiles_device(km.data_ptr(), kflags.data_ptr(), kok.data_ptr(), samples, m, probs.ctypes.data, n_q,
                                                  C.byref(qc), quant_alone.data_ptr(), h)
            assert rc == 0, rc
            result["select"] = quant_alone.cpu().numpy()

    def host_route():
        res = system.tolerance_mc(solved[0], pos, dists, records, samples, seed=SEED, chunk=CHUNK, keep=True)
        result["host"] = numpy_quantiles(res.m, res.flags, res.ok, result["run"][2].view(MC_QUANTILE_DTYPE).reshape(m, n_q))

    timed(lambda: run(keep=True))  # (the kept rows the selection alone runs on; also a warm-up)
    forms = [run, plain, select, host_route]
    for _ in range(WARMUP):
        for fn in forms:
            timed(fn)
    ts = [[] for _ in forms]
    for _ in range(REPEATS):
        for i, fn in enumerate(forms):
            ts[i].append(timed(fn))
    q = result["run"][2].view(MC_QUANTILE_DTYPE).reshape(m, n_q)
    assert result["run"][0].tobytes() == result["plain"][0].tobytes(), "the run's stats are not the plain run's"
    assert result["run"][2].tobytes() == result["select"].tobytes(), "the run's quantiles are not the selection alone on its kept rows"
    with np.errstate(invalid="ignore"):
        worst = np.nanmax(np.abs(q["value"] - result["host"]))
    t_run, t_plain, t_select, t_host = (np.median(v) for v in ts)
    rounds = (samples + CHUNK - 1) // CHUNK
    per_pass = samples * (m * 9 + 1)
    print("-- %s; %d samples, %d driven (normal, sigma %g x max(1, |value|), cut at %g sigma), %d reference dimensions, %d probabilities, "
          "z = %g, %d round(s) of %d" % (name, samples, k, SIGMA, TRUNC, m, n_q, Z, rounds, CHUNK))
    print("   ok %d of %d; valid per record %s; workspace %.1f MiB" % (result["run"][1].view(MC_TOTALS_DTYPE)["n_ok"][0], samples,
                                                                        q["n_valid"][:, 0].tolist(), per_pass / 2 ** 20))
    line("quantiles", ts[0], samples)
    line("plain", ts[1], samples, "   the quantiles add %.3f ms = %.1f%% of the plain run, %.1f us a round" %
         ((t_run - t_plain) * 1e3, 100.0 * (t_run - t_plain) / t_plain, (t_run - t_plain) * 1e6 / rounds))
    line("select", ts[2], samples, "   alone on the kept rows, its records read back; 8 passes x %.1f MiB = %.1f GB/s" %
         (per_pass / 2 ** 20, 8 * per_pass / t_select / 1e9))
    line("host route", ts[3], samples, "   quantiles x%.1f; max |value - numpy.partition's| = %.1e" % (t_host / t_run, worst))
    for i in range(m):
        print("   [%d] value %s" % (i, " ".join("% .6f" % v for v in q["value"][i])))
        print("       band  %s" % " ".join("[% .6f % .6f]" % (a, b) for a, b in zip(q["band_lo"][i], q["band_hi"][i])))
    sys.stdout.flush()


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/quantiles_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("Monte-Carlo quantiles (ezpz_system_tolerance_mc_quantiles_device) on", torch.cuda.get_device_name(0))
    print("host clock around work that ends in a synchronise; %d warm-up run(s) of each form, then %d timed runs, the forms alternating;"
          % (WARMUP, REPEATS))
    print("median (min .. max).  host route = tolerance_mc(keep=True), the rows to the host, numpy.partition: what the parent commit offers.")
    print("probabilities", PROBS)
    for name, system, recs, g in systems():
        for samples in SAMPLES:
            case(name, system, recs, g, samples, stream)


if __name__ == "__main__":
    main()
