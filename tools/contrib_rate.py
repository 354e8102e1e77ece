"""The rate of the tolerance contributors (ezpz_system_tolerance_mc_contrib_device), printed as the text of
profiles/contributors_rate.txt: what the moments add to a Monte-Carlo run, and the run against what the library offered for the
same answer before.

The systems and settings are those of tools/mc_rate.py (8 driven dimensions, normal, cut at 3 sigma; 8 reference dimensions; rounds
of 65536), plus one case with K = 64 (32 driven, 32 reference dimensions) on the connected sketch.  Per case:
  contrib      ezpz_system_tolerance_mc_contrib_device: the run, the moments' round and the closing kernel; stats, totals, info,
               cov, beta, contrib, r2 and dropped read back
  plain        (a) ezpz_system_tolerance_mc_device on the same inputs -- the code path of the parent commit: what the moments add
               is the difference
  keep + numpy (b) what the parent commit offers for the same answer: System.tolerance_mc(keep=True) -- every sample's params
               and m to the host -- then numpy.cov and numpy.linalg.lstsq (with an intercept) over the complete samples
  moments      ezpz_mc_moments_device alone on the kept samples of a run, in the same rounds
No ratio is fixed in advance.  Per reference dimension the tool prints beta beside D of measure_response at the nominal point
(param_sensitivity with lambda 1e-9): reported, not asserted.  On the block system it also prints, for the horizontal distances, how
far r2 is from 1.

Host clock around work that ends in a synchronise; WARMUP untimed runs of each form, then REPEATS timed runs, the forms alternating;
median (min .. max).

    python tools/contrib_rate.py > profiles/contributors_rate.txt
"""
import os
import sys
import time

import numpy as np
import torch  # (before the library: torch brings its own HIP runtime and must be the first to load one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ezpz_amd as E  # noqa: E402
from ezpz_amd._lib import MC_MOMENTS_INFO_DTYPE, MC_STATS_DTYPE, MC_TOTALS_DTYPE  # noqa: E402
from mc_rate import CHUNK, SIGMA, TRUNC, driven, measurements, systems, timed  # noqa: E402
from oracle import oracle as O  # noqa: E402

WARMUP, REPEATS, HOST_REPEATS = 1, 5, 5
SAMPLES = (65536, 1048576)
LAMBDA = 1e-9


def line(what, ts, samples, extra=""):
    ts = np.asarray(ts)
    print("   %-13s %10.3f ms (%.3f .. %.3f)  %12.0f samples/s%s" % (what, np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3,
                                                                    samples / np.median(ts), extra))
    sys.stdout.flush()


def wide(recs, n):
    """32 driven dimensions and 32 reference dimensions of a sketch: K = 64."""
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    pos = np.ascontiguousarray(pos[np.linspace(0, len(pos) - 1, min(32, len(pos))).astype(int)])
    pts = n // 2
    pt = lambda i: (2 * i, 2 * i + 1)  # noqa: E731
    pairs = [(i, (i + 1 + pts // 2) % pts) for i in range(64 - len(pos))]
    records = O.stack([(O.distance if i % 2 else O.horizontal_distance)(pt(a), pt(b), 0.0) for i, (a, b) in enumerate(pairs)])
    return pos, records


def case(name, system, recs, g, samples, stream, pos, records, show):
    k, n_meas = len(pos), len(records)
    K = k + n_meas
    solved, st, _ = system.solve_batch(g[None, :])
    assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
    own = recs["param"][pos].astype(np.float64)
    sigma = SIGMA * np.maximum(1.0, np.abs(own))
    dists = [E.McDist.normal(float(s), TRUNC) for s in sigma]
    h = stream.cuda_stream
    entries = K + K * (K + 1) // 2
    with torch.cuda.stream(stream):
        x0 = torch.from_numpy(solved[0]).cuda()
        stats = torch.zeros(n_meas * MC_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        totals = torch.zeros(MC_TOTALS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
        moments, cov, beta, contrib, r2 = f64(entries), f64(K, K), f64(n_meas, k), f64(n_meas, k), f64(n_meas)
        info, dropped = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        kp, km = f64(samples, k), f64(samples, n_meas)
        kf, ko = torch.zeros((samples, n_meas), dtype=torch.uint8, device="cuda"), torch.zeros(samples, dtype=torch.uint8, device="cuda")
        nominal_p = torch.from_numpy(own).cuda()
        nominal_m = torch.from_numpy(system.measure(solved, records)[0]).cuda()
        moments_alone, info_alone = f64(entries), torch.zeros(2, dtype=torch.int64, device="cuda")
    result = {}

    def run(with_contrib, keep=False):
        extra = dict(moments_ptr=moments.data_ptr(), info_ptr=info.data_ptr(), cov_ptr=cov.data_ptr(), beta_ptr=beta.data_ptr(),
                     contrib_ptr=contrib.data_ptr(), r2_ptr=r2.data_ptr(), dropped_ptr=dropped.data_ptr()) if with_contrib else {}
        kept = dict(keep_params_ptr=kp.data_ptr(), keep_m_ptr=km.data_ptr(), keep_flags_ptr=kf.data_ptr(), keep_ok_ptr=ko.data_ptr()) if keep else {}
        with torch.cuda.stream(stream):
            system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), seed=1, chunk=CHUNK,
                                       stream=h, **extra, **kept)
            out = [stats.cpu().numpy().view(MC_STATS_DTYPE), totals.cpu().numpy().view(MC_TOTALS_DTYPE)]
            if with_contrib:
                out += [t.cpu().numpy() for t in (info, cov, beta, contrib, r2, dropped, moments)]
        result["contrib" if with_contrib else "plain"] = out

    def moments_only():
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_mc_moments_device(kp.data_ptr(), km.data_ptr(), kf.data_ptr(), ko.data_ptr(), nominal_p.data_ptr(), nominal_m.data_ptr(),
                                                samples, k, n_meas, CHUNK, moments_alone.data_ptr(), info_alone.data_ptr(), h)
            assert rc == 0, rc
            result["moments"] = moments_alone.cpu().numpy(), info_alone.cpu().numpy()

    def keep_numpy():
        res = system.tolerance_mc(solved[0], pos, dists, records, samples, seed=1, chunk=CHUNK, keep=True)
        done = (res.ok != 0) & ~((res.flags & 1) != 0).any(axis=1) & np.isfinite(res.m).all(axis=1)
        p, y = res.params[done], res.m[done]
        c = np.cov(np.concatenate([p, y], axis=1).T)
        coef, *_ = np.linalg.lstsq(np.concatenate([p, np.ones((len(p), 1))], axis=1), y, rcond=None)
        result["numpy"] = c, coef[:-1].T

    timed(lambda: run(True, keep=True))  # (the kept samples the moments alone run on; also a warm-up)
    forms = [lambda: run(True), lambda: run(False), moments_only]
    for _ in range(WARMUP):
        for f in forms:
            timed(f)
    ts = [[] for _ in forms]
    for _ in range(REPEATS):
        for i, f in enumerate(forms):
            ts[i].append(timed(f))
    timed(keep_numpy)
    th = [timed(keep_numpy) for _ in range(HOST_REPEATS)]
    s, t, inf, c, b, share, rr, drop, mom = result["contrib"]
    assert s.tobytes() == result["plain"][0].tobytes() and t.tobytes() == result["plain"][1].tobytes(), "the moments changed the statistics"
    assert mom.tobytes() == result["moments"][0].tobytes(), "the run's moments are not the reduction alone on its kept samples"
    mc_, mp, mm = (np.median(v) for v in ts)
    rounds = (samples + CHUNK - 1) // CHUNK
    print("-- %s; %d samples, %d driven (normal, sigma %g x max(1, |value|), cut at %g sigma), %d reference dimensions (K = %d, %d sums), "
          "%d round(s) of %d" % (name, samples, k, SIGMA, TRUNC, n_meas, K, entries, rounds, CHUNK))
    print("   ok %d of %d, complete %d; dropped mask 0x%x" % (t["n_ok"][0], samples, inf[1], int(drop[0]) & (2 ** 64 - 1)))
    line("contrib", ts[0], samples)
    line("plain", ts[1], samples, "   (a) the moments add %.3f ms = %.1f%% of the plain run, %.1f us a round" %
         ((mc_ - mp) * 1e3, 100.0 * (mc_ - mp) / mp, (mc_ - mp) * 1e6 / rounds))
    line("moments", ts[2], samples, "   alone on the kept samples, its results read back")
    line("keep + numpy", th, samples, "   (b) contrib x%.1f" % (np.median(th) / mc_))
    cn, bn = result["numpy"]
    print("   against numpy on the kept samples: max |cov - numpy.cov| / max |cov| = %.2e, max |beta - lstsq| / max |beta| = %.2e"
          % (np.max(np.abs(c - cn)) / np.max(np.abs(cn)), np.max(np.abs(b - bn)) / np.max(np.abs(bn))))
    if show:
        S, sn = system.param_sensitivity(solved, pos, lam=LAMBDA)
        D = system.measure_response(solved, records, S)[0]
        print("   per reference dimension: r2, the largest share, and beta beside D of measure_response at the nominal point (lambda %g)" % LAMBDA)
        for i in range(n_meas):
            print("   [%d] r2 %.12f  1 - r2 %.3e  sum of shares %.12f  largest share %.4f (dimension %d)" %
                  (i, rr[i], 1.0 - rr[i], share[i].sum(), share[i].max(), int(share[i].argmax())))
            print("       beta " + " ".join("% .6e" % v for v in b[i]))
            print("       D    " + " ".join("% .6e" % v for v in D[i]))
        print("       max |beta - D| over the records: %.3e" % np.max(np.abs(b - D)))
    sys.stdout.flush()


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/contrib_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("Tolerance contributors (ezpz_system_tolerance_mc_contrib_device) on", torch.cuda.get_device_name(0))
    print("host clock around work that ends in a synchronise; %d warm-up run(s) of each form, then %d timed runs, the forms alternating;"
          % (WARMUP, REPEATS))
    print("median (min .. max).  plain = ezpz_system_tolerance_mc_device, the parent commit's code path, on the same inputs.")
    all_systems = systems()
    for name, system, recs, g in all_systems:
        pos, records = driven(recs), measurements(len(g))
        for samples in SAMPLES:
            case(name, system, recs, g, samples, stream, pos, records, show=samples == SAMPLES[0])
    name, system, recs, g = all_systems[1]
    pos, records = wide(recs, len(g))
    case(name + ", K = 64", system, recs, g, SAMPLES[0], stream, pos, records, show=False)


if __name__ == "__main__":
    main()
