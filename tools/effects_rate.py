"""The rate of the Monte-Carlo main effects (ezpz_system_tolerance_mc_effects_device), printed as the text of
profiles/effects_rate.txt: what the effects add to the plain run, beside what the contributors add on the same build; the reduction
alone; the route that existed before; and a tolerance_sobol run of the same samples, since first-order indices are what both give.

The systems and settings are those of tools/mc_rate.py (8 driven dimensions, normal, cut at 3 sigma; 8 reference dimensions; rounds
of 65536), with 8 and 64 bins (64: 4096 cells, the limit).  Per case:
  plain        ezpz_system_tolerance_mc_device, stats and totals read back
  effects      ezpz_system_tolerance_mc_effects_device: the same run, one more kernel a round and the closing kernel; its seven
               outputs read back as well
  contrib      ezpz_system_tolerance_mc_contrib_device, its outputs read back: the sibling, for scale
  reduction    ezpz_mc_effects_device alone on the kept samples of a run, sums and counts read back
  host route   what the parent commit offers for the same curve and ratio: the host form with keep=True, numpy.searchsorted per
               dimension and numpy.bincount per (dimension, record)
  sobol        ezpz_system_tolerance_sobol_device on the same samples: k + 2 solves a sample
No ratio is fixed in advance.

Host clock around work that ends in a synchronise; WARMUP untimed runs of each form, then REPEATS timed runs, the forms alternating;
median (min .. max).

    python tools/effects_rate.py > profiles/effects_rate.txt
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
from ezpz_amd._lib import MC_MOMENTS_INFO_DTYPE, MC_STATS_DTYPE, MC_TOTALS_DTYPE  # noqa: E402
from mc_rate import CHUNK, SIGMA, TRUNC, driven, measurements, systems, timed  # noqa: E402

WARMUP, REPEATS = 1, 5
SAMPLES = (65536, 1048576)
BINS = (8, 64)
SEED = 1


def line(what, ts, samples, extra=""):
    ts = np.asarray(ts)
    print("   %-13s %10.3f ms (%.3f .. %.3f)  %12.0f samples/s%s" % (what, np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3,
                                                                    samples / np.median(ts), extra))
    sys.stdout.flush()


def numpy_effects(p, y, flags, ok, nominal, edges):
    """eta2 [m, k] by numpy: the validity rule per record, plain sums."""
    k, m, B = p.shape[1], y.shape[1], edges.shape[1] + 1
    eta2 = np.zeros((m, k))
    which = [np.searchsorted(edges[j], p[:, j], side="right") for j in range(k)]
    for i in range(m):
        live = (ok != 0) & ((flags[:, i] & 1) == 0) & np.isfinite(y[:, i])
        d = y[live, i] - nominal[i]
        sst = ((d - d.mean()) ** 2).sum()
        for j in range(k):
            w = which[j][live]
            n, s = np.bincount(w, minlength=B), np.bincount(w, weights=d, minlength=B)
            with np.errstate(all="ignore"):
                mu = s[n > 0] / n[n > 0]
                eta2[i, j] = (n[n > 0] * (mu - d.mean()) ** 2).sum() / sst
    return eta2


def case(name, system, recs, g, samples, stream):
    pos, records = driven(recs), measurements(len(g))
    k, m = len(pos), len(records)
    solved, st, _ = system.solve_batch(g[None, :])
    assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
    own = recs["param"][pos].astype(np.float64)
    dists = [E.McDist.normal(float(s), TRUNC) for s in SIGMA * np.maximum(1.0, np.abs(own))]
    h = stream.cuda_stream
    K = k + m
    with torch.cuda.stream(stream):
        x0 = torch.from_numpy(solved[0]).cuda()
        stats = torch.zeros(m * MC_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        totals = torch.zeros(MC_TOTALS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
        i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")  # noqa: E731
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
        kp, km, kf, ko = f64(samples, k), f64(samples, m), u8(samples, m), u8(samples)
        moments, info, cov = f64(K + K * (K + 1) // 2), u8(MC_MOMENTS_INFO_DTYPE.itemsize), f64(K, K)
        beta, contrib, r2, dropped = f64(m, k), f64(m, k), f64(m), i64(1)
        s_sums, s_n, s_var, s_idx = f64(m, 4 + 4 * k), i64(m), f64(m), [f64(m, k) for _ in range(4)]
        nominal_m = torch.from_numpy(system.measure(solved, records)[0]).cuda()
    result = {}
    common = dict(seed=SEED, chunk=CHUNK, stream=h)

    def plain(keep=False):
        kept = dict(keep_params_ptr=kp.data_ptr(), keep_m_ptr=km.data_ptr(), keep_flags_ptr=kf.data_ptr(), keep_ok_ptr=ko.data_ptr()) if keep else {}
        with torch.cuda.stream(stream):
            system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), **common, **kept)
            result["plain"] = stats.cpu().numpy(), totals.cpu().numpy()

    def with_contrib():
        with torch.cuda.stream(stream):
            system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), **common,
                                       moments_ptr=moments.data_ptr(), info_ptr=info.data_ptr(), cov_ptr=cov.data_ptr(), beta_ptr=beta.data_ptr(),
                                       contrib_ptr=contrib.data_ptr(), r2_ptr=r2.data_ptr(), dropped_ptr=dropped.data_ptr())
            result["contrib"] = [t.cpu().numpy() for t in (stats, totals, moments, info, cov, beta, contrib, r2, dropped)]

    def sobol():
        with torch.cuda.stream(stream):
            system.tolerance_sobol_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), s_sums.data_ptr(),
                                          s_n.data_ptr(), s_var.data_ptr(), *(t.data_ptr() for t in s_idx), seed=SEED, chunk=CHUNK, stream=h)
            result["sobol"] = [t.cpu().numpy() for t in (stats, totals, s_sums, s_n, s_var, *s_idx)]

    timed(lambda: plain(keep=True))  # (the kept samples the reduction alone runs on; also a warm-up)
    rounds = (samples + CHUNK - 1) // CHUNK
    print("-- %s; %d samples, %d driven (normal, sigma %g x max(1, |value|), cut at %g sigma), %d reference dimensions, %d round(s) of %d"
          % (name, samples, k, SIGMA, TRUNC, m, rounds, CHUNK))
    for bins in BINS:
        cells = k * bins * m
        with torch.cuda.stream(stream):
            e_sums, e_n, e_mean, e_var, e_eta2, e_first = f64(2 * cells), i64(cells), f64(cells), f64(cells), f64(m, k), f64(m, k)
            e_used = torch.zeros((m, k), dtype=torch.int32, device="cuda")
            a_sums, a_n = f64(2 * cells), i64(cells)
        cfg = E.EffectsConfig(bins)
        edges_dev = {}

        def with_effects():
            with torch.cuda.stream(stream):
                result["edges"] = system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), **common,
                                                             effects=cfg, effect_sums_ptr=e_sums.data_ptr(), effect_counts_ptr=e_n.data_ptr(),
                                                             cond_mean_ptr=e_mean.data_ptr(), cond_var_ptr=e_var.data_ptr(), eta2_ptr=e_eta2.data_ptr(),
                                                             first_ptr=e_first.data_ptr(), bins_used_ptr=e_used.data_ptr())
                result["effects"] = [t.cpu().numpy() for t in (stats, totals, e_sums, e_n, e_mean, e_var, e_eta2, e_first, e_used)]

        def reduction():
            with torch.cuda.stream(stream):
                rc = E.lib().ezpz_mc_effects_device(kp.data_ptr(), km.data_ptr(), kf.data_ptr(), ko.data_ptr(), nominal_m.data_ptr(),
                                                    edges_dev["p"].data_ptr(), samples, k, m, bins, CHUNK, a_sums.data_ptr(), a_n.data_ptr(), h)
                assert rc == 0, rc
                result["alone"] = a_sums.cpu().numpy(), a_n.cpu().numpy()

        def host_route():
            res = system.tolerance_mc(solved[0], pos, dists, records, samples, seed=SEED, chunk=CHUNK, keep=True)
            result["host"] = numpy_effects(res.params, res.m, res.flags, res.ok, res.nominal, result["edges"])

        timed(with_effects)
        with torch.cuda.stream(stream):
            edges_dev["p"] = torch.from_numpy(result["edges"]).cuda()
        forms = [plain, with_effects, with_contrib, reduction, host_route, sobol]
        for _ in range(WARMUP):
            for fn in forms:
                timed(fn)
        ts = [[] for _ in forms]
        for _ in range(REPEATS):
            for i, fn in enumerate(forms):
                ts[i].append(timed(fn))
        e = result["effects"]
        assert e[0].tobytes() == result["plain"][0].tobytes() and e[1].tobytes() == result["plain"][1].tobytes(), "the run with effects is not the plain run"
        assert e[2].tobytes() == result["alone"][0].tobytes() and e[3].tobytes() == result["alone"][1].tobytes(), \
            "the run's cells are not the reduction alone on its kept samples"
        t_plain, t_eff, t_con, t_red, t_host, t_sob = (np.median(v) for v in ts)
        row_bytes = samples * ((k + m) * 8 + m + 1)
        print("   bins %d: %d cells" % (bins, cells))
        line("plain", ts[0], samples)
        line("effects", ts[1], samples, "   adds %.3f ms = %.1f%% of the plain run, %.1f us a round" %
             ((t_eff - t_plain) * 1e3, 100.0 * (t_eff - t_plain) / t_plain, (t_eff - t_plain) * 1e6 / rounds))
        line("contrib", ts[2], samples, "   adds %.3f ms = %.1f%%" % ((t_con - t_plain) * 1e3, 100.0 * (t_con - t_plain) / t_plain))
        line("reduction", ts[3], samples, "   alone on the kept samples, its results read back; %.1f GB/s of rows" % (row_bytes / t_red / 1e9))
        line("host route", ts[4], samples, "   effects x%.1f" % (t_host / t_eff))
        line("sobol", ts[5], samples, "   effects x%.1f" % (t_sob / t_eff))
        s_first, s_se = result["sobol"][5], np.sqrt(np.maximum(result["sobol"][7], 0.0))
        print("   against the host route: max |eta2 - numpy| = %.3e;  against pick-freeze: max |first - sobol first| = %.3e (largest first_se %.3e)"
              % (np.nanmax(np.abs(e[6] - result["host"])), np.nanmax(np.abs(e[7] - s_first)), np.nanmax(s_se)))
        if samples == SAMPLES[-1]:
            for i in range(m):
                print("   [%d] first by the bins %s" % (i, " ".join("% .4f" % v for v in e[7][i])))
                print("       by pick-freeze    %s" % " ".join("% .4f" % v for v in s_first[i]))
        sys.stdout.flush()


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/effects_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("Monte-Carlo main effects (ezpz_system_tolerance_mc_effects_device) on", torch.cuda.get_device_name(0))
    print("host clock around work that ends in a synchronise; %d warm-up run(s) of each form, then %d timed runs, the forms alternating;"
          % (WARMUP, REPEATS))
    print("median (min .. max).  host route = tolerance_mc(keep=True) on the host form, numpy.searchsorted and bincount: what the parent commit offers.")
    for name, system, recs, g in systems():
        for samples in SAMPLES:
            case(name, system, recs, g, samples, stream)


if __name__ == "__main__":
    main()
