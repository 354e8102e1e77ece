"""The rate of the Monte-Carlo tolerance analysis (ezpz_system_tolerance_mc_device), printed as the text of
profiles/tolerance_mc_rate.txt: samples per second of the entry against the same work done through the public chain, and the share
of a run that is not the driven solve.

Per system (a block system; one connected sketch of tests/gen.py) and per number of samples:
  entry        ezpz_system_tolerance_mc_device in rounds of 65536 samples, its n_meas records of statistics read back
  one round    the same with chunk = samples: the memory the chain below takes (samples x n_vars values, twice), the same bits
  solve alone  the rounds' ezpz_system_solve_batch_params_device calls on the entry's own draws (kept from a run) and ready copies
               of x0, in the entry's rounds: what the entry adds to them -- sampler, copies of x0, measure, reduction -- is the rest
  chain        torch draws on the device -> solve_batch_params_device -> measure_device -> torch statistics on the device (sums,
               extremes and their samples, counts), the small results read back; the whole batch at once
  host chain   numpy draws -> System.solve_batch_params -> System.measure -> numpy statistics: x travels to the host and back

The chains draw other numbers than the entry (their generators are their own): the forms do the same amount of work, not the same
solves.  Host clock around work that ends in a synchronise; WARMUP untimed runs of each form, then REPEATS timed runs, the forms
alternating; median (min .. max).

    python tools/mc_rate.py > profiles/tolerance_mc_rate.txt
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
from ezpz_amd._lib import MC_STATS_DTYPE, MC_TOTALS_DTYPE, STATUS_DTYPE  # noqa: E402
from oracle import oracle as O  # noqa: E402

WARMUP, REPEATS, HOST_REPEATS = 1, 5, 3
SAMPLES = (65536, 1048576)
CHUNK = 65536
MAX_DRIVEN, SIGMA, TRUNC = 8, 1e-3, 3.0


def systems():
    from gen import connected_sketch

    block = E.textual.Problem.from_str(E.textual.gen_big_problem(16)).to_constraint_system()
    recs, g = connected_sketch(40, 11)
    return [("block system, 16 blocks, %d variables" % block.num_vars, E.System(block.records, block.num_vars), block.records,
             np.asarray(block.guesses, dtype=float)),
            ("connected sketch, %d variables" % len(g), E.System(recs, len(g)), recs, np.asarray(g, dtype=float))]


def driven(recs):
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    return np.ascontiguousarray(pos[np.linspace(0, len(pos) - 1, min(MAX_DRIVEN, len(pos))).astype(int)])


def measurements(n):
    pts = n // 2
    pt = lambda i: (2 * i, 2 * i + 1)  # noqa: E731
    pairs = [(0, pts - 1), (1, pts // 2), (pts // 3, pts - 2), (2, pts - 3)]
    return O.stack([O.distance(pt(a), pt(b), 0.0) for a, b in pairs] + [O.horizontal_distance(pt(a), pt(b), 0.0) for a, b in pairs])


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def line(what, ts, samples, extra=""):
    ts = np.asarray(ts)
    print("   %-12s %10.3f ms (%.3f .. %.3f)  %12.0f samples/s%s" % (what, np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3,
                                                                   samples / np.median(ts), extra))
    sys.stdout.flush()


def case(name, system, recs, g, samples, stream):
    n, pos, records = len(g), driven(recs), measurements(len(g))
    k, n_meas = len(pos), len(records)
    solved, st, _ = system.solve_batch(g[None, :])
    assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
    own = recs["param"][pos].astype(np.float64)
    sigma = SIGMA * np.maximum(1.0, np.abs(own))
    dists = [E.McDist.normal(float(s), TRUNC) for s in sigma]
    L, cfg, h = E.lib(), C.byref(E.Config()._c()), stream.cuda_stream
    with torch.cuda.stream(stream):
        x0 = torch.from_numpy(solved[0]).cuda()
        stats = torch.zeros(n_meas * MC_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        totals = torch.zeros(MC_TOTALS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        kept = torch.zeros((samples, k), dtype=torch.float64, device="cuda")
        x_in, x_out = x0.repeat(CHUNK, 1), torch.zeros((CHUNK, n), dtype=torch.float64, device="cuda")
        status = torch.zeros((samples, STATUS_DTYPE.itemsize // 4), dtype=torch.int32, device="cuda")
        xs_all = torch.zeros((samples, n), dtype=torch.float64, device="cuda")
        m_all = torch.zeros((samples, n_meas), dtype=torch.float64, device="cuda")
        f_all = torch.zeros((samples, n_meas), dtype=torch.uint8, device="cuda")
        own_d, sigma_d = torch.from_numpy(own).cuda(), torch.from_numpy(sigma).cuda()
        nominal = torch.from_numpy(system.measure(solved, records)[0]).cuda()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    result = {}

    def entry(keep=0, chunk=CHUNK, into="stats"):
        with torch.cuda.stream(stream):
            system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, samples, stats.data_ptr(), totals.data_ptr(), seed=1, chunk=chunk,
                                       keep_params_ptr=keep, stream=h)
            result[into], result["totals"] = stats.cpu().numpy().view(MC_STATS_DTYPE), totals.cpu().numpy().view(MC_TOTALS_DTYPE)

    def one_round():
        entry(chunk=samples, into="stats, one round")

    def solve_alone():
        for first in range(0, samples, CHUNK):
            count = min(CHUNK, samples - first)
            rc = L.ezpz_system_solve_batch_params_device(system._h, x_in.data_ptr(), pos.ctypes.data, k, kept[first:].data_ptr(), count, cfg,
                                                         x_out.data_ptr(), status[first:].data_ptr(), None, None, 0, h)
            assert rc == 0, rc

    def chain():
        with torch.cuda.stream(stream):
            z = torch.randn((samples, k), dtype=torch.float64, device="cuda", generator=gen).clamp_(-TRUNC, TRUNC)
            params = own_d + sigma_d * z
            xs = x0.expand(samples, n).contiguous()
            system.solve_batch_params_device(xs.data_ptr(), pos, params.data_ptr(), samples, xs_all.data_ptr(), status.data_ptr(), stream=h)
            system.measure_device(xs_all.data_ptr(), records, samples, m_all.data_ptr(), flags_ptr=f_all.data_ptr(), stream=h)
            ok = (status[:, 1] != 0) & (status[:, 2] == 0)
            valid = ok[:, None] & ((f_all & 1) == 0) & torch.isfinite(m_all)
            d = torch.where(valid, m_all - nominal, torch.zeros_like(m_all))
            lo, hi = torch.where(valid, m_all, torch.full_like(m_all, np.inf)).min(0), torch.where(valid, m_all, torch.full_like(m_all, -np.inf)).max(0)
            small = [valid.sum(0), d.sum(0), (d * d).sum(0), lo.values, lo.indices, hi.values, hi.indices, ok.sum()]
            result["chain"] = [t.cpu() for t in small]

    def host_chain():
        rng = np.random.default_rng(1)
        params = own + sigma * np.clip(rng.standard_normal((samples, k)), -TRUNC, TRUNC)
        x, st, _ = system.solve_batch_params(np.broadcast_to(solved[0], (samples, n)), pos, params)
        m, fl = system.measure(x, records, want_flags=True)
        ok = (st["converged"] != 0) & (st["n_unsatisfied"] == 0)
        valid = ok[:, None] & ((fl & 1) == 0) & np.isfinite(m)
        d = np.where(valid, m - nominal_host, 0.0)
        result["host"] = [valid.sum(0), d.sum(0), (d * d).sum(0), np.where(valid, m, np.inf).min(0), np.where(valid, m, -np.inf).max(0), ok.sum()]

    nominal_host = nominal.cpu().numpy()
    timed(lambda: entry(kept.data_ptr()))  # (the draws the solve alone runs on; also a warm-up)
    forms = [entry, solve_alone, chain, one_round]
    for _ in range(WARMUP):
        for f in forms:
            timed(f)
    assert result["stats"].tobytes() == result["stats, one round"].tobytes(), "the statistics depend on the rounds"
    ts = [[] for _ in forms]
    for _ in range(REPEATS):
        for i, f in enumerate(forms):
            ts[i].append(timed(f))
    timed(host_chain)
    th = [timed(host_chain) for _ in range(HOST_REPEATS)]
    s, t = result["stats"], result["totals"]
    cn, cd, cd2 = (float(result["chain"][i][0]) for i in (0, 1, 2))
    chain_std = np.sqrt((cd2 - cd * cd / cn) / (cn - 1))
    me, ms, mc, mo = (np.median(v) for v in ts)
    print("-- %s; %d samples, %d driven (normal, sigma %g x max(1, |value|), cut at %g sigma), %d reference dimensions, rounds of %d"
          % (name, samples, k, SIGMA, TRUNC, n_meas, CHUNK))
    print("   ok %d of %d; first reference dimension: mean %.9g, std %.3g (the chain's own draws: ok %d, std %.3g)"
          % (t["n_ok"][0], samples, s["mean"][0], np.sqrt(s["var"][0]), int(result["chain"][7]), chain_std))
    line("entry", ts[0], samples)
    line("one round", ts[3], samples, "   entry x%.2f" % (mo / me))
    line("solve alone", ts[1], samples, "   not the solve: %.1f%% of the entry" % (100.0 * (1.0 - ms / me)))
    line("chain", ts[2], samples, "   entry x%.2f" % (mc / me))
    line("host chain", th, samples, "   entry x%.2f" % (np.median(th) / me))


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/mc_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("Monte-Carlo tolerance analysis (ezpz_system_tolerance_mc_device) on", torch.cuda.get_device_name(0))
    print("host clock around work that ends in a synchronise; %d warm-up run(s) of each form, then %d timed runs (host chain: %d), the forms"
          % (WARMUP, REPEATS, HOST_REPEATS))
    print("alternating; median (min .. max).  The chains draw their own numbers: the same amount of work, not the same solves.")
    for name, system, recs, g in systems():
        for samples in SAMPLES:
            case(name, system, recs, g, samples, stream)


if __name__ == "__main__":
    main()
