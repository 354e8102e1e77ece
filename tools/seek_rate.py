"""The rate of the dimension targets (ezpz_system_seek_targets[_device]), printed as the text of
profiles/seek_rate.txt: seeks per second of the entry against the same loop driven from the host, and the share of a round that is
not the four existing entries.

Per system (a block system; one connected sketch of tests/gen.py), with 8 driven and 8 reference dimensions, and per batch:
  device form     ezpz_system_seek_targets_device with max_iterations 40: 41 rounds enqueued whatever the systems need, info read back
  device form, 8  the same with max_iterations 8 (9 rounds): what a caller who knows the seeks are short pays
  host form       ezpz_system_seek_targets: x0, params0, targets up, one counter read per round, stops when every system is done
  entries alone   the rounds' four entries (solve_batch_params, param_sensitivity, measure, measure_response, _device forms) on the
                  device form's buffers, 41 rounds: what the device form adds to them -- seek_step_kernel, seek_commit_kernel -- is the rest
  device chain    the four _device entries per iteration, ok, m and D copied to the host, the step in numpy, p_trial and the verdict
                  copied back, x committed by torch.where; stops when every system is done
  host chain      System.solve_batch_params -> param_sensitivity -> measure -> measure_response (host forms: x and S travel) and the
                  same numpy step; stops when every system is done

The numpy step is the header's algebra (scaled columns, the damping with its floor, accept iff the cost falls) through
numpy.linalg.solve: the same amount of work, not the same bits; no bounds are set.  Targets: the reference dimensions of the sketch
solved with its driven values scaled by 1 + 1e-3 * z, z normal -- targets that can be met, not necessarily by those values.  Host
clock around work that ends in a synchronise; WARMUP untimed runs of each form, then REPEATS timed runs (the chains:
CHAIN_REPEATS), the forms alternating; median (min .. max).

    python tools/seek_rate.py > profiles/seek_rate.txt
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
from ezpz_amd._lib import SEEK_INFO_DTYPE, STATUS_DTYPE  # noqa: E402
from mc_rate import driven, measurements, systems, timed  # noqa: E402

WARMUP, REPEATS, CHAIN_REPEATS = 1, 5, 3
BATCHES = (64, 4096, 65536)
MAX_ITERATIONS, SHORT = 40, 8
MU0, MU_UP, MU_DOWN, MU_MIN, MU_MAX, TOL, LAMBDA = 1e-3, 10.0, 0.1, 1e-12, 1e12, 1e-6, 1e-9


def line(what, ts, batch, extra=""):
    ts = np.asarray(ts)
    print("   %-15s %10.3f ms (%.3f .. %.3f)  %12.0f seeks/s%s" % (what, np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3,
                                                                 batch / np.median(ts), extra))
    sys.stdout.flush()


class NumpyLoop:
    """The seek's bookkeeping and step for a whole batch in numpy; `evaluate(p) -> (ok, m, D)` and `commit(accept)` are the caller's."""

    def __init__(self, targets):
        self.t = targets

    def cost(self, m):
        return ((self.t - m) ** 2).sum(1)

    def step(self, p, m, D, mu):
        g = np.einsum("bir,bi->br", D, self.t - m)
        A = np.einsum("bir,bic->brc", D, D)
        diag = np.einsum("brr->br", A)
        f = np.maximum(1e-2 * diag.max(1, keepdims=True), 1e-300)
        A[:, np.arange(A.shape[1]), np.arange(A.shape[1])] = diag + mu[:, None] * np.maximum(diag, f)
        return p + np.linalg.solve(A, g[:, :, None])[:, :, 0]

    def run(self, p0, evaluate, commit):
        batch = len(p0)
        ok, m, D = evaluate(p0)
        commit(ok)
        p, cost, mu = p0.copy(), self.cost(m), np.full(batch, MU0)
        active = ok & ~(np.abs(self.t - m) <= TOL).all(1)
        its = 0
        while active.any() and its < MAX_ITERATIONS:
            its += 1
            pt = np.where(active[:, None], self.step(p, m, D, mu), p)
            ok, mt, Dt = evaluate(pt)
            ct = self.cost(mt)
            accept = active & ok & np.isfinite(mt).all(1) & np.isfinite(Dt).all((1, 2)) & (ct < cost)
            commit(accept)
            p, m, D, cost = (np.where(accept.reshape((-1,) + (1,) * (a.ndim - 1)), b, a) for a, b in ((p, pt), (m, mt), (D, Dt), (cost, ct)))
            mu = np.where(accept, np.maximum(mu * MU_DOWN, MU_MIN), np.minimum(mu * MU_UP, MU_MAX))
            active &= ~(accept & (np.abs(self.t - m) <= TOL).all(1)) & ~(~accept & (mu >= MU_MAX))
        return p, m, its, int(active.sum())


def case(name, system, recs, g, batch, stream):
    n, pos, records = len(g), driven(recs), measurements(len(g))
    k, n_meas = len(pos), len(records)
    solved, st, _ = system.solve_batch(g[None, :])
    assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
    own = recs["param"][pos].astype(np.float64)
    rng = np.random.default_rng(1)
    x0, p0 = np.tile(solved[0], (batch, 1)), np.tile(own, (batch, 1))
    # targets that can be met: what the reference dimensions read on the sketch with other driven values
    there, st, _ = system.solve_batch_params(x0, pos, p0 * (1.0 + 1e-3 * rng.standard_normal((batch, k))))
    assert np.all((st["converged"] != 0) & (st["n_unsatisfied"] == 0)), name
    targets = system.measure(there, records)
    h = stream.cuda_stream
    with torch.cuda.stream(stream):
        dx0, dp0, dt = (torch.from_numpy(a).cuda() for a in (x0, p0, targets))
        params, x, m = (torch.zeros((batch, c), dtype=torch.float64, device="cuda") for c in (k, n, n_meas))
        info = torch.zeros(batch * SEEK_INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        chunk = min(batch, 32768)  # (S [chunk][8][n_vars] within 256 MiB for both systems: the entry's own cut at 65 536)
        xt = torch.zeros((chunk, n), dtype=torch.float64, device="cuda")
        S = torch.zeros((chunk, k, n), dtype=torch.float64, device="cuda")
        D = torch.zeros((chunk, n_meas, k), dtype=torch.float64, device="cuda")
        mt = torch.zeros((chunk, n_meas), dtype=torch.float64, device="cuda")
        fl = torch.zeros((chunk, n_meas), dtype=torch.uint8, device="cuda")
        status = torch.zeros((chunk, STATUS_DTYPE.itemsize // 4), dtype=torch.int32, device="cuda")
        sens = torch.zeros(chunk, dtype=torch.int32, device="cuda")
    result = {}

    def device_form(max_iterations=MAX_ITERATIONS, into="device"):
        with torch.cuda.stream(stream):
            system.seek_targets_device(dx0.data_ptr(), pos, dp0.data_ptr(), records, dt.data_ptr(), batch, params.data_ptr(), x.data_ptr(),
                                       m.data_ptr(), info.data_ptr(), config=E.SeekConfig(max_iterations=max_iterations), stream=h)
            result[into] = info.cpu().numpy().view(SEEK_INFO_DTYPE)

    def device_short():
        device_form(SHORT, "short")

    def host_form():
        result["host form"] = system.seek_targets(x0, pos, p0, records, targets).info

    def round_entries(x_from, p, first, count):
        system.solve_batch_params_device(x_from, pos, p, count, xt.data_ptr(), status.data_ptr(), stream=h)
        system.param_sensitivity_device(xt.data_ptr(), pos, p, count, S.data_ptr(), sens.data_ptr(), lam=LAMBDA, stream=h)
        system.measure_device(xt.data_ptr(), records, count, mt.data_ptr(), flags_ptr=fl.data_ptr(), stream=h)
        system.measure_response_device(xt.data_ptr(), records, S.data_ptr(), k, count, D.data_ptr(), stream=h)

    def entries_alone():
        with torch.cuda.stream(stream):
            for first in range(0, batch, chunk):
                for _ in range(MAX_ITERATIONS + 1):
                    round_entries(x[first:].data_ptr(), params[first:].data_ptr(), first, min(chunk, batch - first))

    loop = NumpyLoop(targets)

    def device_chain():
        with torch.cuda.stream(stream):
            xb = dx0.clone()
            out = []
            for first in range(0, batch, chunk):
                count = min(chunk, batch - first)
                sub = NumpyLoop(targets[first:first + count])

                def evaluate(p):
                    pd = torch.from_numpy(np.ascontiguousarray(p)).cuda()
                    round_entries(xb[first:].data_ptr(), pd.data_ptr(), first, count)
                    ok = (status[:count, 1] != 0) & (status[:count, 2] == 0) & (sens[:count] == 0) & ((fl[:count] & 1) == 0).all(1)
                    return ok.cpu().numpy(), mt[:count].cpu().numpy(), D[:count].cpu().numpy()

                def commit(accept):
                    a = torch.from_numpy(accept).cuda()
                    xb[first:first + count] = torch.where(a[:, None], xt[:count], xb[first:first + count])

                out.append(sub.run(p0[first:first + count], evaluate, commit))
            result["device chain"] = out

    def host_chain():
        xb = x0.copy()

        def evaluate(p):
            xs, st, _ = system.solve_batch_params(xb, pos, p)
            Ss, sn = system.param_sensitivity(xs, pos, p, lam=LAMBDA)
            ms, fs = system.measure(xs, records, want_flags=True)
            Ds = system.measure_response(xs, records, Ss)
            evaluate.x = xs
            return (st["converged"] != 0) & (st["n_unsatisfied"] == 0) & (sn == 0) & ((fs & 1) == 0).all(1), ms, Ds

        def commit(accept):
            xb[accept] = evaluate.x[accept]

        result["host chain"] = loop.run(p0, evaluate, commit)

    forms = [device_form, device_short, host_form, entries_alone]
    chains = [device_chain, host_chain]
    for _ in range(WARMUP):
        for f in forms + chains:
            timed(f)
    ts = [[] for _ in forms]
    for _ in range(REPEATS):
        for i, f in enumerate(forms):
            ts[i].append(timed(f))
    tc = [[] for _ in chains]
    for _ in range(CHAIN_REPEATS):
        for i, f in enumerate(chains):
            tc[i].append(timed(f))
    d, s, hf = result["device"], result["short"], result["host form"]
    assert d.tobytes() == hf.tobytes(), "the device form and the host form disagree"
    names = E.SEEK_STATUS
    count = lambda inf: ", ".join("%s %d" % (names[v], c) for v, c in zip(*np.unique(inf["status"], return_counts=True)))  # noqa: E731
    md, ms_, mh, me = (np.median(v) for v in ts)
    print("-- %s; batch %d, %d driven, %d reference dimensions, targets measured at driven values 1 + 1e-3 z off the start" % (name, batch, k, n_meas))
    print("   device form: %s; iterations %d .. %d (mean %.2f).  max_iterations %d: %s.  host chain: %d iterations, %d unfinished"
          % (count(d), d["iterations"].min(), d["iterations"].max(), d["iterations"].mean(), SHORT, count(s), result["host chain"][2],
             result["host chain"][3]))
    line("device form", ts[0], batch, "   41 rounds")
    line("device form, 8", ts[1], batch, "   9 rounds; device form x%.2f" % (ms_ / md))
    line("host form", ts[2], batch, "   device form x%.2f" % (mh / md))
    line("entries alone", ts[3], batch, "   not the four entries: %.1f%% of the device form" % (100.0 * (1.0 - me / md)))
    line("device chain", tc[0], batch, "   device form x%.2f, host form x%.2f" % (np.median(tc[0]) / md, np.median(tc[0]) / mh))
    line("host chain", tc[1], batch, "   device form x%.2f, host form x%.2f" % (np.median(tc[1]) / md, np.median(tc[1]) / mh))


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/seek_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("Dimension targets (ezpz_system_seek_targets[_device]) on", torch.cuda.get_device_name(0))
    print("host clock around work that ends in a synchronise; %d warm-up run(s) of each form, then %d timed runs (the chains: %d), the forms"
          % (WARMUP, REPEATS, CHAIN_REPEATS))
    print("alternating; median (min .. max).  The chains' step is numpy's: the same amount of work, not the same bits.")
    only = [int(a) for a in sys.argv[1:]] or BATCHES
    for name, system, recs, g in systems():
        for batch in only:
            case(name, system, recs, g, batch, stream)


if __name__ == "__main__":
    main()
