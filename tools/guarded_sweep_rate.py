"""Two measurements of the guarded sweep (ezpz_system_sweep_guarded_device), printed as the text of
profiles/guarded_sweep_rate.txt.

1. The guard's overhead: a guarded sweep whose every step is accepted at its first attempt against ezpz_system_sweep_params_device
   on the same inputs in the same run, per route the device form serves, at batch 1 and at a batch that fills the device -- with
   the default policy (no displacement test) and with a max_move no step comes near (the test runs, and never rejects).
2. A drag with a limit in it: one sweep of 240 steps of the 300-variable sketch, a distance of which is pulled in below what the
   sketch can follow and let out again, in one launch, against the same rule driven from the host (one solve_batch_params_device call per
   attempt, the status and the values read back to decide on it).

Device resident, both forms enqueued on one stream, the host clock from the first enqueue to the stream's synchronise (for the
host-driven rule: to its last decision); WARMUP untimed runs of each form, then REPEATS timed runs, the forms alternating; median
and spread (min .. max).  Equal bits of the forms are asserted before anything is timed.

    python tools/guarded_sweep_rate.py > profiles/guarded_sweep_rate.txt
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
from ezpz_amd._lib import GUARD_STEP_DTYPE, STATUS_DTYPE, CGuardConfig  # noqa: E402

WARMUP, REPEATS = 2, 7
BATCHES, STEPS = (1, 4096), 240
MAX_DRIVEN = 8


def systems():
    from gen import connected_sketch
    from sweep_common import chain, record_walk_sketch

    recs, g = connected_sketch(150, 11)
    crecs, cg = chain(40)
    rrecs, rg = record_walk_sketch()
    return [("sketch, 300 variables", E.System(recs, len(g), team_size=256), recs, np.asarray(g, dtype=float)),
            ("chain of 40 points", E.System(crecs, len(cg), team_size=64), crecs, cg),
            ("sketch of 70 points", E.System(rrecs, len(rg), team_size=E.TEAM_LATENCY_RECORDS), rrecs, rg)]


def driven(recs):
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    return np.ascontiguousarray(pos[np.linspace(0, len(pos) - 1, min(MAX_DRIVEN, len(pos))).astype(int)])


def timed(stream, f):
    stream.synchronize()
    t0 = time.perf_counter()
    f()
    stream.synchronize()
    return time.perf_counter() - t0


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return "%9.3f (%.3f .. %.3f)" % (np.median(ts), ts.min(), ts.max())


class Buffers:
    """The device arrays of one form of a sweep."""

    def __init__(self, steps, batch, n, k):
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
        self.x, self.reached = z(steps, batch, n), z(steps, batch, k)
        self.status = torch.zeros((steps, batch, STATUS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        self.guard = torch.zeros((steps, batch, GUARD_STEP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")


def overhead(name, system, recs, g, batch, stream):
    n, pos = len(g), driven(recs)
    rng = np.random.default_rng(batch)
    # (the walk starts at the solved sketch, so that every step converges and nothing is unsatisfied)
    solved, st, _ = system.solve_batch(g[None, :])
    assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
    walk = np.cumsum(rng.uniform(-0.001, 0.001, (STEPS, batch, len(pos))), axis=0)
    own = recs["param"][pos].astype(np.float64)
    params = np.ascontiguousarray(own[None, None, :] + walk)
    x0 = np.repeat(solved, batch, axis=0)
    with torch.cuda.stream(stream):
        pd, xin, p0 = torch.from_numpy(params).cuda(), torch.from_numpy(x0).cuda(), torch.from_numpy(np.tile(own, (batch, 1))).cuda()
        plain, guarded, bounded = (Buffers(STEPS, batch, n, len(pos)) for _ in range(3))
    L, cfg, h, pp = E.lib(), C.byref(E.Config()._c()), stream.cuda_stream, pos.ctypes.data
    free, far = CGuardConfig(4, 12, 0.0), CGuardConfig(4, 12, 1e3)

    def sweep():
        rc = L.ezpz_system_sweep_params_device(system._h, xin.data_ptr(), pp, len(pos), pd.data_ptr(), STEPS, batch, cfg, plain.x.data_ptr(),
                                               plain.status.data_ptr(), None, None, 0, h)
        assert rc == 0, rc

    def guarded_sweep(b, policy):
        rc = L.ezpz_system_sweep_guarded_device(system._h, xin.data_ptr(), pp, len(pos), p0.data_ptr(), pd.data_ptr(), STEPS, batch, cfg,
                                                C.byref(policy), b.x.data_ptr(), b.status.data_ptr(), b.guard.data_ptr(),
                                                b.reached.data_ptr(), None, None, 0, h)
        assert rc == 0, rc

    forms = [sweep, lambda: guarded_sweep(guarded, free), lambda: guarded_sweep(bounded, far)]
    for _ in range(WARMUP):
        for f in forms:
            timed(stream, f)
    at_once = True
    for b in (guarded, bounded):
        gs = b.guard.cpu().numpy().view(GUARD_STEP_DTYPE)
        at_once = at_once and bool(np.all(gs["attempts"] == 1) and np.all(gs["accepted"] == 1) and np.all(gs["reached"] == 1.0))
        if at_once:  # (the same solves then, from the same values: the same bits)
            assert torch.equal(b.x, plain.x) and torch.equal(b.status, plain.status), "the guarded sweep and the sweep differ"
    ts = [[], [], []]
    for _ in range(REPEATS):
        for i, f in enumerate(forms):
            ts[i].append(timed(stream, f))
    m = [np.median(t) for t in ts]
    print(f"{name:24s} batch {batch:5d} steps {STEPS}  sweep {spread(ts[0])}  guarded {spread(ts[1])} x{m[1] / m[0]:5.3f}"
          f"  guarded, max_move 1e3 {spread(ts[2])} x{m[2] / m[0]:5.3f}"
          + ("" if at_once else "  NOT every step accepted at once: the forms did different work"))
    sys.stdout.flush()


def host_driven(system, pos, xin, p0, targets, stream, policy):
    """The rule for ONE sweep driven from the host, device resident: a params call per attempt, its status and values read back."""
    L, cfg, h, pp = E.lib(), C.byref(E.Config()._c()), stream.cuda_stream, pos.ctypes.data
    n, k = xin.shape[1], len(pos)
    with torch.cuda.stream(stream):
        xs, x_try = xin.clone(), torch.zeros_like(xin)
        pu = torch.zeros((1, k), dtype=torch.float64, device="cuda")
        st = torch.zeros(STATUS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ps = p0.copy()
    xs_host = xs.cpu().numpy()
    table = np.zeros(len(targets), dtype=GUARD_STEP_DTYPE)
    for step, pb in enumerate(targets):
        pa, t, hh, attempts, accepted = ps.copy(), 0.0, 1.0, 0, 0
        while t < 1 and attempts < policy.max_attempts:
            u = t + hh
            d = pb - pa
            d = u * d
            p_u = pb.copy() if u == 1.0 else pa + d
            with torch.cuda.stream(stream):
                pu.copy_(torch.from_numpy(p_u[None, :]), non_blocking=False)
                rc = L.ezpz_system_solve_batch_params_device(system._h, xs.data_ptr(), pp, k, pu.data_ptr(), 1, cfg, x_try.data_ptr(),
                                                             st.data_ptr(), None, None, 0, h)
                assert rc == 0, rc
                status = st.cpu().numpy().view(STATUS_DTYPE)[0]
                ok = status["converged"] == 1 and status["n_unsatisfied"] == 0
                if ok and policy.max_move > 0:
                    x_host = x_try.cpu().numpy()
                    ok = bool(np.all(np.abs(x_host - xs_host) <= policy.max_move))
            attempts += 1
            if ok:
                with torch.cuda.stream(stream):
                    xs.copy_(x_try)
                if policy.max_move > 0:
                    xs_host = x_host
                ps, t, accepted = p_u, u, accepted + 1
            else:
                hh /= 2
                if hh < 2.0 ** -policy.max_halvings:
                    break
        table[step] = (t, attempts, accepted)
    stream.synchronize()
    return table, xs.cpu().numpy()


def drag(stream):
    from oracle import oracle as O

    name, system, recs, g = systems()[0]
    solved, st, _ = system.solve_batch(g[None, :])
    policy = CGuardConfig(4, 12, 0.5)
    L, cfg, h = E.lib(), C.byref(E.Config()._c()), stream.cuda_stream
    k = np.arange(1, STEPS + 1) / STEPS
    with torch.cuda.stream(stream):
        xin = torch.from_numpy(solved).cuda()
        b = Buffers(STEPS, 1, len(g), 1)
    # a distance pulled in to a tenth of its value and let out again: where the point it places is also held by a coordinate or
    # an axis distance, the sketch cannot follow below that -- the first distance whose drag is held at some steps and ends at its
    # target is the one measured
    distance_kind = int(O.distance((0, 1), (2, 3), 1.0)["kind"])
    for position in [i for i in range(len(recs)) if int(recs["kind"][i]) == distance_kind][:40]:
        pos = np.asarray([position], dtype=np.uint32)
        own = recs["param"][pos].astype(np.float64)
        targets = np.ascontiguousarray((own[None, :] * (1.0 - 0.9 * np.sin(np.pi * k))[:, None]).reshape(STEPS, 1, 1))
        with torch.cuda.stream(stream):
            pd, p0 = torch.from_numpy(targets).cuda(), torch.from_numpy(own[None, :]).cuda()

        def one_launch():
            rc = L.ezpz_system_sweep_guarded_device(system._h, xin.data_ptr(), pos.ctypes.data, 1, p0.data_ptr(), pd.data_ptr(), STEPS, 1, cfg,
                                                    C.byref(policy), b.x.data_ptr(), b.status.data_ptr(), b.guard.data_ptr(),
                                                    b.reached.data_ptr(), None, None, 0, h)
            assert rc == 0, rc

        timed(stream, one_launch)
        gs = b.guard.cpu().numpy().view(GUARD_STEP_DTYPE).reshape(STEPS)
        if (gs["reached"] == 0).any() and gs["reached"][-1] == 1.0 and gs["accepted"][-1] >= 1:
            break
    else:
        raise SystemExit("no distance of the sketch has a limit in this drag")

    result = {}

    def from_the_host():
        result["table"], result["x"] = host_driven(system, pos, xin, own, targets[:, 0, :], stream, policy)

    for _ in range(WARMUP):
        timed(stream, one_launch), timed(stream, from_the_host)
    gs = b.guard.cpu().numpy().view(GUARD_STEP_DTYPE).reshape(STEPS)
    assert gs.tobytes() == result["table"].tobytes(), "the launch and the host-driven rule took different decisions"
    assert np.array_equal(b.x[-1].cpu().numpy(), result["x"]), "the launch and the host-driven rule end at different values"
    tl, th = [], []
    for _ in range(REPEATS):
        tl.append(timed(stream, one_launch)), th.append(timed(stream, from_the_host))
    print(f"-- drag: {name}, the distance at position {int(pos[0])} ({own[0]:.4f}) pulled in to a tenth of its value and let out again in"
          f" {STEPS} steps, max_move 0.5, defaults otherwise")
    print(f"   attempts {int(gs['attempts'].sum())} in all, {int(gs['accepted'].sum())} accepted; steps that reached their target "
          f"{int((gs['reached'] == 1).sum())} of {STEPS}, stopped short {int(((gs['reached'] > 0) & (gs['reached'] < 1)).sum())}, "
          f"held {int((gs['reached'] == 0).sum())}")
    print(f"   one launch {spread(tl)} ms   host-driven rule {spread(th)} ms   x{np.median(th) / np.median(tl):6.2f}   same decisions and values")


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/guarded_sweep_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("guarded sweep (ezpz_system_sweep_guarded_device) on", torch.cuda.get_device_name(0))
    print("device resident, one stream, host clock from the first enqueue to the stream's synchronise; %d warm-up runs, then %d timed" % (WARMUP, REPEATS))
    print("runs of each form, alternating; median (min .. max) in milliseconds; equal bits asserted before anything is timed.")
    print("-- the guard's overhead: every step accepted at its first attempt, against ezpz_system_sweep_params_device on the same inputs")
    for name, system, recs, g in systems():
        plan = system.sweep_guarded_plan(driven(recs))
        print(f"-- {name}: route {plan['route_name']}, in_kernel {plan['in_kernel']}, params_in_lds {plan['params_in_lds']}, {len(driven(recs))} driven")
        for batch in BATCHES:
            overhead(name, system, recs, g, batch, stream)
    drag(stream)


if __name__ == "__main__":
    main()
