"""What the guarded-sweep tests share (ezpz_system_sweep_guarded; tests/test_guarded_sweep_cpu.py, tests/test_gpu_guarded_sweep.py):
the rule of include/ezpz_amd.h written once over any "solve these systems from these values with these driven values", its two
instances -- over the oracle, as sweep_common.oracle_chain runs it per attempt, and over System.solve_batch_params, which is the
DEFINITION and the reference of every bitwise test -- and the crank, the one input whose every decision is known."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from sweep_common import CASES, chain, driven_walk, record_walk_sketch, substituted

GUARD_DTYPE = np.dtype([("reached", "<f8"), ("attempts", "<u4"), ("accepted", "<u4")])  # EzpzGuardStep
DEFAULT_GUARD = dict(max_halvings=4, max_attempts=12, max_move=0.0)


def between(pa, pb, u):
    """p_u of the rule, row by row: p_b itself where u == 1, else p_a + u * (p_b - p_a) in three separately rounded operations
    (numpy fuses nothing).  pa, pb [batch, k], u [batch]."""
    d = pb - pa
    d = u[:, None] * d
    return np.where((u == 1.0)[:, None], pb, pa + d)


def run_rule(solve, x0, params0, params, max_halvings=4, max_attempts=12, max_move=0.0, on_attempt=None):
    """The rule.  solve(x_s [batch, n], p_u [batch, k], active [batch] bool) -> (x [batch, n], converged [batch], n_unsatisfied
    [batch], extra): one attempt for every sweep; rows of finished sweeps (active False) are ignored.  on_attempt(k, b, extra,
    displacement, accepted) sees every attempt of every sweep inside its step.  Returns x [steps, batch, n], guard [steps, batch]
    (GUARD_DTYPE), params_reached [steps, batch, k] and last [steps, batch]: the round (index into the step's solves) of each
    sweep's last attempt, with the list of every step's `extra` values in `rounds`."""
    steps, batch, k = params.shape
    xs, ps = np.array(x0, dtype=np.float64), np.array(params0, dtype=np.float64)
    x_out = np.zeros((steps, batch, xs.shape[1]))
    reached = np.zeros((steps, batch, k))
    guard = np.zeros((steps, batch), dtype=GUARD_DTYPE)
    last = np.zeros((steps, batch), dtype=np.int64)
    rounds = []
    h_min = 2.0 ** -max_halvings
    for step in range(steps):
        pa, pb = ps.copy(), params[step]
        t, h = np.zeros(batch), np.ones(batch)
        attempts, accepted = np.zeros(batch, np.uint32), np.zeros(batch, np.uint32)
        inside = np.ones(batch, bool)
        extras = []
        while inside.any():
            pu = np.where(inside[:, None], between(pa, pb, t + h), ps)
            x, conv, nun, extra = solve(xs, pu, inside.copy())
            extras.append(extra)
            with np.errstate(invalid="ignore"):
                moved = np.abs(x - xs)
                ok = inside & (np.asarray(conv) == 1) & (np.asarray(nun) == 0)
                if max_move > 0:
                    ok &= np.all(moved <= max_move, axis=1)  # (a NaN rejects)
            attempts[inside] += 1
            last[step, inside] = len(extras) - 1
            if on_attempt is not None:
                for b in np.nonzero(inside)[0]:
                    on_attempt(step, int(b), extra, moved[b], bool(ok[b]))
            xs[ok], ps[ok] = x[ok], pu[ok]
            t[ok] += h[ok]
            accepted[ok] += 1
            rejected = inside & ~ok
            h[rejected] /= 2
            inside &= ~((t >= 1) | (attempts >= max_attempts) | (rejected & (h < h_min)))
        x_out[step], reached[step] = xs, ps
        guard[step]["reached"], guard[step]["attempts"], guard[step]["accepted"] = t, attempts, accepted
        rounds.append(extras)
    return x_out, guard, reached, last, rounds


def oracle_rule(recs, pos, x0, params0, params, cfg=None, on_attempt=None, **guard):
    """The rule over the oracle, one oracle solve per attempt on the substituted constraints.  on_attempt's `extra` is the list of
    every sweep's (iterations, converged, n_unsatisfied) of that round.  Returns x, guard, params_reached."""

    def solve(xs, pu, active):
        x = xs.copy()
        conv, nun = np.zeros(len(xs), np.int64), np.zeros(len(xs), np.int64)
        info = [None] * len(xs)
        for b in np.nonzero(active)[0]:
            rc, xo, it, c, u = O.solve_batch(substituted(recs, pos, pu[b]), xs[b][None, :], cfg, linsolve=O.LINSOLVE_SPARSE)
            assert rc == 0
            x[b], conv[b], nun[b] = xo[0], int(c[0]), int(u[0])
            info[b] = (int(it[0]), int(c[0]), int(u[0]))
        return x, conv, nun, info

    x, g, reached, _, _ = run_rule(solve, x0, params0, params, on_attempt=on_attempt, **{**DEFAULT_GUARD, **guard})
    return x, g, reached


def params_entry_rule(system, pos, x0, params0, params, config=None, warn_cap=0, **guard):
    """The rule over System.solve_batch_params (the C entry, for the warning log): THE DEFINITION.  Returns a dict of every output
    of ezpz_system_sweep_guarded: x, status, mask, guard, params_reached, and log [steps, batch, warn_cap] with the entries
    behind a row's n_warnings zero."""
    import ezpz_amd
    from ezpz_amd._lib import STATUS_DTYPE

    pos = np.ascontiguousarray(pos, dtype=np.uint32)
    cfg = (config or ezpz_amd.Config())._c()
    n_cs = max(len(system.records), 1)

    def solve(xs, pu, active):
        batch = len(xs)
        xs, pu = np.ascontiguousarray(xs), np.ascontiguousarray(pu)
        x, st = np.empty_like(xs), np.zeros(batch, dtype=STATUS_DTYPE)
        mask = np.zeros((batch, n_cs), dtype=np.uint8)
        log = np.zeros((batch, max(warn_cap, 1)), dtype=np.uint64)
        rc = ezpz_amd.lib().ezpz_system_solve_batch_params(system._h, xs.ctypes.data, pos.ctypes.data, len(pos), pu.ctypes.data, batch,
                                                           C.byref(cfg), x.ctypes.data, st.ctypes.data, mask.ctypes.data,
                                                           log.ctypes.data if warn_cap else None, warn_cap)
        assert rc == 0, rc
        return x, st["converged"], st["n_unsatisfied"], (st, mask, log[:, :warn_cap])

    x, g, reached, last, rounds = run_rule(solve, x0, params0, params, **{**DEFAULT_GUARD, **guard})
    steps, batch = g.shape
    st = np.zeros((steps, batch), dtype=STATUS_DTYPE)
    mask = np.zeros((steps, batch, n_cs), dtype=np.uint8)
    log = np.zeros((steps, batch, warn_cap), dtype=np.uint64)
    for k in range(steps):  # (a row of a round's log is zero behind the n_warnings entries the host form copied)
        for r, (s_, m_, l_) in enumerate(rounds[k]):
            sel = last[k] == r
            st[k, sel], mask[k, sel], log[k, sel] = s_[sel], m_[sel], l_[sel]
    return dict(x=x, status=st, mask=mask, guard=g, params_reached=reached, log=log)


def guarded(system, pos, x0, params0, params, config=None, warn_cap=0, **guard):
    """System.sweep_guarded with every output, as the dict params_entry_rule returns."""
    import ezpz_amd

    steps, batch = params.shape[:2]
    log = np.zeros((steps, batch, warn_cap), dtype=np.uint64)
    x, st, mask, g, reached = system.sweep_guarded(x0, pos, params0, params, guard=ezpz_amd.GuardConfig(**{**DEFAULT_GUARD, **guard}),
                                                   config=config, want_mask=True, warn_log=log if warn_cap else None)
    return dict(x=x, status=st, mask=mask, guard=g, params_reached=reached, log=log)


def assert_same_outputs(got, want, what):
    """Every output byte for byte; a row of the warning log as the sorted entries the last attempt wrote (lanes append to it in
    no defined order, in the sweep as in the params entry), nothing behind them."""
    for key in ("x", "status", "mask", "guard", "params_reached"):
        a, b = got[key], want[key]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, key, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint8).reshape(a.shape[:2] + (-1,)) != b.view(np.uint8).reshape(b.shape[:2] + (-1,)))
            raise AssertionError((what, key, "first difference at (step, sweep, byte)", bad[0].tolist(), len(bad)))
    assert got["log"].shape == want["log"].shape, what
    if got["log"].shape[2]:
        assert np.array_equal(np.sort(got["log"], axis=2), np.sort(want["log"], axis=2)), (what, "log")


# ---- the crank: P0 fixed at the origin, P1 a unit away, its x driven ----------------------------------------------------------------
def crank():
    """(records, position of the driven constraint, x0, params0): P1 = (p, sqrt(1 - p^2)) while |p| <= 1, and no solution beyond."""
    recs = O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.distance((0, 1), (2, 3), 1.0), O.fixed(2, 0.2)])
    return recs, np.asarray([3], dtype=np.uint32), np.asarray([[0.0, 0.0, 0.2, 0.9797959]]), np.asarray([[0.2]])


CRANK_TARGETS = [0.5, 0.9, 1.4, 1.4, 0.6]
CRANK_MAX_MOVE = 0.25
# step: (reached, attempts, accepted, params_reached) with max_move 0.25 and the defaults otherwise
CRANK_TABLE = [(1.0, 3, 2, 0.5), (1.0, 5, 3, 0.9), (0.1875, 7, 2, 0.99375), (0.0, 5, 0, 0.99375), (1.0, 11, 8, 0.6)]
CRANK_PLAIN_TARGETS = [0.5, 1.4, 0.6]
CRANK_PLAIN_TABLE = [(1.0, 1), (0.0, 1), (1.0, 1)]  # (reached, attempts) with max_halvings 0 and max_move 0


def crank_params(targets):
    return np.asarray(targets, dtype=np.float64).reshape(-1, 1, 1)


def guard_table(g, reached):
    """[(reached, attempts, accepted, params_reached)] of sweep 0, driven value 0."""
    return [(float(g["reached"][k, 0]), int(g["attempts"][k, 0]), int(g["accepted"][k, 0]), float(reached[k, 0, 0])) for k in range(len(g))]


# ---- the GPU tests' shapes and their random-walk inputs ----------------------------------------------------------------------------
def guarded_shapes(E):
    """name -> (records, guesses, team_size, expected team_mode): the three shapes the device form serves."""
    recs, g, _ = CASES["distance"]
    crecs, cg = chain(40)
    rrecs, rg = record_walk_sketch()
    return {"sub-wavefront teams": (recs, g, E.TEAM_AUTO_LISTS, 0), "barrier workgroup": (crecs, cg, 256, 2),
            "record walk": (rrecs, rg, E.TEAM_LATENCY_RECORDS, 4)}


# (amplitude, jitter, max_move) of each shape's walk: steps large enough against max_move that some attempts are rejected for
# their displacement and the sweeps of a wavefront, and of a workgroup, take different numbers of attempts -- the tests assert it
# (the record walk's sketch answers a change of 0.01 in its dimensions with displacements of up to 0.8: a smaller walk)
WALKS = {"sub-wavefront teams": (0.45, 0.03, 0.3), "barrier workgroup": (0.2, 0.03, 0.3), "record walk": (0.01, 0.01, 0.25)}


def walk_inputs(E, name, recs, g, sweeps, steps, seed, n_drive=None):
    """(positions, params0 [sweeps, k] -- the records' own values --, params, x0, max_move) of a shape's walk."""
    amplitude, jitter, max_move = WALKS[name]
    # (x0 belongs to params0: the walk starts at the oracle's answer for the records' own values, jittered, not at the guesses)
    rc, solved, _, conv, _ = O.solve_batch(recs, np.asarray(g, dtype=np.float64)[None, :], None, linsolve=O.LINSOLVE_SPARSE)
    assert rc == 0 and conv[0] == 1
    pos, params, x0 = driven_walk(E, recs, solved[0], sweeps, steps, seed, amplitude=amplitude, jitter=jitter, n_drive=n_drive)
    params0 = np.ascontiguousarray(np.tile(recs["param"][pos].astype(np.float64), (sweeps, 1)))
    return pos, params0, params, x0, max_move
