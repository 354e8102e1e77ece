"""What the sweep tests share (ezpz_system_sweep_params; tests/test_sweep_cpu.py, tests/test_gpu_sweep.py): the small per-kind
systems, the launch shapes, the paths the driven parameters take, the chain of params calls a sweep is defined as, and the
oracle run once per (sweep, step)."""
import numpy as np

from oracle import oracle as O
from oracle import textual as T
from sensitivity import residual_inf

P0, P1, P2, P3 = (0, 1), (2, 3), (4, 5), (6, 7)
SWEEPS, STEPS = 64, 12  # the oracle test's sweeps and steps per sweep


def _fix(values):
    return [O.fixed(i, float(v)) for i, v in values]


def kind_cases():
    """kind -> (records, guesses, [(position, nominal, half-width of the range)]): small, determined, well-conditioned systems in
    which the constraint under test decides at least one coordinate (the systems and ranges of the params entry's tests)."""
    c = {}
    c["distance"] = (_fix([(0, 0), (1, 0)]) + [O.horizontal(P0, P1), O.distance(P0, P1, 2.0)], [0, 0, 2.1, 0.1], [(3, 2.0, 0.5)])
    c["axis_distances_and_fixed"] = (_fix([(0, 1), (1, -1)]) + [O.vertical_distance(P1, P0, 1.5), O.horizontal_distance(P1, P0, 2.5)],
                                     [1, -1, 3, 1], [(0, 1.0, 0.5), (1, -1.0, 0.5), (2, 1.5, 1.0), (3, 2.5, 1.0)])
    c["circle_radius"] = (_fix([(0, 0), (1, 1)]) + [O.circle_radius(P0, 2, 1.5)], [0, 1, 1.0], [(2, 1.5, 1.0)])
    c["arc_radius"] = (_fix([(0, 0), (1, 0), (3, 0), (4, 0)]) + [O.arc_radius(P0, P1, P2, 2.0)], [0, 0, 2.1, 0, 0, 1.9], [(4, 2.0, 0.5)])
    line = _fix([(2, 0), (3, 0), (4, 4), (5, 0)])
    c["point_line_distance"] = (line + _fix([(0, 1)]) + [O.point_line_distance(P0, P1, P2, 1.5)], [1, 1.4, 0, 0, 4, 0], [(5, 1.5, 1.0)])
    c["vertical_point_line_distance"] = (line + _fix([(0, 1)]) + [O.vertical_point_line_distance(P0, P1, P2, 1.5)],
                                         [1, 1.4, 0, 0, 4, 0], [(5, 1.5, 1.0)])
    c["horizontal_point_line_distance"] = (_fix([(2, 0), (3, 0), (4, 0), (5, 4), (1, 1)]) + [O.horizontal_point_line_distance(P0, P1, P2, 1.5)],
                                           [1.4, 1, 0, 0, 0, 4], [(5, 1.5, 1.0)])
    c["arc_length"] = (_fix([(0, 0), (1, 0), (2, 2), (3, 0)]) + [O.arc_length(P0, P1, P2, 2.0)], [0, 0, 2, 0, 1.1, 1.7], [(4, 2.0, 0.4)])
    for unit, nominal, half in (("deg", 30.0, 15.0), ("rad", 0.5, 0.25)):
        c["lines_at_angle_" + unit] = (_fix([(0, 0), (1, 0), (2, 2), (3, 0), (4, 0), (5, 0)]) +
                                       [O.distance(P2, P3, 2.0), O.lines_at_angle(P0, P1, P2, P3, (unit, nominal))],
                                       [0, 0, 2, 0, 0, 0, 1.7, 1.0], [(7, nominal, half)])
        c["arc_angle_" + unit] = (_fix([(0, 0), (1, 0), (2, 2), (3, 0)]) + [O.distance(P0, P2, 2.0), O.arc_angle(P0, P1, P2, (unit, nominal))],
                                  [0, 0, 2, 0, 1.7, 1.0], [(5, nominal, half)])
        c["points_at_angle_" + unit] = (_fix([(0, 0), (1, 0), (2, 2), (3, 0)]) + [O.points_at_angle(P0, P1, P2, (unit, nominal))],
                                        [0, 0, 2, 0, 1.7, 1.0], [(4, nominal, half)])
    return {k: (O.stack(cons), np.asarray(g, dtype=float), drv) for k, (cons, g, drv) in c.items()}


CASES = kind_cases()


def paths(driven, sweeps, steps, seed):
    """(positions, params [steps, sweeps, k]): every driven parameter moves linearly across nominal - half .. nominal + half, one
    range per steps - 1 steps, from a random phase in a random direction per sweep (turning round at the ends of the range)."""
    rng = np.random.default_rng(seed)
    pos = np.asarray([p for p, _, _ in driven], dtype=np.uint32)
    k = np.arange(steps)[:, None, None] / max(steps - 1, 1)
    phase = rng.uniform(0.0, 1.0, (1, sweeps, len(driven)))
    direction = rng.choice([-1.0, 1.0], (1, sweeps, len(driven)))
    u = np.abs((phase + direction * k + 1.0) % 2.0 - 1.0)  # a triangle wave of period 2 through [0, 1]
    nom = np.asarray([n for _, n, _ in driven])[None, None, :]
    half = np.asarray([h for _, _, h in driven])[None, None, :]
    return pos, np.ascontiguousarray(nom - half + 2.0 * half * u)


def oracle_inputs(name, seed=7):
    """The inputs of the oracle test for one kind: positions, params [STEPS, SWEEPS, k], starts [SWEEPS, n] jittered by +-0.05."""
    recs, g, driven = CASES[name]
    pos, params = paths(driven, SWEEPS, STEPS, seed)
    x0 = g[None, :] + np.random.default_rng(seed + 1).uniform(-0.05, 0.05, (SWEEPS, len(g)))
    return recs, pos, params, x0


def substituted(recs, pos, row):
    r = recs.copy()
    r["param"][pos] = row
    return r


def oracle_chain(recs, pos, params, x0, starts=None, cfg=None):
    """The oracle once per (sweep, step) on the substituted constraints.  Step k starts from the oracle's own answer of step k - 1 --
    or, with `starts` [steps, sweeps, n] (a device's answers), from starts[k - 1]: every step is then judged on its own, and an
    error within the bar at one step is not carried into the next.  Returns x [steps, sweeps, n], iterations, converged,
    n_unsatisfied [steps, sweeps], mask [steps, sweeps, n_cs], and the start of every step."""
    steps, sweeps = params.shape[:2]
    n = x0.shape[1]
    x = np.zeros((steps, sweeps, n))
    begin = np.zeros((steps, sweeps, n))
    it, conv, nun = (np.zeros((steps, sweeps), np.int64) for _ in range(3))
    mask = np.zeros((steps, sweeps, len(recs)), np.uint8)
    for b in range(sweeps):
        for k in range(steps):
            start = x0[b] if k == 0 else (x[k - 1, b] if starts is None else starts[k - 1, b])
            r = substituted(recs, pos, params[k, b])
            rc, xs, i, c, u = O.solve_batch(r, start[None, :], cfg, linsolve=O.LINSOLVE_SPARSE)
            assert rc == 0
            begin[k, b], x[k, b], it[k, b], conv[k, b], nun[k, b] = start, xs[0], int(i[0]), int(c[0]), int(u[0])
            mask[k, b, sorted(residual_inf(r, xs[0])[1])] = 1
    return x, it, conv, nun, mask, begin


def chain_of_calls(system, x0, pos, params, config=None, want_mask=True):
    """A sweep as its definition: `steps` calls of solve_batch_params, each from the answer of the one before."""
    xs, sts, masks = [], [], []
    x = np.ascontiguousarray(x0, dtype=np.float64)
    for k in range(params.shape[0]):
        x, st, mask = system.solve_batch_params(x, pos, params[k], config=config, want_mask=want_mask)
        xs.append(x), sts.append(st), masks.append(mask)
    return np.stack(xs), np.stack(sts), (np.stack(masks) if want_mask else None)


def chain(n_pts):
    """A chain of points a unit apart, alternately horizontal and vertical: one connected component."""
    cons = [O.fixed(0, 0.0), O.fixed(1, 0.0)]
    guesses = [0.0, 0.0]
    for k in range(1, n_pts):
        a, b = (2 * (k - 1), 2 * k - 1), (2 * k, 2 * k + 1)
        cons.append(O.distance(a, b, 1.0))
        cons.append(O.horizontal(a, b) if k % 2 else O.vertical(a, b))
        guesses += [0.55 * k + 0.1, 0.45 * k - 0.1]
    return O.stack(cons), np.asarray(guesses)


def record_walk_sketch(npts=70):
    """One connected sketch whose linear solve is a record walk: points tied by a distance and a horizontal distance."""
    rng = np.random.default_rng(0)
    true = np.cumsum(rng.uniform(0.5, 2.0, (npts, 2)), axis=0)
    true[0] = 0.0
    cons = [O.fixed(0, 0.0), O.fixed(1, 0.0)]
    for i in range(1, npts):
        j = max(0, i - 2)
        cons += [O.distance((2 * i, 2 * i + 1), (2 * i - 2, 2 * i - 1), float(np.hypot(*(true[i] - true[i - 1])))),
                 O.horizontal_distance((2 * i, 2 * i + 1), (2 * j, 2 * j + 1), float(true[i][0] - true[j][0]))]
    return O.stack(cons), true.reshape(-1)


ROUTES = ("interpreter", "sub-wavefront teams", "partitioned workgroup", "barrier workgroup", "record walk")


def shapes(E):
    """(route name, records, guesses, team_size, expected team_mode) for the five launch shapes a sweep reaches."""
    recs, g, _ = CASES["distance"]
    out = [("sub-wavefront teams", recs, g, E.TEAM_AUTO_LISTS, 0)]
    ref = T.load(T.gen_big_problem(64))
    brecs = O.stack(ref.constraints)
    out.append(("partitioned workgroup", brecs, ref.guesses, E.TEAM_AUTO_LISTS, 1))
    out.append(("interpreter", brecs, ref.guesses, 0, 3))
    crecs, cg = chain(40)
    out.append(("barrier workgroup", crecs, cg, 256, 2))
    rrecs, rg = record_walk_sketch()
    out.append(("record walk", rrecs, rg, E.TEAM_LATENCY_RECORDS, 4))
    return out


def driven_walk(E, recs, g, sweeps, steps, seed, amplitude=0.1, jitter=0.03, n_drive=None):
    """Every parametrised constraint driven (or n_drive of them, spread over the list): params [steps, sweeps, k] a random walk
    around the system's own values that differs between consecutive steps and between sweeps, starts jittered."""
    rng = np.random.default_rng(seed)
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    if n_drive is not None:
        pos = np.ascontiguousarray(pos[np.linspace(0, len(pos) - 1, n_drive).astype(int)])
    params = recs["param"][pos][None, None, :] + rng.uniform(-amplitude, amplitude, (steps, sweeps, len(pos)))
    x0 = g[None, :] + rng.uniform(-jitter, jitter, (sweeps, len(g)))
    return pos, np.ascontiguousarray(params), x0
