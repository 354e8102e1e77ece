"""The redundancy analysis of include/ezpz_amd.h (ezpz_system_redundancy) restated in numpy, float64, and the inputs the CPU and
GPU tests share.  J, r and w come from the CPU oracle (oracle.residual, oracle.jacobian_rows, times the weight), rows in request
order; the analysis runs on the whole matrix (the device runs it per connected component: the same result).

analyse() also returns what the statuses were decided on -- per row tau = ||v|| / ||a|| and |rho| / w, per focus entry the
coefficient ratios |c_j| ||a_j|| / ||a_i|| -- so that test_redundancy_cpu.py can hold every input of the GPU tests to a margin
around the tolerances: a status the device and this file could disagree on by rounding is not a test input."""
import numpy as np

import gen
from oracle import oracle as O
from sensitivity_ref import jacobian

INDEPENDENT, ZERO, REDUNDANT, CONFLICTING = 0, 1, 2, 3
RANK_TOL, CONFLICT_TOL, GROUP_TOL = 1e-6, 1e-4, 1e-6


def matrices(recs, n_vars, x):
    """(J [m, n] weighted, r [m] weighted, w [m], row_con [m])."""
    J = jacobian(recs, x, n_vars)
    r, w, con = [], [], []
    for i in range(len(recs)):
        ri, _ = O.residual(recs[i], x)
        r += [float(recs[i]["weight"]) * v for v in ri]
        w += [float(recs[i]["weight"])] * len(ri)
        con += [i] * len(ri)
    return J, np.asarray(r), np.asarray(w), np.asarray(con, dtype=int)


def analyse(recs, n_vars, x, focus=(), rank_tol=RANK_TOL, conflict_tol=CONFLICT_TOL, group_tol=GROUP_TOL):
    J, r, w, row_con = matrices(recs, n_vars, x)
    m, n_cs = len(r), len(recs)
    Q, s, acc, L = np.zeros((0, n_vars)), np.zeros(0), [], []
    norm = np.sqrt((J * J).sum(axis=1))
    row_status = np.zeros(m, np.uint8)
    tau = np.full(m, np.nan)
    rho_w = np.full(m, np.nan)
    focus = [int(f) for f in focus]
    group = np.zeros((len(focus), n_cs), np.uint8)
    ratios = [[] for _ in focus]  # per focus entry: one array of |c_j| ||a_j|| / ||a_i|| per dependent row
    for i in range(m):
        a, rho = J[i].copy(), r[i]
        if norm[i] == 0.0:
            row_status[i] = ZERO
            continue
        v, hs = a.copy(), np.zeros(len(acc))
        for _ in range(2):  # classical Gram-Schmidt, twice
            h = Q @ v
            v = v - h @ Q
            rho = rho - h @ s
            hs += h
        nv = np.sqrt(v @ v)
        tau[i] = nv / norm[i]
        if tau[i] > rank_tol:
            row_status[i] = INDEPENDENT
            Q = np.vstack([Q, v / nv])
            s = np.append(s, rho / nv)
            L.append(np.append(hs, nv))
            acc.append(i)
            continue
        rho_w[i] = abs(rho) / w[i]
        row_status[i] = CONFLICTING if rho_w[i] > conflict_tol else REDUNDANT
        if int(row_con[i]) in focus:
            k = focus.index(int(row_con[i]))
            p = len(acc)
            Lm = np.zeros((p, p))
            for q, row in enumerate(L):
                Lm[q, : q + 1] = row
            c = np.linalg.solve(Lm.T, hs) if p else np.zeros(0)  # a_i = sum c_j a_(acc j): A_accepted = L Q
            ratio = np.abs(c) * norm[acc] / norm[i] if p else np.zeros(0)
            ratios[k].append(ratio)
            for j in np.nonzero(ratio > group_tol)[0]:
                group[k, row_con[acc[j]]] = 1
            group[k, row_con[i]] = 1
    con_status = np.zeros(n_cs, np.uint8)
    np.maximum.at(con_status, row_con, row_status)
    return dict(con_status=con_status, row_status=row_status, rank=int((row_status == INDEPENDENT).sum()), group=group, tau=tau,
                rho_w=rho_w, ratios=ratios, J=J, accepted=acc, row_con=row_con)


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------
def polished(recs, x0):
    """The oracle's answers [B, n] at residual_tolerance 1e-13: what holds on the solution set holds there to rounding."""
    x0 = np.atleast_2d(np.asarray(x0, dtype=np.float64))
    rc, x, _, _, _ = O.solve_batch(recs, x0, O.Config(max_iterations=80, residual_tolerance=1e-13, step_tolerance=1e-15), linsolve=O.LINSOLVE_SPARSE)
    assert rc == 0
    return x


P = lambda i: (2 * i, 2 * i + 1)


def one_variable(kind, order, weights):
    """fixed(v, 1) with a second fixed(v, .): the same value (`dup`) or 2 (`conflict`), either record first, weighted."""
    a, b = O.fixed(0, 1.0, weight=weights[0]), O.fixed(0, 1.0 if kind == "dup" else 2.0, weight=weights[1])
    recs = O.stack([a, b] if order == 0 else [b, a])
    return dict(recs=recs, n_vars=1, x=polished(recs, [[0.3]]), focus=[1])


RECTANGLE = [O.fixed(0, 0.0), O.fixed(1, 0.0), O.horizontal(P(0), P(1)), O.vertical(P(1), P(2)), O.horizontal(P(2), P(3)),
             O.vertical(P(3), P(0)), O.distance(P(0), P(1), 4.0), O.distance(P(1), P(2), 3.0)]
RECTANGLE_EXTRA = {
    "equal_length": O.lines_equal_length(P(0), P(1), P(3), P(2)),
    "side_weighted": O.distance(P(2), P(3), 4.0, weight=0.5),
    "side_conflict": O.distance(P(2), P(3), 4.5),
    "coincident": O.points_coincident(P(0), P(3)),
}


def rectangle(extra):
    """Eight records that determine a 4 x 3 rectangle, one more that does not add anything -- or cannot hold."""
    x = polished(O.stack(RECTANGLE), [[0.1, -0.1, 3.8, 0.2, 4.1, 2.9, -0.2, 3.2]])
    return dict(recs=O.stack(RECTANGLE + [RECTANGLE_EXTRA[extra]]), n_vars=8, x=x, focus=[8, 6])


def zero_row():
    """distance(p, q, d) at p == q: the guard leaves the row without entries."""
    recs = O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.distance(P(0), P(1), 1.0), O.fixed(2, 0.0)])
    return dict(recs=recs, n_vars=4, x=np.zeros((1, 4)), focus=[2])


VALUE_KINDS = (O.DISTANCE, O.VERTICAL_DISTANCE, O.HORIZONTAL_DISTANCE, O.FIXED, O.CIRCLE_RADIUS, O.ARC_RADIUS, O.POINT_LINE_DISTANCE,
               O.VERTICAL_POINT_LINE_DISTANCE, O.HORIZONTAL_POINT_LINE_DISTANCE)  # the parameter is an offset of the residual


def all_kinds(moved):
    """Every kind once on variables of its own (gen.arb_constraint, ids made distinct), then every record again: as it is, or --
    `moved`, the nine kinds whose parameter offsets the residual -- with the parameter moved by 0.3.  Values drawn, not solved: a
    repeated row depends on the first whatever the values.  (The parameter of the three angle kinds and of arc_length turns the
    Jacobian: a copy with another value is a row of its own, not a dependent one, so these are repeated as they are in both.)"""
    rng = np.random.default_rng(2024)
    first, second, n = [], [], 0
    for kind in range(25):
        c = gen.arb_constraint(rng, kind)
        k = O.KIND_NUM_IDS[kind]
        c["ids"][:k] = n + rng.permutation(k)
        n += k
        first.append(c)
        d = c.copy()
        if moved and int(c["kind"]) in VALUE_KINDS:
            d["param"] = float(c["param"]) + 0.3
        second.append(d)
    x = rng.uniform(0.5, 4.0, (2, n))
    return dict(recs=O.stack(first + second), n_vars=n, x=x, focus=None)


def blocks(batch=130, lines=40):
    """massive40: 40 lines = 120 components of one or two variables; every 5th line repeats a record, every 7th gets one that
    cannot hold.  Linear, so every system's own values (drawn, not solved) see the same dependencies."""
    from ezpz_amd import synthetic

    base = O.stack(np.ascontiguousarray(synthetic.make_workload("massive%d" % lines)[1]))
    extra = []
    for k in range(lines):
        if k % 5 == 0:
            extra.append(O.fixed(4 * k, float(k), weight=2.0))  # p_a.x = k once more
        if k % 7 == 0:
            extra.append(O.fixed(4 * k + 3, 4.5))  # p_b.y = 4 is there already
    recs = O.stack(list(base) + extra)
    x = gen.keyed_uniform(17, batch, 4 * lines, -2.0, 6.0)
    return dict(recs=recs, n_vars=4 * lines, x=x, focus=[len(base), len(base) + 1, 3, len(recs) - 1])


def sketch(npts, seed, dropped, batch):
    """gen.connected_sketch with three records repeated, two repeated with another value and one scaled combination of rows (a
    weighted horizontal distance between two placed points, at its true value); `dropped`: without the second record of each of
    the last `dropped` points (fewer rows than variables; what the appended records touch stays determined)."""
    recs, g = gen.connected_sketch(npts, seed)
    rng = np.random.default_rng(seed + 1)
    x = polished(recs, g[None, :] + rng.uniform(-0.01, 0.01, (batch, 2 * npts)))
    base = [recs[i] for i in range(len(recs)) if not (i >= len(recs) - 2 * dropped and i % 2 == 1)]
    early = npts // 2
    dist = [i for i in range(len(base) - 2 * 4) if int(base[i]["kind"]) == O.DISTANCE]
    dup = [3, dist[len(dist) // 2], len(base) // 2 | 1]
    extra = [base[i].copy() for i in dup]
    for i in (dist[1], dist[-1]):
        c = base[i].copy()
        c["param"] = float(c["param"]) + 0.3
        extra.append(c)
    extra.append(O.horizontal_distance(P(early), P(early - 1), float(x[0][2 * early] - x[0][2 * (early - 1)]), weight=2.5))
    out = O.stack(base + extra)
    nb = len(base)
    return dict(recs=out, n_vars=2 * npts, x=x, focus=[nb + 3, nb + 5, nb + 4, 5, nb])


CASES = {}
for _kind in ("dup", "conflict"):
    for _order in (0, 1):
        for _w in ((1.0, 1.0), (1e-3, 1.0), (1.0, 1e-3)):
            CASES[f"one_variable:{_kind}:{_order}:{_w[0]:g}:{_w[1]:g}"] = (one_variable, (_kind, _order, _w))
for _extra in RECTANGLE_EXTRA:
    CASES[f"rectangle:{_extra}"] = (rectangle, (_extra,))
CASES["zero_row"] = (zero_row, ())
CASES["all_kinds:repeated"] = (all_kinds, (False,))
CASES["all_kinds:moved"] = (all_kinds, (True,))
CASES["blocks"] = (blocks, ())
CASES["sketch24"] = (sketch, (24, 5, 0, 3))          # TEAM, workspace in LDS, more rows than variables
CASES["sketch24:dropped"] = (sketch, (24, 5, 10, 3))  # ... fewer rows than variables
CASES["sketch150"] = (sketch, (150, 7, 0, 3))        # TEAM, workspace in global memory

_BUILT, _REFS = {}, {}


def case(name):
    if name not in _BUILT:
        fn, args = CASES[name]
        _BUILT[name] = fn(*args)
    return _BUILT[name]


def references(name, systems=None):
    """analyse() of every system of a case (or of the first `systems`), computed once."""
    c = case(name)
    nb = len(c["x"]) if systems is None else min(systems, len(c["x"]))
    have = _REFS.setdefault(name, [])
    while len(have) < nb:
        have.append(analyse(c["recs"], c["n_vars"], c["x"][len(have)], c["focus"] or ()))
    return have[:nb]
