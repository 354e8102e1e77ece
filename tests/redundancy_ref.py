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

# ---- drawn inputs: every placement and batch grouping (tests/test_gpu_redundancy.py: fuzz, grouping, grid loop) ------------------
def relabel(recs, perm):
    """The records with variable v renamed perm[v]."""
    out = O.stack(recs).copy()
    perm = np.asarray(perm, dtype=np.uint32)
    for c in out:
        k = O.KIND_NUM_IDS[int(c["kind"])]
        c["ids"][:k] = perm[c["ids"][:k]]
    return out


def components(recs, n_vars):
    """[(m, n)] of the connected components of the Jacobian's row / variable graph (O.nonzeroes: the variables a row depends on,
    fewer than the record names for the axis-aligned kinds), by union-find: what csrc/freedom.hip: build_freedom finds,
    restated.  A variable in no row is no component."""
    parent = list(range(n_vars))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    rows = [[int(v) for v in row] for c in recs for row in O.nonzeroes(c)]
    for row in rows:
        for v in row[1:]:
            parent[find(v)] = find(row[0])
    m, n = {}, {}
    for row in rows:
        m[find(row[0])] = m.get(find(row[0]), 0) + 1
    for v in {v for row in rows for v in row}:
        n[find(v)] = n.get(find(v), 0) + 1
    return [(m[k], n[k]) for k in sorted(m)]


LANE, TEAM_LDS, TEAM_GLOBAL = "lane", "team_lds", "team_global"


def component_ws(m, n, shared, with_l):
    """csrc/redundancy.hip.hpp: component_ws, restated."""
    pm = min(m, n)
    ld = ((n + 1) | 1) if shared else n + 1
    return m * ld + m + 3 * pm + (pm * pm if with_l else 0)


def placement(recs, n_vars, with_focus):
    """Where csrc/redundancy.hip: redundancy_device runs the call, restated: (placement, systems per workgroup, threads, largest n).
    LANE while the largest private workspace is at most 64 doubles; else one workgroup per system, the workspace in LDS while it
    fits 128 KiB beside the 17 doubles in front of it."""
    comps = components(recs, n_vars)
    max_n = max(n for _, n in comps)
    if max(component_ws(m, n, False, with_focus) for m, n in comps) <= 64:
        return LANE, (1 if len(comps) >= 128 else 128 // len(comps)), 128, max_n
    ws = max(component_ws(m, n, True, with_focus) for m, n in comps)
    return (TEAM_LDS if (17 + ws) * 8 <= 128 * 1024 else TEAM_GLOBAL), 1, (1024 if max_n > 64 else 256), max_n


REPEAT_WEIGHTS = (1.0, 2.5, 0.5)


def mosaic(sizes, seed, shuffle=True, blocks=()):
    """Several components of different sizes in one system.  A size of 1 is one fixed variable, any other size a
    gen.connected_sketch of that many points at its polished values, each on a variable range of its own; three records of every
    part (drawn) come again: the first as it is, the second with its parameter moved by 0.3 where that offsets the residual, the
    third as it is, each with a weight from REPEAT_WEIGHTS.  `blocks`: ready parts (recs, n_vars, x [n_vars]) taken as they are.  The
    record list is permuted, so the components' rows interleave in request order; `origin` [(part, record of the part)] says where
    every record came from.  The focus list: the first six constraints the reference calls redundant or conflicting."""
    rng = np.random.default_rng([seed, 77])
    parts = []
    for k, size in enumerate(sizes):
        if size == 1:
            value = float(rng.uniform(0.5, 4.0))
            recs, x = O.stack([O.fixed(0, value)]), np.asarray([value])
        else:
            recs, g = gen.connected_sketch(size, seed * 131 + k)
            x = polished(recs, g)[0]
        extra = []
        for j, i in enumerate(rng.choice(len(recs), 3, replace=len(recs) < 3)):
            c = recs[i].copy()
            if j == 1 and int(c["kind"]) in VALUE_KINDS:
                c["param"] = float(c["param"]) + 0.3
            c["weight"] = REPEAT_WEIGHTS[int(rng.integers(0, 3))]
            extra.append(c)
        parts.append((O.stack(list(recs) + extra), len(x), x))
    parts += [(O.stack(r), int(n), np.asarray(x, dtype=np.float64)) for r, n, x in blocks]
    all_recs, xs, origin, off = [], [], [], 0
    for k, (recs, n, x) in enumerate(parts):
        all_recs += list(relabel(recs, off + np.arange(n)))
        origin += [(k, i) for i in range(len(recs))]
        xs.append(x)
        off += n
    order = rng.permutation(len(all_recs)) if shuffle else np.arange(len(all_recs))
    recs = O.stack([all_recs[i] for i in order])
    x = np.concatenate(xs)[None, :]
    flagged = np.nonzero(analyse(recs, off, x[0])["con_status"] >= REDUNDANT)[0]
    return dict(recs=recs, n_vars=off, x=x, focus=[int(f) for f in flagged[:6]], origin=[origin[i] for i in order])


def _draw_fuzz(count=44, seed=20240611):
    """(sizes, seed) pairs: the largest part goes round LARGEST (every lane-group width, thread count and workspace home; a largest
    part of two points is LANE without a focus list and TEAM with one), one to four more parts no larger are drawn."""
    largest = (1, 2, 2, 4, 7, 12, 17, 28, 36, 45)
    pool = (1, 1, 2, 3, 5, 7, 9, 12, 17, 24, 36)
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        top = largest[k % len(largest)]
        rest = [int(v) for v in rng.choice([p for p in pool if p <= top], int(rng.integers(1, 5)))]
        sizes = rest + [top]
        rng.shuffle(sizes)
        out.append((tuple(int(v) for v in sizes), int(rng.integers(0, 10000))))
    return out


FUZZ_DRAWN = _draw_fuzz()
# the drawn systems with a row inside a band of test_inputs_keep_their_distance_from_the_tolerances (test_redundancy_cpu.py holds
# this list to what the reference finds, and to a tenth of the draws)
FUZZ_REJECTED = ()
FUZZ = [f for k, f in enumerate(FUZZ_DRAWN) if k not in FUZZ_REJECTED]


def within_margins(ref):
    """The bands of test_inputs_keep_their_distance_from_the_tolerances: what lies inside them ([] when the input is fair)."""
    bad = []
    tau = ref["tau"][~np.isnan(ref["tau"])]
    bad += [("tau", v) for v in tau[(tau >= 1e-11) & (tau <= 1e-3)]]
    rho = ref["rho_w"][~np.isnan(ref["rho_w"])]
    bad += [("rho", v) for v in rho[(rho >= 1e-7) & (rho <= 1e-2)]]
    for per_focus in ref["ratios"]:
        for ratio in per_focus:
            bad += [("ratio", v) for v in ratio[(ratio >= 1e-9) & (ratio <= 1e-3)]]
    return bad


def coincident(b, c, seed):
    """About a third of the (system, component) pairs of pairs(), by a keyed hash."""
    h = (b * 2654435761 + c * 40503 + seed * 7919 + 12345) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 2246822519) & 0xFFFFFFFF
    h ^= h >> 13
    return h % 3 == 0


def pairs(ncomp, batch, seed):
    """The LANE batch whose systems differ: `ncomp` components of two points p, q with distance(p, q, d) and distance(p, q, d'),
    d' = d (REDUNDANT) or d + 0.3 (CONFLICTING) by component; values drawn in [0.5, 4], and q = p where coincident() says so -- the
    guard leaves both rows without entries there, ZERO, in that system only.  18 workspace doubles per component, 22 with groups."""
    rng = np.random.default_rng([seed, ncomp])
    recs, moved = [], []
    for c in range(ncomp):
        d = float(rng.uniform(0.5, 4.0))
        moved.append(bool(rng.integers(0, 2)))
        p, q = (4 * c, 4 * c + 1), (4 * c + 2, 4 * c + 3)
        recs += [O.distance(p, q, d), O.distance(p, q, d + 0.3 if moved[-1] else d, weight=REPEAT_WEIGHTS[c % 3])]
    x = gen.keyed_uniform(seed, batch, 4 * ncomp, 0.5, 4.0)
    for b in range(batch):
        for c in range(ncomp):
            if coincident(b, c, seed):
                x[b, 4 * c + 2: 4 * c + 4] = x[b, 4 * c: 4 * c + 2]
    focus = sorted({1, 2 * (ncomp // 2) + 1, 2 * ncomp - 1}) + [0]
    return dict(recs=O.stack(recs), n_vars=4 * ncomp, x=x, focus=focus, moved=moved, seed=seed)


def pairs_expected(c):
    """con_status [batch, 2 ncomp] of a pairs() case from how it was built."""
    want = np.zeros((len(c["x"]), len(c["recs"])), np.uint8)
    for b in range(len(c["x"])):
        for k, moved in enumerate(c["moved"]):
            want[b, 2 * k: 2 * k + 2] = [ZERO, ZERO] if coincident(b, k, c["seed"]) else [INDEPENDENT, CONFLICTING if moved else REDUNDANT]
    return want


def embedded():
    """The records of pairs:3 as one part of a mosaic beside a 24-point sketch (TEAM) and a fixed variable: `at` [6] says where they
    are; both systems of the block, the other parts' values twice; the block's focus list at its new positions."""
    block = case("pairs:3")
    m = mosaic([24, 1], 9, blocks=[(block["recs"], block["n_vars"], block["x"][0])])
    at = [m["origin"].index((2, i)) for i in range(len(block["recs"]))]
    x = np.repeat(m["x"], len(block["x"]), axis=0)
    x[:, -block["n_vars"]:] = block["x"]
    return dict(recs=m["recs"], n_vars=m["n_vars"], x=x, focus=[at[f] for f in block["focus"]], at=at)


def grid_lane():
    """65 components (G = 1) for the LANE grid loop: 64 fixed variables, each fixed once more (every third to another value), and
    one pairs() component in the middle of the record list; six systems, the pair coincident in three of them."""
    rng = np.random.default_rng(65)
    recs = []
    for v in range(64):
        value = float(rng.uniform(0.5, 4.0))
        recs += [O.fixed(v, value), O.fixed(v, value + (0.3 if v % 3 == 0 else 0.0), weight=REPEAT_WEIGHTS[v % 3])]
    p, q = (64, 65), (66, 67)
    recs[64:64] = [O.distance(p, q, 2.0), O.distance(p, q, 2.3, weight=2.5)]
    x = rng.uniform(0.5, 4.0, (6, 68))
    for b in (0, 3, 4):  # (no shift of the six repeats the pattern)
        x[b, 66:68] = x[b, 64:66]
    return dict(recs=O.stack(recs), n_vars=68, x=x, focus=[65, 1, 3, 129])


def grid_rectangle():
    """rectangle:side_conflict at three value vectors: polished, all zeros (the guards of the three distances fire) and polished with one
    corner moved up by 0.5: the long side that cannot hold leans, and the horizontal joins what it is made of."""
    c = rectangle("side_conflict")
    moved = c["x"][0].copy()
    moved[7] += 0.5
    return dict(c, x=np.stack([c["x"][0], np.zeros(8), moved]))


def grid_sketch():
    """The 45-point sketch (workspace in global memory with its focus list): three polished starts and all zeros, the zeros twice: a period
    of five does not divide the 1024 workgroups, so a workgroup's second round differs from its first."""
    c = sketch(45, 11, 0, 3)
    zero = np.zeros((1, c["n_vars"]))
    return dict(c, x=np.vstack([c["x"][:1], zero, c["x"][1:], zero]))


# (components, batch): 3 G + 1 systems at G = 128 / components systems per workgroup; 150 components: lanes 0 .. 21 take two
PAIRS = {f"pairs:{n}": (pairs, (n, b, 3)) for n, b in ((30, 13), (63, 7), (1, 385), (150, 3))}
DRAWN = dict(PAIRS)
DRAWN["pairs:3"] = (pairs, (3, 2, 15))
DRAWN["pairs:3:embedded"] = (embedded, ())
DRAWN["grid:lane"] = (grid_lane, ())
DRAWN["grid:rectangle"] = (grid_rectangle, ())
DRAWN["grid:sketch45"] = (grid_sketch, ())
for _k, (_sizes, _seed) in enumerate(FUZZ_DRAWN):
    DRAWN[f"fuzz:{_k}"] = (mosaic, (list(_sizes), _seed))
FUZZ_NAMES = [f"fuzz:{k}" for k in range(len(FUZZ_DRAWN)) if k not in FUZZ_REJECTED]

_BUILT, _REFS = {}, {}


def case(name):
    if name not in _BUILT:
        fn, args = CASES[name] if name in CASES else DRAWN[name]
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
