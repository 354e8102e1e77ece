"""GPU tests (-m gpu) of the constraint evaluators at the edge cases of tests/edge_cases.py: guard thresholds one ulp either side,
branch cuts and signs of zero, duplicate ids, and scales from 2^-30 to 2^520 -- through eval_batch, System.measure (both
placements) and every solve route with max_iterations = 0 (one evaluation of residual and Jacobian, the warnings logged, the start
values returned), against the CPU oracle and the host function ezpz_constraint_measure.

Bars.  eval_batch: the bars of test_gpu_parity.py::test_residual_and_jacobian_match_oracle -- 1e-11 * max(1, |want|) for a residual
row, 1e-10 * max(1, |want|) for a Jacobian entry -- with the 1 of the residual bar replaced by the scale s = 2^k of the value vector
(power-of-two scaling is exact in every operation of the evaluators, so the error scales with the data); non-finite on both sides at
the same entries counts as equal.  At the designated (record, vector) pair of a guard case the rows are additionally exactly zero
where the table's plain-Python restatement of the reference's comparison says the guard fires, and not zero where it does not.
measure: the bars of test_gpu_measure.py.  Solve routes: everything bitwise or equal."""
import math

import numpy as np
import pytest

import edge_cases as T
import measure_ref as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROW, DIRECT, LAUNCHED = 52, 53, 51  # csrc/call_trace.hpp (tests/test_gpu_measure.py)
CFG0 = dict(max_iterations=0)


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


def _distinct(cases_recs):
    """The distinct records of a list, in order of first appearance, weights cycling through T.WEIGHTS; and each input's position."""
    seen, recs, pos = {}, [], []
    for rec in cases_recs:
        key = rec.tobytes()
        if key not in seen:
            seen[key] = len(recs)
            r = rec.copy()
            r["weight"] = T.WEIGHTS[len(recs) % len(T.WEIGHTS)]
            recs.append(r)
        pos.append(seen[key])
    return recs, pos


def _oracle_eval(recs, X):
    """(r [B, m], J [B, m, n], degenerate counts [B], first row of each record) by the oracle, weights applied as solver.rs:403 does."""
    dims = [O.residual_dim(c) for c in recs]
    first = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    B, m = len(X), int(first[-1])
    r, J, deg = np.zeros((B, m)), np.zeros((B, m, T.N_VARS)), np.zeros(B, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for i, c in enumerate(recs):
                rr, d0 = O.residual(c, X[b])
                rows, d1 = O.jacobian_rows(c, X[b])
                deg[b] += int(d0) + int(d1)
                w = float(c["weight"])
                for k in range(dims[i]):
                    r[b, first[i] + k] = w * rr[k]
                    for v, pd in rows[k]:
                        J[b, first[i] + k, v] += w * pd
    return r, J, deg, first


def _assert_close(kind, got_r, got_J, want_r, want_J, scale):
    """The parity bars, per value vector b with scale[b] in place of the 1 of the residual bar.  Returns the largest errors / bar."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(scale)[:, None]
        both = ~np.isfinite(want_r) & ~np.isfinite(got_r)
        err_r = np.where(both, 0.0, np.abs(got_r - want_r) / (1e-11 * np.maximum(s, np.abs(want_r))))
        assert not np.any(np.isnan(err_r)) and np.all(err_r <= 1.0), (O.KIND_NAMES[kind], "residual", np.argwhere(~(err_r <= 1.0))[:5].tolist(),
                                                                      got_r[~(err_r <= 1.0)][:5], want_r[~(err_r <= 1.0)][:5])
        both = ~np.isfinite(want_J) & ~np.isfinite(got_J)
        err_J = np.where(both, 0.0, np.abs(got_J - want_J) / (1e-10 * np.maximum(1.0, np.abs(want_J))))
        assert not np.any(np.isnan(err_J)) and np.all(err_J <= 1.0), (O.KIND_NAMES[kind], "jacobian", np.argwhere(~(err_J <= 1.0))[:5].tolist(),
                                                                      got_J[~(err_J <= 1.0)][:5], want_J[~(err_J <= 1.0)][:5])
    return err_r, err_J


# ---- eval_batch: every record of a kind's cases at every vector of that kind's cases -----------------------------------------------
@pytest.mark.parametrize("kind", range(O.NUM_KINDS), ids=O.KIND_NAMES)
def test_eval_batch_at_every_case(kind, E):
    cases = T.by_kind()[kind]
    items = []  # (record, x, scale exponent or None, case)
    for c in cases:
        if c.group == "scale":
            items.append((c.rec, c.x, 0, c))
            items += [T.scaled(c, k) + (k, c) for k in T.SCALE_EXPONENTS]
        else:
            items.append((c.rec, c.x, None, c))
    recs, pos = _distinct([it[0] for it in items])
    X = np.stack([it[1] for it in items])
    scale = [math.ldexp(1.0, it[2] or 0) for it in items]
    sysobj = E.System(O.stack(recs), T.N_VARS)
    r, J, deg = sysobj.eval_batch(X)
    want_r, want_J, want_deg, first = _oracle_eval(recs, X)
    err_r, err_J = _assert_close(kind, r, J, want_r, want_J, scale)
    assert np.array_equal(deg, want_deg), (O.KIND_NAMES[kind], np.nonzero(deg != want_deg)[0][:8].tolist())
    # the designated pair of every guard case: exactly zero where the table says the guard fires, not zero where it does not
    for b, (rec, x, k, c) in enumerate(items):
        if c.group != "guard":
            continue
        i = pos[b]
        rows = slice(first[i], first[i + 1])
        assert np.all(r[b, rows] == 0.0) if c.expect[0] else np.any(r[b, rows] != 0.0), (c.name, "residual", r[b, rows])
        zeroed = c.jac_rows if c.jac_rows is not None else (c.expect[1],) * (first[i + 1] - first[i])
        for kk, z in enumerate(zeroed):
            row = J[b, first[i] + kk]
            assert np.all(row == 0.0) if z else np.any(row != 0.0), (c.name, "jacobian row", kk, row)
    for k in (None,) + T.SCALE_EXPONENTS:
        sel = [b for b, it in enumerate(items) if (it[2] == k if k is not None else it[2] in (None, 0))]
        if sel:
            T.log(f"eval_batch  {O.KIND_NAMES[kind]:28s} scale {'1' if k is None else '2^%d' % k:6s} {len(recs)} records x {len(sel)} vectors: "
                  f"residual {np.max(err_r[sel]):.2e} of its bar, jacobian {np.max(err_J[sel]):.2e} of its bar")


def test_scale_property_on_the_device(E):
    """eval_batch(s x) against s eval_batch(x) for s = 2^k, |k| <= 200, on the generic pairs: within the bars wherever no guard
    changes state, and the number of entries that are bitwise equal (a libm whose hypot / atan2 were not scale-exact shows here)."""
    for kind in range(O.NUM_KINDS):
        cases = T.by_kind(("scale",))[kind]
        base_recs = []
        for i, c in enumerate(cases):
            base_recs.append(c.rec.copy())
            base_recs[-1]["weight"] = T.WEIGHTS[i % len(T.WEIGHTS)]
        X1 = np.stack([c.x for c in cases])
        sys1 = E.System(O.stack(base_recs), T.N_VARS)
        r1, J1, _ = sys1.eval_batch(X1)
        dims = [O.residual_dim(c) for c in base_recs]
        first = np.concatenate([[0], np.cumsum(dims)]).astype(int)
        for k in [k for k in T.SCALE_EXPONENTS if abs(k) <= 200]:
            s = math.ldexp(1.0, k)
            recs = []
            for c, b in zip(cases, base_recs):
                rec, _ = T.scaled(c, k)
                rec["weight"] = b["weight"]
                recs.append(rec)
            rs, Js, _ = E.System(O.stack(recs), T.N_VARS).eval_batch(X1 * s)
            bit_r = bit_j = n_r = n_j = 0
            for i, c in enumerate(cases):  # record i at its own vector
                if O.residual(recs[i], X1[i] * s)[1] or O.jacobian_rows(recs[i], X1[i] * s)[1]:
                    continue  # a guard changed state: test_eval_batch_at_every_case holds these to the oracle
                rows = slice(first[i], first[i + 1])
                a, b_ = rs[i, rows], s * r1[i, rows]
                assert np.all(np.abs(a - b_) <= 1e-11 * np.maximum(s, np.abs(b_))), (c.name, k, a, b_)
                assert np.all(np.abs(Js[i, rows] - J1[i, rows]) <= 1e-10 * np.maximum(1.0, np.abs(J1[i, rows]))), (c.name, k)
                bit_r += int(np.sum(a == b_))
                n_r += a.size
                bit_j += int(np.sum(Js[i, rows] == J1[i, rows]))
                n_j += Js[i, rows].size
            T.log(f"device scale  {O.KIND_NAMES[kind]:28s} 2^{k:<4d} bitwise: residual {bit_r} of {n_r}, jacobian {bit_j} of {n_j}")


# ---- System.measure on both placements against the host function ----------------------------------------------------------------
def _trace(E, call):
    trace = np.zeros(64, dtype=np.uint64)
    E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
    try:
        out = call()
    finally:
        k = E.lib().ezpz_debug_call_trace(None, 0)
    return out, [int(v) for v in trace[:k:2]]


@pytest.mark.parametrize("route,stamp", [("row", ROW), ("direct", DIRECT)])
def test_measure_at_the_guard_and_branch_cases(E, monkeypatch, route, stamp):
    monkeypatch.setenv("EZPZ_MEASURE_ROUTE", route)
    cases = [c for c in T.GUARD + T.BRANCH if E.constraint_has_param(c.rec)]
    assert len({c.kind for c in cases}) == 13
    recs, pos = _distinct([c.rec for c in cases])
    recs = O.stack(recs)
    X = np.stack([c.x for c in cases])
    hm, hg, hf = np.zeros((len(X), len(recs))), np.zeros((len(X), len(recs), 8)), np.zeros((len(X), len(recs)), np.uint8)
    for b in range(len(X)):
        for i in range(len(recs)):
            m, g, fl = E.constraint_measure(recs[i], X[b])
            hm[b, i], hg[b, i, : len(g)], hf[b, i] = m, g, fl
    s = E.System(O.stack([O.fixed(v, 0.0) for v in range(T.N_VARS)]), T.N_VARS)
    (m, grad, flags), stamps = _trace(E, lambda: s.measure(X, recs, want_grad=True, want_flags=True))
    assert stamp in stamps and LAUNCHED in stamps, stamps
    assert np.array_equal(flags, hf), np.argwhere(flags != hf)[:8].tolist()
    exact = np.isin(recs["kind"], M.NO_LIBM)
    assert m[:, exact].tobytes() == hm[:, exact].tobytes() and grad[:, exact].tobytes() == hg[:, exact].tobytes()
    with np.errstate(invalid="ignore"):
        same = (~np.isfinite(hm) & ~np.isfinite(m)) | (np.abs(m - hm) <= 1e-11 * np.maximum(1.0, np.abs(hm)))
        assert np.all(same), (np.argwhere(~same)[:8].tolist(), m[~same][:8], hm[~same][:8])
        bar = 1e-10 * np.maximum(1.0, np.nanmax(np.where(np.isfinite(hg), np.abs(hg), 0.0), axis=2, keepdims=True))
        same = (~np.isfinite(hg) & ~np.isfinite(grad)) | (np.abs(grad - hg) <= bar)
        assert np.all(same), (np.argwhere(~same)[:8].tolist(), grad[~same][:8], hg[~same][:8])
    # the designated pair of every guard case carries the flags the header documents
    for b, c in enumerate(cases):
        if c.group == "guard":
            grad_guard = c.expect[1] if c.kind in (O.DISTANCE, O.ARC_RADIUS) else False
            assert flags[b, pos[b]] == (1 if c.expect[0] else 0) | (2 if grad_guard else 0), c.name


# ---- the solve routes at the thresholds, without a step ------------------------------------------------------------------------------
def _finite_cases(kinds):
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for c in T.GUARD + T.BRANCH:
            if c.kind in kinds and c.finite:
                r, _ = O.residual(c.rec, c.x)
                rows, _ = O.jacobian_rows(c.rec, c.x)
                if np.all(np.isfinite(r)) and all(math.isfinite(pd) for row in rows for _, pd in row):
                    out.append(c)
    return out


def _assert_untouched(what, x, x0, st, mask, logs, wants):
    """One batch of solves with max_iterations = 0 against the oracle's outcomes `wants` (one per system)."""
    assert x.tobytes() == np.ascontiguousarray(x0).tobytes(), what
    for b, want in enumerate(wants):
        assert want.error == 0 and want.iterations == 0
        assert int(st["iterations"][b]) == 0, (what, b)
        assert bool(st["converged"][b]) == want.converged, (what, b)
        assert np.nonzero(mask[b])[0].tolist() == want.unsatisfied, (what, b, np.nonzero(mask[b])[0].tolist(), want.unsatisfied)
        assert int(st["n_unsatisfied"][b]) == len(want.unsatisfied), (what, b)
        # (the batch entries log the evaluators' Degenerate warnings; the lints of lib.rs on a record -- an angle of 0 or 180 degrees
        # should be Parallel -- belong to ezpz_solve: test_small_system_kernels_and_single_solves_without_a_step)
        degenerate = [w[0] for w in want.warnings if w[1] == O.WARN_DEGENERATE]
        assert int(st["n_warnings"][b]) == len(degenerate), (what, b, int(st["n_warnings"][b]), len(degenerate))
        if logs is not None:
            assert [p for _, p in logs[b]] == degenerate, (what, b)


def _run(E, what, sysobj, x0, wants):
    cfg = E.Config(**CFG0)
    x, st, mask = sysobj.solve_batch(x0, cfg, want_mask=True)
    xl, stl, logs = sysobj.solve_batch_logged(x0, cfg, warn_cap=1024)
    assert xl.tobytes() == x.tobytes()
    _assert_untouched(what, x, x0, st, mask, logs, wants)


KIND_GROUPS = ((O.LINE_TANGENT_TO_CIRCLE, O.CIRCLE_TANGENT_TO_CIRCLE, O.DISTANCE, O.DISTANCE_VAR, O.ARC_RADIUS, O.ARC, O.LINES_EQUAL_LENGTH),
               (O.LINES_AT_ANGLE, O.ARC_ANGLE, O.POINTS_AT_ANGLE),
               (O.POINT_LINE_DISTANCE, O.VERTICAL_POINT_LINE_DISTANCE, O.HORIZONTAL_POINT_LINE_DISTANCE, O.SYMMETRIC, O.POINT_ARC_COINCIDENT,
                O.ARC_LENGTH),
               (O.VERTICAL_DISTANCE, O.HORIZONTAL_DISTANCE, O.VERTICAL, O.HORIZONTAL, O.FIXED, O.SCALAR_EQUAL, O.POINTS_COINCIDENT,
                O.CIRCLE_RADIUS, O.MIDPOINT))


def test_the_kind_groups_cover_every_kind():
    assert sorted(k for g in KIND_GROUPS for k in g) == list(range(O.NUM_KINDS))


def _class_of(c):
    """What makes two one-record components one class of the component-resident shape (comp_program.cpp: find_classes), but the weight."""
    return (c.kind, int(c.rec["tag"]), tuple(int(v) for v in c.rec["ids"][: O.KIND_NUM_IDS[c.kind]]))


def _chunks(cases, classes_per_system):
    """The cases cut into systems of at most `classes_per_system` classes, classes in order of first appearance."""
    order = []
    for c in cases:
        if _class_of(c) not in order:
            order.append(_class_of(c))
    return [[c for c in cases if _class_of(c) in order[lo: lo + classes_per_system]] for lo in range(0, len(order), classes_per_system)]


FREE_VARIABLES = 128  # components of their own without a constraint: with them every system has the shape's 128 components


def block_system(cases):
    """One 8-variable component per case, then FREE_VARIABLES variables that no constraint names: (records, values).  The weight
    goes by class: the shape takes at most 32 classes, and the state of all of them has to fit the LDS (hence _chunks)."""
    recs, weight_of = [], {}
    for i, c in enumerate(cases):
        rec = c.rec.copy()
        n_ids = O.KIND_NUM_IDS[c.kind]
        rec["weight"] = weight_of.setdefault(_class_of(c), T.WEIGHTS[len(weight_of) % len(T.WEIGHTS)])
        rec["ids"][:n_ids] = rec["ids"][:n_ids] + T.N_VARS * i
        recs.append(rec)
    return O.stack(recs), np.concatenate([c.x for c in cases] + [np.full(FREE_VARIABLES, 0.25)])


def _oracle_block(recs, x, cases):
    want = O.solve(recs, x, O.Config(**CFG0), linsolve=O.LINSOLVE_SPARSE, warn_cap=1 << 16, inner=True)
    # one Degenerate warning per evaluator that fires, in constraint order: the table's expectation, not only the oracle's
    fired = [i for i, c in enumerate(cases) if c.group == "guard" for _ in range(int(c.expect[0]) + int(c.expect[1]))]
    guard_positions = {i for i, c in enumerate(cases) if c.group == "guard"}
    assert sorted(w[0] for w in want.warnings if w[0] in guard_positions) == fired
    assert want.iterations == 0 and want.error == 0 and want.final_values.tobytes() == x.tobytes()
    return want


@pytest.mark.parametrize("group", range(len(KIND_GROUPS)))
def test_block_system_routes_without_a_step(E, group):
    """One 8-variable component per finite guard and branch case of the group's kinds, four classes to a system, max_iterations = 0,
    on the component interpreter and the list-walk teams: values untouched bit for bit, 0 iterations, the oracle's `converged`,
    unsatisfied mask and warnings (2 / 1 / 0 for HorizontalPointLineDistance below / at / above its threshold)."""
    for cases in _chunks(_finite_cases(KIND_GROUPS[group]), 4):
        recs, x = block_system(cases)
        n = len(x)
        x0 = np.stack([x, x])
        want = _oracle_block(recs, x, cases)
        wants = [want, want]
        comp = E.System(recs, n)
        assert comp.info()["team_mode"] == 3, comp.info()
        _run(E, "component interpreter", comp, x0, wants)
        walk = E.System(recs, n, team_size=E.TEAM_AUTO_LISTS)
        assert walk.info()["team_mode"] in (0, 1, 2), walk.info()
        _run(E, "list-walk teams", walk, x0, wants)


def chained_system(cases):
    """The cases' 8-variable groups as ONE connected sketch: the case records first (positions = case numbers), then a ScalarEqual
    between every two neighbouring variables.  The links are linear and have no guard; with max_iterations = 0 they only add rows.
    A connected system of more than 20 variables is what the lanes-across-the-batch plan takes (shape.cpp): no component plan, no
    lane plan."""
    recs, x = block_system(cases)
    n = T.N_VARS * len(cases)
    links = [O.scalar_equal(v, v + 1) for v in range(n - 1)]
    return O.stack(list(recs) + links), x[:n]


@pytest.mark.parametrize("group", range(len(KIND_GROUPS)))
def test_lanes_across_the_batch_without_a_step(E, group):
    """The finite guard and branch cases of the group's kinds chained into one connected sketch, on the lanes-across-the-batch
    kernel (batch_kernel.hip.hpp; TEAM_BATCH_LANES takes it from a batch of one system).  info() shows every condition under which
    shape.cpp builds the plan: not component-resident, not a small system's lane kernel, one partition, one workgroup, no frontal
    plan that serves every call -- so a quiet fall to another route would show."""
    cases = _finite_cases(KIND_GROUPS[group])
    recs, x = chained_system(cases)
    n = len(x)
    assert n > 20
    want = _oracle_block(recs, x, cases)
    lanes = E.System(recs, n, team_size=E.TEAM_BATCH_LANES)
    info = lanes.info()
    assert info["team_mode"] in (2, 4) and info["n_components"] == 1 and info["n_partitions"] == 1 and info["grid_workgroups"] == 1 \
        and info["front_max_batch"] != 0xFFFFFFFF, info
    assert E.specialized_source(recs, n) == ""  # neither a component plan nor a lane plan
    _run(E, "lanes across the batch", lanes, np.stack([x, x, x]), [want, want, want])


# the guard cases, every site's record a class of its own, two classes to a compiled kernel; the linear kinds (no guard: their branch
# cases) six classes to a kernel
COMPILED = [ch for g in KIND_GROUPS[:3] for ch in _chunks([c for c in _finite_cases(g) if c.group == "guard"], 2)] + \
    _chunks(_finite_cases(KIND_GROUPS[3]), 6)


@pytest.mark.parametrize("cases", COMPILED, ids=["%d:" % i + "+".join(sorted({O.KIND_NAMES[c.kind] for c in ch})) for i, ch in enumerate(COMPILED)])
def test_compiled_component_kernel_without_a_step(E, cases):
    """The run-time compiled component kernel on the guard cases -- every site's record, two classes to a kernel -- and on the
    branch cases of the nine linear kinds (they have no guard).  A kernel for the whole table of a group would take above ten
    seconds of run-time compilation; the interpreter and the list walk run the whole table above, the lanes across the batch and the
    compiled kernels of a small system run it below."""
    recs, x = block_system(cases)
    x0 = np.stack([x, x])
    want = _oracle_block(recs, x, cases)
    comp = E.System(recs, len(x))
    assert comp.info()["team_mode"] == 3, comp.info()
    assert comp.specialize(wait=True) == 2
    _run(E, "compiled component kernel", comp, x0, [want, want])


@pytest.mark.parametrize("kind", range(O.NUM_KINDS), ids=O.KIND_NAMES)
def test_small_system_kernels_and_single_solves_without_a_step(E, kind):
    """Per kind: the run-time compiled kernels of a small system -- one lane per system and one wavefront per system, both for every
    system -- on all distinct records of the kind's finite guard and branch cases, 6 records to a system, the batch being the case
    vectors; and every case alone through one ezpz_solve call."""
    cases = _finite_cases((kind,))
    cfg = E.Config(**CFG0)
    # one ezpz_solve per case
    for c in cases:
        got = E.solve_records(O.stack([c.rec]), c.x, cfg, warn_cap=64)
        want = O.solve(O.stack([c.rec]), c.x, O.Config(**CFG0), warn_cap=64)
        assert got.error == 0 and want.error == 0, c.name
        assert got.final_values.tobytes() == c.x.tobytes(), c.name
        assert (got.iterations, got.converged, got.unsatisfied, got.warnings) == (0, want.converged, want.unsatisfied, want.warnings), \
            (c.name, got.warnings, want.warnings)
        if c.group == "guard":
            assert len([w for w in got.warnings if w[1] == O.WARN_DEGENERATE]) == int(c.expect[0]) + int(c.expect[1]), c.name
    # lane and wavefront kernels
    recs, _ = _distinct([c.rec for c in cases])
    X = np.stack([c.x for c in cases])
    for lo in range(0, len(recs), 6):
        chunk = O.stack(recs[lo: lo + 6])
        wants = [O.solve(chunk, X[b], O.Config(**CFG0), warn_cap=1 << 12, inner=True) for b in range(len(X))]
        for form, team, entry in (("lane", 0, "ezpz_jit_lane"), ("wave", E.TEAM_LATENCY_WAVE, "ezpz_jit_wave")):
            assert entry in E.specialized_source(chunk, T.N_VARS, wave=(form == "wave")), (O.KIND_NAMES[kind], form, lo)
            sysobj = E.System(chunk, T.N_VARS, team_size=team)
            assert sysobj.specialize(wait=True) == 2, (O.KIND_NAMES[kind], form, lo)
            _run(E, (O.KIND_NAMES[kind], form, lo), sysobj, X, wants)
