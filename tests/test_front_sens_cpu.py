"""Dimension sensitivities on the FRONTAL shape, what a machine without a GPU can check: the surface of
ezpz_system_set_sensitivity_route; the host tables of csrc/front_sens_plan.cpp -- the rhs-only assembly streams, the rhs-only
extend-add, the homes of the listed constraints -- executed in numpy (tests/front_sens_ref.py) against the dense
-(JtJ + lam I)^-1 Jt g_j of tests/sensitivity_ref.py; and the condition on the inputs of tests/test_gpu_front_sens.py: the
reference's own spread on every system that file uses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import front_sens_ref as FS
import sensitivity_ref as R
from sensitivity import BAR_CEILING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface():
    import ezpz_amd as E
    from ezpz_amd import _lib

    header = open(os.path.join(ROOT, "include", "ezpz_amd.h")).read()
    assert re.search(r"#define\s+EZPZ_SENSITIVITY_ROUTE_DEFAULT\s+0u", header)
    assert re.search(r"#define\s+EZPZ_SENSITIVITY_ROUTE_FRONTS\s+1u", header)
    assert re.search(r"int\s+ezpz_system_set_sensitivity_route\(EzpzSystem\*\s*sys,\s*uint32_t\s+route\);", header)
    assert "ezpz_system_set_sensitivity_route" in _lib.EXPORTS and "ezpz_debug_front_sens_tables" in _lib.EXPORTS
    L = E.lib()
    assert L.ezpz_system_set_sensitivity_route(None, 1) == -103
    assert L.ezpz_system_set_sensitivity_route(None, 0) == -103
    assert callable(E.System.set_sensitivity_route)
    assert _lib.SENSITIVITY_ROUTES == {"default": 0, "fronts": 1}
    fields = [f for f, _ in _lib.CSensitivityPlan._fields_]
    assert fields[-5:] == ["route", "front_workgroups", "rhs_per_item", "items_per_system", "front_lds_bytes"]
    assert C.sizeof(_lib.CSensitivityPlan) == 64


def _half_permuted(pos):
    return np.random.default_rng(4).permutation(pos)[: max(1, len(pos) // 2)]


def _tables_case(name, wgs):
    s = FS.system(name)
    b = 0
    recs = R.substituted(s["recs"], s["pos"], s["params"][b])
    Sref, spread = FS.references(name)[b]
    S, bad = FS.executed(recs, s["n_vars"], wgs, s["pos"], s["x"][b], s["lam"])
    assert not bad
    scale = np.maximum(1.0, np.abs(Sref).max(axis=1))[:, None]
    err = float((np.abs(S - Sref) / scale).max())
    print(name, wgs, "error", err, "bar", R.bar(spread))
    assert err <= R.bar(spread), (name, wgs, err, R.bar(spread))
    half = _half_permuted(s["pos"])
    Sh, bad = FS.executed(recs, s["n_vars"], wgs, half, s["x"][b], s["lam"])
    assert not bad
    where = {int(p): j for j, p in enumerate(s["pos"])}
    assert np.array_equal(Sh, S[[where[int(p)] for p in half]])


@pytest.mark.parametrize("wgs", [1, 2, 4])
@pytest.mark.parametrize("name", ["sketch25", "sketch75", "band", "hub"])
def test_tables_executed_in_numpy(name, wgs):
    """Factorisation with a zero right-hand side, then per listed position the rhs-only pass through the tables: S against the
    dense solve from the oracle's rows, at the bar the reference's own spread grants; the full list and a permuted half list give
    the same rows bit for bit (a row does not depend on the rest of the list)."""
    _tables_case(name, wgs)


@pytest.mark.parametrize("name,wgs", [("mixed40", 1), ("mixed40", 3), ("mixed40+corner", 1), ("mixed40+corner", 3), ("linear100", 1),
                                      ("linear100:weighted", 3)])
def test_tables_executed_in_numpy_all_kinds_guards_linear(name, wgs):
    """The same on the systems with two-row listed constraints, angle kinds, weights, guards that fire and linear kinds only
    (test_inputs_are_what_they_claim): the host tables are not what the GPU test of these systems finds wrong.  (Measured errors:
    mixed40 3.1e-10 on 1 workgroup and on 3, bar 7.9e-9; with the corner 3.3e-10 on both, bar 8.1e-9; linear100 4.1e-13, weighted on 3
    workgroups 4.4e-13, bar 1e-10.)"""
    _tables_case(name, wgs)


def _wide_positions(name, wgs):
    """The positions the executor runs on a wide input: every listed constraint of tree60 and tree108; of tree144 and comb213
    (0.05 s per right-hand side) FS.sixteen and every listed constraint on a pivot variable of the plan's widest front: the
    right-hand sides that enter the elimination there or below it."""
    import front_ref as F
    from oracle import oracle as O

    s = FS.system(name)
    if name in ("tree60", "tree108"):
        return s["pos"]
    plan = F.Plan(s["recs"], s["n_vars"], wgs)
    widest = set()
    for g in range(plan.n_wgs):
        descs, _, _, rows, _, _ = plan.wg_tables(g)
        vg = plan.arr("<u4", plan.wgs[g]["o_var_glob"], int(plan.wgs[g]["n_loc"]))
        for d in descs:
            if int(d["S"]) == plan.max_rows:
                widest |= set(int(vg[int(r)]) for r in rows[int(d["rows"]): int(d["rows"]) + int(d["K"])])
    at_home = [int(p) for p in s["pos"]
               if set(int(v) for v in s["recs"]["ids"][int(p)][: O.KIND_NUM_IDS[int(s["recs"]["kind"][int(p)])]]) & widest]
    assert at_home, name
    return np.unique(np.concatenate([FS.sixteen(s["pos"]), np.asarray(at_home, dtype=np.uint32)])).astype(np.uint32)


@pytest.mark.parametrize("name,wgs", [(n, w) for n in FS.WIDE for w in FS.WIDE_WGS[n]])
def test_tables_executed_in_numpy_wide_fronts(name, wgs):
    """The same on the wide inputs (test_wide_inputs_are_what_they_claim): fronts of up to 63 rows, remote children of up to 56
    rows arriving as chunks, minimum-degree plans -- the host tables are not what the GPU test of these systems finds wrong.
    tree144 and comb213 on the positions of _wide_positions (38 and 40 of them).  (Measured errors: tree60 4.9e-13 on 1 and on 2
    workgroups, 5.3e-13 on 4, bar 1e-10; tree108 1.4e-9 on 1, 2 and 4, bar 1.1e-8; tree144 2.5e-11, bar 8.3e-10; comb213 7.7e-8,
    bar 2.5e-6.)  A permuted part of the list gives the same rows bit for bit."""
    s = FS.system(name)
    pos = _wide_positions(name, wgs)
    where = {int(p): j for j, p in enumerate(s["pos"])}
    rows = [where[int(p)] for p in pos]
    recs = R.substituted(s["recs"], s["pos"], s["params"][0])
    Sref, spread = FS.references(name)[0]
    S, bad = FS.executed(recs, s["n_vars"], wgs, pos, s["x"][0], s["lam"])
    assert not bad
    scale = np.maximum(1.0, np.abs(Sref[rows]).max(axis=1))[:, None]
    err = float((np.abs(S - Sref[rows]) / scale).max())
    print(name, wgs, len(pos), "positions, error", err, "bar", R.bar(spread))
    assert err <= R.bar(spread), (name, wgs, err, R.bar(spread))
    half = _half_permuted(pos)[:24]
    Sh, bad = FS.executed(recs, s["n_vars"], wgs, half, s["x"][0], s["lam"])
    back = {int(p): j for j, p in enumerate(pos)}
    assert not bad and np.array_equal(Sh, S[[back[int(p)] for p in half]])


# name -> per workgroup count (max_rows, ordering, remote children, the least the largest remote FrontChild.rows may be)
WIDE_PLANS = {"tree60": {1: (58, 0, 0, 0), 2: (58, 0, 11, 52), 4: (58, 0, 18, 23)},
              "tree108": {1: (36, 1, 0, 0), 2: (36, 1, 6, 30), 4: (36, 1, 21, 22)},
              "tree144": {4: (59, 1, 15, 34)},
              "comb213": {4: (63, 0, 14, 56)}}


def test_wide_inputs_are_what_they_claim():
    """The shapes the GPU tests of tree60, tree108, tree144 and comb213 rest on, from the plan blob: the widest front (63 rows in
    comb213: lane 63 holds the right-hand side's row), the ordering (1: minimum degree), the workgroups, the largest update matrix
    of a child in another workgroup (FrontChild.rows counts its right-hand side's row: more than 50 rows arrive as chunks), every
    K from 1 to 8, one component below the default route's limit, listed constraints at home off workgroup 0.  A planner that
    loses one of them fails here; the GPU test must not thin out unnoticed."""
    import front_ref as F

    assert set(WIDE_PLANS) == set(FS.WIDE) and all(tuple(WIDE_PLANS[n]) == FS.WIDE_WGS[n] for n in FS.WIDE)
    for name, (family, npts, seed) in FS.WIDE.items():
        recs, g = FS.inputs(name)
        n = len(g)
        pos = FS.driven(recs)
        assert n == 2 * npts <= 1024 and len(pos) == len(recs) == n, name
        for wgs in (1, 2, 4):
            plan = F.Plan(recs, n, wgs)
            if wgs not in WIDE_PLANS[name]:
                assert not plan.ok, (name, wgs)  # the share of a workgroup does not fit the LDS
                continue
            max_rows, ordering, n_remote, largest = WIDE_PLANS[name][wgs]
            assert plan.ok and plan.n_wgs == wgs and plan.n_components == 1, (name, wgs)
            assert (plan.max_rows, plan.ordering) == (max_rows, ordering), (name, wgs, plan.max_rows, plan.ordering)
            S, K, remote = [], set(), []
            for gi in range(plan.n_wgs):
                descs, _, children, _, _, _ = plan.wg_tables(gi)
                S += [int(d["S"]) for d in descs]
                K |= set(int(d["K"]) for d in descs)
                remote += [int(c["rows"]) for c in children if int(c["flags"]) & F.FRONT_CHILD_REMOTE]
            assert max(S) == max_rows and K == set(range(1, 9)), (name, wgs, max(S), sorted(K))
            assert len(remote) == n_remote and max(remote, default=0) >= largest, (name, wgs, len(remote), max(remote, default=0))
            if wgs > 1:
                T = FS.Tables(recs, n, wgs, pos)
                homes = set(T.home(j)[0] for j in range(len(pos)))
                assert homes - {0} and homes <= set(range(wgs)), (name, wgs, homes)
    assert WIDE_PLANS["comb213"][4][0] == 63 and WIDE_PLANS["tree60"][2][3] > 50 and WIDE_PLANS["comb213"][4][3] > 50
    for name in FS.WIDE:
        s = FS.system(name)
        for b in range(len(s["x"])):
            assert R.degenerate_count(s["recs"], s["x"][b], s["pos"], s["params"][b]) == 0, (name, b)


def test_inputs_are_what_they_claim():
    """The properties the GPU tests of mixed40, mixed40+corner and linear100 rest on: a test that passes on inputs that lost them
    would prove nothing."""
    import front_ref as F
    from oracle import oracle as O

    s = FS.system("mixed40")
    recs, pos = s["recs"], s["pos"]
    listed = recs[pos]
    assert len(pos) == len(recs) and all(R.has_param(r) for r in recs)
    kinds = set(int(k) for k in listed["kind"])
    assert kinds == {O.DISTANCE, O.VERTICAL_DISTANCE, O.HORIZONTAL_DISTANCE, O.FIXED, O.CIRCLE_RADIUS, O.ARC_RADIUS, O.POINT_LINE_DISTANCE,
                     O.VERTICAL_POINT_LINE_DISTANCE, O.HORIZONTAL_POINT_LINE_DISTANCE, O.ARC_LENGTH, O.LINES_AT_ANGLE, O.ARC_ANGLE,
                     O.POINTS_AT_ANGLE}
    for k in (O.LINES_AT_ANGLE, O.ARC_ANGLE, O.POINTS_AT_ANGLE):  # both angle units of every angle kind
        assert set(int(t) for t in listed["tag"][listed["kind"] == k]) == {O.ANGLE_OTHER_DEG, O.ANGLE_OTHER_RAD}, k
    two = FS.two_row(recs, pos)
    assert set(int(recs["kind"][pos[j]]) for j in two) == {O.ARC_RADIUS, O.ARC_LENGTH, O.POINTS_AT_ANGLE}
    for wgs in (1, 3):
        assert F.Plan(recs, s["n_vars"], wgs).n_wgs == wgs
    T = FS.Tables(recs, s["n_vars"], 3, pos)
    assert any(T.home(j)[0] != 0 for j in two)
    assert np.any(recs["weight"] != 1.0) and np.all(FS.system("mixed40:unit")["recs"]["weight"] == 1.0)
    assert np.all(FS.system("mixed40:double")["recs"]["weight"] == 2.0) and FS.system("mixed40:double")["lam"] == 4.0 * s["lam"]
    assert np.array_equal(FS.system("mixed40:double")["x"], FS.system("mixed40:unit")["x"])
    for b in range(len(s["x"])):
        assert R.degenerate_count(recs, s["x"][b], pos, s["params"][b]) == 0
    c = FS.system("mixed40+corner")
    assert len(c["pos"]) == len(pos) + 3 and np.array_equal(c["pos"][:-3], pos) and c["n_vars"] == s["n_vars"] + 8
    assert [int(k) for k in c["recs"]["kind"][c["pos"][-3:]]] == [O.VERTICAL_POINT_LINE_DISTANCE, O.LINES_AT_ANGLE, O.ARC_LENGTH]
    for b in range(len(c["x"])):
        assert R.degenerate_count(c["recs"], c["x"][b], c["pos"], c["params"][b]) == 3
    for name in ("linear100", "linear100:weighted"):
        lin = FS.system(name)
        assert all(int(k) in FS.LINEAR_KINDS for k in lin["recs"]["kind"]) and len(lin["pos"]) == len(lin["recs"]) == 200
        assert [F.Plan(lin["recs"], lin["n_vars"], wgs).n_wgs for wgs in (1, 3)] == [1, 3]
        assert np.all(lin["recs"]["weight"] == 1.0) == (name == "linear100")


def test_tables_hold_rhs_entries_only():
    """Every entry of the rhs-only assembly stream is a FASM_RHS entry of the plan's assembly stream, each exactly once."""
    import front_ref as F

    s = FS.system("sketch75")
    for wgs in (1, 3):
        plan = F.Plan(s["recs"], s["n_vars"], wgs)
        T = FS.Tables(s["recs"], s["n_vars"], wgs, s["pos"])
        for g in range(plan.n_wgs):
            W = plan.wgs[g]
            t_end = int(W["t_cons"]) if int(W["t_cons"]) != 0xFFFFFFFF else int(W["tab_bytes"])
            stream = plan.arr("<u4", int(W["o_tables"]) + int(W["t_stream"]), (t_end - int(W["t_stream"])) // 4)
            want = []
            for tr in range(int(W["asm_trips"])):
                base = int(stream[int(W["asm_word0"]) + tr])
                wdt = int(stream[base]) >> 24
                for l in range(64):
                    hdr = int(stream[base + l])
                    if hdr & F.FASM_RHS and not hdr & F.FASM_NOP:
                        want.append((hdr, tuple(int(stream[base + 64 * (1 + q) + l]) for q in range(wdt))))
            w_asm_offs, asm_trips, _, _ = T.wg(g)
            got = []
            for tr in range(asm_trips):
                base = int(T.w[w_asm_offs + tr])
                wdt = int(T.w[base]) >> 24
                for l in range(64):
                    hdr = int(T.w[base + l])
                    if not hdr & F.FASM_NOP:
                        got.append((hdr, tuple(int(T.w[base + 64 * (1 + q) + l]) for q in range(wdt))))
            assert sorted(got) == sorted(want) and len(want) > 0


NEW_INPUTS = ["mixed40", "mixed40:unit", "mixed40:double", "mixed40+corner", "linear100", "linear100:weighted"]
SMALL_INPUTS = R.kind_names() + ["weighted", "under"]  # tests/sensitivity_ref.py's own systems, on the fronts in the GPU test


@pytest.mark.parametrize("name", ["sketch25", "sketch75", "sketch150", "band", "hub"] + NEW_INPUTS + list(FS.WIDE) + SMALL_INPUTS)
def test_reference_spread_on_the_gpu_inputs(name):
    """The numpy reference's Cholesky-against-lstsq spread on the systems tests/test_gpu_front_sens.py checks: at most 5e-6, so no
    granted bar exceeds BAR_CEILING.  (Measured, 2 systems each: sketch25 1.4e-12, sketch75 2.9e-10, sketch150 8.7e-8, band 3.9e-9,
    hub 6.1e-8, sketch600 5.6e-8; mixed40 4.0e-10, mixed40:unit 2.7e-10, mixed40:double 2.7e-10, mixed40+corner 4.0e-10, linear100
    6.0e-13, linear100:weighted 5.2e-13; tree60 4.9e-13, tree108 3.2e-9, tree144 1.2e-10, comb213 1.3e-7; the 16 small systems 1.2e-10 at most (points_at_angle_rad) -- it depends on the linear
    algebra library in its last digits, so the numbers are not asserted.)"""
    refs = R.references(name) if name in SMALL_INPUTS else FS.references(name)
    for b, (_, spread) in enumerate(refs):
        print(name, b, "spread", spread)
        assert spread <= 5e-6 and R.bar(spread) <= BAR_CEILING


def test_reference_spread_above_the_limit():
    """sketch600 with its 16 listed positions (1200 variables in one component)."""
    for b, (_, spread) in enumerate(FS.references("sketch600", 2, FS.sixteen)):
        print("sketch600", b, "spread", spread)
        assert spread <= 5e-6 and R.bar(spread) <= BAR_CEILING
