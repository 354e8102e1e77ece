"""Reference dimensions, what can be checked without a device: the symbols and their signatures, ezpz_constraint_measure against
the ORACLE for every parametrised kind and tag -- its residual vanishes (or is smallest) at param := m, its Jacobian rows are
the gradient of the subtracting kinds -- the gradient of the curved kinds against central differences of the numpy definition
(tests/measure_ref.py), the ranges at the branch cuts, and the flags on degenerate configurations.

Bars.  Value: the oracle's residual at param := m at most 1e-11 * max(1, |x|inf), the project's residual parity bar.  Gradient of
the nine subtracting kinds: 1e-10 * max(1, |row|inf), the project's Jacobian bar.  Gradient of ArcLength and the angle kinds:
central differences at h = 2^-10 and h / 2 differ by three times the error of the finer one, so 4 x their difference + 1e-11 *
max(1, |d2|), the rule of tests/test_sensitivity_cpu.py."""
import ctypes as C
import math
import os
import re

import numpy as np

import ezpz_amd as E
import measure_ref as M
import sensitivity_ref as R
from ezpz_amd._lib import EXPORTS
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_ROW = tuple(k for k in M.SUBTRACTING + M.CURVED if k not in (O.ARC_RADIUS, O.ARC_LENGTH, O.POINTS_AT_ANGLE))

SIGNATURES = {
    "ezpz_constraint_measure": ["c", "x", "m_out", "grad_out[8]", "flags"],
    "ezpz_system_measure": ["sys", "records", "n_meas", "x", "batch", "m_out", "flags_out", "grad_out"],
    "ezpz_system_measure_device": ["sys", "records", "n_meas", "x_dev", "batch", "m_out_dev", "flags_out_dev", "grad_out_dev", "stream"],
    "ezpz_system_measure_response": ["sys", "records", "n_meas", "x", "S", "n_param", "batch", "tol", "D_out", "worst_out", "rss_out"],
    "ezpz_system_measure_response_device": ["sys", "records", "n_meas", "x_dev", "S_dev", "n_param", "batch", "tol_dev", "D_out_dev",
                                            "worst_out_dev", "rss_out_dev", "stream"],
    "ezpz_system_measure_vjp": ["sys", "records", "n_meas", "x", "grad_m", "batch", "grad_x_out"],
    "ezpz_system_measure_vjp_device": ["sys", "records", "n_meas", "x_dev", "grad_m_dev", "batch", "grad_x_out_dev", "stream"],
}


def test_symbols_are_exported_with_the_documented_signatures():
    L = E.lib()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ezpz_amd.h")).read())
    for name, params in SIGNATURES.items():
        assert name in EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(params), name
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl, name
        assert [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")] == params, name
    for method in ("measure", "measure_response", "measure_vjp", "measure_device", "measure_response_device", "measure_vjp_device"):
        assert callable(getattr(E.System, method))
    assert callable(E.constraint_measure)
    assert L.ezpz_constraint_measure(None, None, None, None, None) == 0
    assert "def measure(" in open(os.path.join(ROOT, "ezpz_amd", "torch_ops.py")).read()
    assert "torch" not in open(os.path.join(ROOT, "ezpz_amd", "__init__.py")).read()


def _points(rng):
    return rng.uniform(0.5, 3.0, 8) * rng.choice([-1.0, 1.0], 8) + np.arange(8) * 0.37


def _draws():
    """(record, x) for every kind x tag x three draws, the generator of tests/test_sensitivity_cpu.py."""
    for kind in range(O.NUM_KINDS):
        for tag in range(4):
            rng = np.random.default_rng(100 * kind + tag)
            ids = list(rng.permutation(8)[: O.KIND_NUM_IDS[kind]])
            for _ in range(3):
                x = _points(rng)
                yield O.stack([O._mk(kind, ids, float(rng.uniform(0.3, 1.4)), tag=tag)])[0], x


def _with_param(rec, m):
    r = rec.copy()
    r["param"] = m
    return r


def _sum_sq(rec, x, m):
    r, deg = O.residual(_with_param(rec, m), x)
    assert not deg
    return float(np.sum(np.square(r)))


def test_the_oracles_residual_vanishes_at_the_measured_value():
    checked, widest = 0, {}
    for rec, x in _draws():
        kind = int(rec["kind"])
        m, grad, flags = E.constraint_measure(rec, x)
        if not E.constraint_has_param(rec):
            assert not M.measurable(rec) and len(grad) == 0 and m == 0.0 and flags == 0
            continue
        assert M.measurable(rec) and len(grad) == O.KIND_NUM_IDS[kind] and flags == 0
        want, wflags = M.measure_ref(rec, x)
        assert wflags == 0 and abs(m - want) <= 1e-11 * max(1.0, abs(want)), (O.KIND_NAMES[kind], m, want)
        if kind in ONE_ROW or kind == O.POINTS_AT_ANGLE:
            r, deg = O.residual(_with_param(rec, m), x)
            bar = 1e-11 * max(1.0, float(np.abs(x).max()))
            err = float(np.abs(r).max())
            assert not deg and err <= bar, (O.KIND_NAMES[kind], int(rec["tag"]), r, bar)
            key = O.KIND_NAMES[kind]
            widest[key] = max(widest.get(key, 0.0), err)
        else:
            at = _sum_sq(rec, x, m)
            assert at <= _sum_sq(rec, x, m + 1e-4) and at <= _sum_sq(rec, x, m - 1e-4), O.KIND_NAMES[kind]
        if kind == O.ARC_RADIUS:
            X = x[rec["ids"][:6]]
            mean = (np.hypot(X[0] - X[2], X[1] - X[3]) + np.hypot(X[0] - X[4], X[1] - X[5])) / 2.0
            assert m == mean  # (numpy's hypot is libm's, the host function's: the same bits)
        checked += 1
    assert checked == (10 * 4 + 3 * 2) * 3
    for name, err in sorted(widest.items()):
        R.log(f"measure, {name}: the oracle's residual at param := m at most {err:.3e}")


def _oracle_rows(rec, x):
    """The oracle's unweighted Jacobian rows by slot of the record's ids (its ids are distinct here)."""
    rows, deg = O.jacobian_rows(rec, x)
    n_ids = O.KIND_NUM_IDS[int(rec["kind"])]
    slot_of = {int(v): s for s, v in enumerate(rec["ids"][:n_ids])}
    out = np.zeros((len(rows), n_ids))
    for k, row in enumerate(rows):
        for vid, pd in row:
            out[k, slot_of[int(vid)]] += pd
    return out, deg


def test_gradient_of_the_subtracting_kinds_is_the_oracles_jacobian():
    checked = 0
    for rec, x in _draws():
        kind = int(rec["kind"])
        if kind not in M.SUBTRACTING:
            continue
        m, grad, flags = E.constraint_measure(rec, x)
        rows, deg = _oracle_rows(_with_param(rec, m), x)
        assert not deg and flags == 0
        want = rows.mean(axis=0) if kind == O.ARC_RADIUS else rows[0]
        bar = 1e-10 * max(1.0, float(np.abs(want).max()))
        assert np.all(np.abs(grad - want) <= bar), (O.KIND_NAMES[kind], grad, want)
        checked += 1
    assert checked == 9 * 4 * 3


def test_gradient_of_the_curved_kinds_against_central_differences():
    checked, widest = 0, {}
    for rec, x in _draws():
        kind = int(rec["kind"])
        if kind not in M.CURVED or not M.measurable(rec):
            continue
        _, grad, flags = E.constraint_measure(rec, x)
        d1, d2 = M.central_grad(rec, x, R.H), M.central_grad(rec, x, R.H / 2)
        bar = 4.0 * np.abs(d2 - d1) + 1e-11 * np.maximum(1.0, np.abs(d2))
        err = np.abs(grad - d2)
        assert flags == 0 and np.all(err <= bar), (O.KIND_NAMES[kind], int(rec["tag"]), grad, d2, bar)
        key = (O.KIND_NAMES[kind], int(rec["tag"]))
        widest[key] = max(widest.get(key, (0.0, 0.0)), (float(bar.max()), float(err.max())))
        checked += 1
    assert checked == (4 + 3 * 2) * 3
    for (name, tag), (bar, err) in sorted(widest.items()):
        R.log(f"d measure / d x, {name} tag {tag}: widest bar granted {bar:.3e}, largest error {err:.3e}")


def test_ranges_at_the_branch_cuts():
    # centre / first point at the origin; arms at +90, -90 and exactly 180 degrees
    for end, want in (((0.0, 2.0), math.pi / 2), ((0.0, -2.0), -math.pi / 2), ((-3.0, 0.0), math.pi), ((-3.0, -0.0), math.pi)):
        x = np.asarray([0.0, 0.0, 1.5, 0.0, end[0], end[1], 0.0, 0.0])
        for tag, unit in (("rad", 1.0), ("deg", 180.0 / math.pi)):
            for rec in (O.arc_angle((0, 1), (2, 3), (4, 5), (tag, 0.0)), O.points_at_angle((0, 1), (2, 3), (4, 5), (tag, 0.0)),
                        O.lines_at_angle((0, 1), (2, 3), (6, 7), (4, 5), (tag, 0.0))):
                m, _, flags = E.constraint_measure(O.stack([rec])[0], x)
                # (exactly: atan2 of an argument on an axis is the correctly rounded multiple of pi / 2, then one product)
                assert flags == 0 and m == want * unit == M.measure_ref(O.stack([rec])[0], x)[0], (end, tag, m)
    # (arms that point away from each other in a direction whose cross product rounds to -0.0 still give +pi)
    x = np.asarray([0.0, 0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    assert E.constraint_measure(O.stack([O.arc_angle((0, 1), (2, 3), (4, 5), ("deg", 0.0))])[0], x)[0] == 180.0
    # an arc whose end equals its start is 0 long; three quarters of a turn, counter-clockwise from start to end
    r = 2.5
    arc = lambda: O.stack([O.arc_length((0, 1), (2, 3), (4, 5), 1.0)])[0]
    assert E.constraint_measure(arc(), np.asarray([1.0, 1.0, 1.0 + r, 1.0, 1.0 + r, 1.0]))[0] == 0.0
    m = E.constraint_measure(arc(), np.asarray([1.0, 1.0, 1.0 + r, 1.0, 1.0, 1.0 - r]))[0]
    assert m == r * (-math.pi / 2 + 2.0 * math.pi)  # (rem_euclid's sum and one product: exact operations on exact inputs)
    m = E.constraint_measure(arc(), np.asarray([1.0, 1.0, 1.0 + r, 1.0, 1.0, 1.0 + r]))[0]
    assert m == r * (math.pi / 2)


def test_flags_on_degenerate_configurations():
    x = np.asarray([1.0, 1.0, 1.0, 1.0, 2.0, 3.0, 0.5, 0.25])  # points 0 and 1 coincide
    for rec in (O.lines_at_angle((0, 1), (2, 3), (4, 5), (6, 7), ("rad", 0.4), weight=2.0), O.arc_length((0, 1), (2, 3), (4, 5), 1.5),
                O.points_at_angle((0, 1), (2, 3), (4, 5), ("deg", 20.0)), O.arc_angle((0, 1), (2, 3), (4, 5), ("deg", 20.0)),
                O.point_line_distance((4, 5), (0, 1), (2, 3), 1.0), O.vertical_point_line_distance((4, 5), (0, 1), (2, 3), 1.0)):
        rec = O.stack([rec])[0]
        assert O.residual(rec, x)[1]  # the oracle's residual calls it degenerate
        m, grad, flags = E.constraint_measure(rec, x)
        assert flags == 1 and m == 0.0 and np.all(grad == 0.0) and not np.any(np.signbit(grad))
        assert M.measure_ref(rec, x) == (0.0, 1)
    # the same records where the oracle does not call them degenerate: no flag
    y = np.asarray([1.0, 1.0, 2.0, 1.5, 2.0, 3.0, 0.5, 0.25])
    for rec in (O.arc_length((0, 1), (2, 3), (4, 5), 1.5), O.point_line_distance((4, 5), (0, 1), (2, 3), 1.0)):
        rec = O.stack([rec])[0]
        assert not O.residual(rec, y)[1] and E.constraint_measure(rec, y)[2] == 0
    # Distance at coincident points: the value is valid, the gradient guarded (the Jacobian's guard, not the residual's)
    dist = O.stack([O.distance((0, 1), (2, 3), 1.0)])[0]
    assert not O.residual(dist, x)[1] and O.jacobian_rows(dist, x)[1]
    m, grad, flags = E.constraint_measure(dist, x)
    assert flags == 2 and m == 0.0 and np.all(grad == 0.0)
    # ArcRadius: each row on its own -- the start on the centre guards its row, the end's row stays
    arc = O.stack([O.arc_radius((0, 1), (2, 3), (4, 5), 1.0)])[0]
    m, grad, flags = E.constraint_measure(arc, x)
    rows, deg = _oracle_rows(arc, x)
    assert flags == 2 and deg and m == np.hypot(1.0 - 2.0, 1.0 - 3.0) / 2.0
    assert np.all(np.abs(grad - rows.mean(axis=0)) <= 1e-10) and np.all(grad[2:4] == 0.0)
    # parallel / perpendicular: not measurable
    assert E.constraint_measure(O.stack([O.lines_at_angle((0, 1), (2, 3), (4, 5), (6, 7), "parallel")])[0], x)[1].size == 0
