"""The edge-case table (tests/edge_cases.py) on the CPU: its own consistency, the oracle's guard flags against the table's
plain-Python restatement of the reference's comparisons, the two host copies of those guards (ezpz_constraint_param_derivative,
ezpz_constraint_measure), and the oracle's residuals and Jacobian rows against a 50-digit restatement of the reference's residual
definitions (constraints.rs:499-950) that shares no code with oracle/.

Bars.  Oracle residual against the 50-digit value: 1e-13 * max(1, sum of the |terms| of the row's outermost sum).  Oracle Jacobian
against mpmath.diff of the 50-digit residual: 1e-9 relative + 1e-12.  Scale: power-of-two scaling is exact in every operation of
the evaluators, so residual(s x) == s residual(x) and jacobian(s x) == jacobian(x) bit for bit wherever no guard changes state and
nothing overflows or underflows; where a guard does, the flags and zeros are the oracle's own at the scaled point.

NOT_A_DERIVATIVE lists the Jacobian entries that the reference's formula deliberately does not take from the residual (none of
them is met at the generic points; the branch cases reach them and compare at the reference's value)."""
import math

import mpmath as mp
import numpy as np
import pytest

import edge_cases as T
import ezpz_amd as E
from oracle import oracle as O

mp.mp.dps = 50

# cases per guard site: (below, at, above).  A site cannot lose a case without this table changing.
SITE_COUNTS = {
    "R:531": (2, 2, 2), "J:1032": (2, 2, 2),
    "J:1107": (1, 1, 1),
    "J:1174": (3, 3, 3),
    "J:1217": (1, 1, 1),
    "R:632": (4, 4, 4), "J:1373": (4, 4, 4),
    "J:1437": (2, 2, 2),
    "J:1559": (2, 2, 2),
    "R:729": (2, 1, 1), "J:none": (2, 1, 1),
    "R:756": (5, 3, 5), "J:1692": (5, 3, 5),
    "R:778": (5, 3, 5), "J:1750": (5, 3, 5),
    "J:2381": (2, 0, 2),
    "R:829": (3, 3, 3), "J:1908": (3, 3, 3),
    "R:879": (3, 1, 4), "J:2079": (3, 1, 4),
    "R:935": (2, 2, 2), "J:2195": (2, 2, 2),
}

# Jacobian entries the reference does not differentiate: (kind, entry, constraints.rs line, what it uses instead)
NOT_A_DERIVATIVE = (
    ("LineTangentToCircle", "d r / d radius at radius == +-0.0", ":1057", "-signum(radius): -1 at +0.0, +1 at -0.0 (|radius| has no derivative there)"),
    ("CircleTangentToCircle", "d r / d a_r, d r / d b_r at a radius == +-0.0", ":1121-1122", "signum of the radius: +-1 by the sign bit of the zero"),
    ("CircleTangentToCircle", "interior, |a_r| == |b_r|", ":1125", "signum(|a_r| - |b_r|) = signum(+0.0) = +1 (| |a_r| - |b_r| | has a kink there)"),
)


# ---- the table's own consistency ----------------------------------------------------------------------------------------------
def test_table_has_every_site_on_both_sides_of_its_threshold():
    counts = T.site_counts()
    assert set(counts) == set(T.RESIDUAL_SITES) | set(T.JACOBIAN_SITES)
    for site, c in sorted(counts.items()):
        T.log(f"cases per site  {site:7s} below {c['below']} at {c['at']} above {c['above']}")
        assert (c["below"], c["at"], c["above"]) == SITE_COUNTS[site], site
        assert c["below"] >= 1 and c["above"] >= 1, site
    # the bands where exactly one of the two evaluators fires
    one_sided = {c.kind for c in T.GUARD if c.expect[0] != c.expect[1]}
    assert one_sided == {O.DISTANCE, O.DISTANCE_VAR, O.ARC_RADIUS, O.CIRCLE_TANGENT_TO_CIRCLE, O.LINES_EQUAL_LENGTH, O.ARC, O.SYMMETRIC,
                         O.POINT_LINE_DISTANCE, O.HORIZONTAL_POINT_LINE_DISTANCE}
    at_eps = [c for c in T.GUARD if c.kind == O.HORIZONTAL_POINT_LINE_DISTANCE and c.side == "at"]
    assert at_eps and all(c.expect == (True, False) for c in at_eps)
    # both outcomes occur at every site
    for site in counts:
        col = 0 if site.startswith("R:") else 1
        seen = {c.expect[col] for c in T.GUARD if site in c.sites}
        assert seen == ({False} if site == "J:none" else {False, True}), site
    assert all(len(c.x) == T.N_VARS and int(c.rec["ids"].max()) < T.N_VARS for c in T.CASES)


def test_margins_and_the_drop_share():
    for c in T.BRANCH:
        if c.kind == O.POINT_ARC_COINCIDENT and "pac" in c.tags:
            gap_a, gap_d = T.pac_margins(c.x[list(c.rec["ids"])])
            if "tie_angle" in c.tags:
                assert gap_a == 0.0 and gap_d >= T.MARGIN, c.name
            elif "tie_distance" in c.tags:
                assert gap_d == 0.0 and gap_a >= T.MARGIN, c.name
            else:
                assert gap_a >= T.MARGIN and (gap_d is None or gap_d >= T.MARGIN), (c.name, gap_a, gap_d)
                assert c.margin >= T.MARGIN and c.margin_of, c.name
        else:
            # no decision of these cases compares two libm results (PointArcCoincident with all ids one variable: its guard fires
            # before the classification)
            assert c.margin is None, c.name
            assert c.kind != O.POINT_ARC_COINCIDENT or O.residual(c.rec, c.x)[1], c.name
    for name, reason in T.DROPPED:
        T.log(f"dropped by the margin rule  {name}: {reason}")
    T.log(f"margin rule: {len(T.DROPPED)} of {len(T.BRANCH) + len(T.DROPPED)} branch cases dropped, 0 of {len(T.GUARD)} guard cases")
    assert len(T.DROPPED) * 10 <= len(T.BRANCH) + len(T.DROPPED)
    assert all(c.group != "guard" for c in T.CASES if c.name in {n for n, _ in T.DROPPED})
    per_kind = {k: len(v) for k, v in T.by_kind().items()}
    assert set(per_kind) == set(range(O.NUM_KINDS)) and all(n >= 10 for n in per_kind.values()), per_kind
    assert len(T.SCALE) == 8 * O.NUM_KINDS
    # the signs of zero the branch cases promise
    for c in T.BRANCH:
        if "cross_zero" in c.tags:
            x = c.x
            u, v = ((x[2] - x[0], x[3] - x[1]), (x[6] - x[4], x[7] - x[5])) if c.kind == O.LINES_AT_ANGLE else \
                ((x[2] - x[0], x[3] - x[1]), (x[4] - x[0], x[5] - x[1]))
            cross = u[0] * v[1] - u[1] * v[0]
            assert cross == 0.0 and bool(np.signbit(cross)) == ("cross-0" in c.tags[1]), c.name


# ---- the oracle and the two host copies at every guard case ----------------------------------------------------------------------
def _dense_rows(rec, x):
    rows, deg = O.jacobian_rows(rec, x)
    J = np.zeros((len(rows), T.N_VARS))
    with np.errstate(invalid="ignore", over="ignore"):
        for k, row in enumerate(rows):
            for i, pd in row:
                J[k, i] += pd
    return J, deg


@pytest.mark.parametrize("case", T.GUARD, ids=[c.name for c in T.GUARD])
def test_oracle_flags_equal_the_restated_comparisons(case):
    r, d0 = O.residual(case.rec, case.x)
    J, d1 = _dense_rows(case.rec, case.x)
    assert (d0, d1) == case.expect, (case.name, (d0, d1), case.expect)
    if d0:
        assert all(v == 0.0 for v in r)
    else:
        assert any(v != 0.0 for v in r), r  # (an axis-aligned case may have one of two rows at zero)
    zeroed = case.jac_rows if case.jac_rows is not None else (case.expect[1],) * len(J)
    for k, z in enumerate(zeroed):
        assert np.all(J[k] == 0.0) if z else np.any(J[k] != 0.0), (case.name, k, J[k])


def test_oracle_solve_without_a_step_logs_one_warning_per_evaluator_that_fires():
    """max_iterations = 0: the reference evaluates residual and Jacobian once, logs their warnings and returns the start values.
    HorizontalPointLineDistance below / at / above |dy| = EPS: 2 / 1 / 0 warnings (`<=` at :778, `<` at :1750)."""
    seen = {}
    for case in T.GUARD:
        if not case.finite:
            continue
        out = O.solve([case.rec], case.x, O.Config(max_iterations=0))
        assert out.error == 0 and out.iterations == 0 and out.final_values.tobytes() == case.x.tobytes(), case.name
        assert len(out.warnings) == int(case.expect[0]) + int(case.expect[1]), (case.name, out.warnings)
        if case.kind == O.HORIZONTAL_POINT_LINE_DISTANCE and case.quantity == "abs_d+":
            seen[case.side] = len(out.warnings)
    assert seen == {"below": 2, "at": 1, "above": 0}


def test_dparam_host_copy_has_the_residual_guards():
    done = set()
    for case in T.GUARD:
        if not E.constraint_has_param(case.rec):
            continue
        g, deg = E.constraint_param_derivative(case.rec, case.x)
        assert deg == case.expect[0], case.name
        assert len(g) == O.residual_dim(case.rec)
        if deg:
            assert np.all(g == 0.0), case.name
        else:
            assert np.all(g != 0.0), (case.name, g)
        done.add(case.kind)
    # every parametrised kind that has a residual guard, and the two whose Jacobian alone is guarded
    assert done == {O.DISTANCE, O.ARC_RADIUS, O.LINES_AT_ANGLE, O.POINT_LINE_DISTANCE, O.VERTICAL_POINT_LINE_DISTANCE,
                    O.HORIZONTAL_POINT_LINE_DISTANCE, O.ARC_LENGTH, O.ARC_ANGLE, O.POINTS_AT_ANGLE}


def expected_measure_flags(case):
    """include/ezpz_amd.h, ezpz_constraint_measure: bit 0 the residual's guard; bit 1 distance_jac's guard of a Distance row."""
    grad_guard = case.expect[1] if case.kind in (O.DISTANCE, O.ARC_RADIUS) else False
    return (1 if case.expect[0] else 0) | (2 if grad_guard else 0)


def test_measure_host_copy_has_the_documented_guards():
    done = set()
    for case in T.GUARD:
        if not E.constraint_has_param(case.rec):
            continue
        m, grad, flags = E.constraint_measure(case.rec, case.x)
        assert flags == expected_measure_flags(case), (case.name, flags)
        if flags & 1:
            assert m == 0.0 and np.all(grad == 0.0), case.name
        elif case.kind in (O.DISTANCE, O.ARC_RADIUS):
            zeroed = case.jac_rows if case.jac_rows is not None else (case.expect[1],)
            ids = [(0, 1, 2, 3), (0, 1, 4, 5)]
            for k, z in enumerate(zeroed):  # the guarded row contributes zeros: its own point's slots
                own = list(ids[k][2:])
                assert np.all(grad[own] == 0.0) if z else np.any(grad[own] != 0.0), (case.name, k, grad)
            assert m != 0.0
        else:
            assert np.any(grad != 0.0), case.name
        done.add(case.kind)
    assert len(done) == 9


# ---- 50-digit restatement of the 25 residuals (constraints.rs:499-950) -----------------------------------------------------------
def _mp_rot(tag, val):
    """rotation_for_angle_kind (:2641-2647): (cos, sin)."""
    if tag == O.ANGLE_PARALLEL:
        return mp.mpf(1), mp.mpf(0)
    if tag == O.ANGLE_PERPENDICULAR:
        return mp.mpf(0), mp.mpf(1)
    rad = mp.mpf(val) * mp.pi / 180 if tag == O.ANGLE_OTHER_DEG else mp.mpf(val)
    return mp.cos(rad), mp.sin(rad)


def _mp_lines_at_angle(u, v, tag, val):
    c, s = _mp_rot(tag, val)
    riv = (c * v[0] + s * v[1], -s * v[0] + c * v[1])  # R^-1 v
    mean = (mp.hypot(*u) + mp.hypot(*v)) / 2
    a, b = u[0] * riv[1], u[1] * riv[0]
    return [((a - b) / mean, (abs(a) + abs(b)) / mean)]


def mp_residual(rec, x):
    """[(row value, sum of the |terms| of its outermost sum)] in 50-digit arithmetic; x: mpf values."""
    kind, tag, param = int(rec["kind"]), int(rec["tag"]), mp.mpf(float(rec["param"]))
    X = [x[int(i)] for i in rec["ids"]]
    A = abs
    if kind == O.LINE_TANGENT_TO_CIRCLE:  # :509-544
        u, v = (X[2] - X[0], X[3] - X[1]), (X[4] - X[0], X[5] - X[1])
        sign = -1 if tag == O.LINE_RIGHT else 1
        a, b, mag_u = u[0] * v[1], u[1] * v[0], mp.hypot(*u)
        return [(sign * (a - b) / mag_u - A(X[6]), (A(a) + A(b)) / mag_u + A(X[6]))]
    if kind == O.CIRCLE_TANGENT_TO_CIRCLE:  # :545-564
        dist = mp.hypot(X[0] - X[3], X[1] - X[4])
        ar, br = A(X[2]), A(X[5])
        return [((A(ar - br) if tag == O.CIRCLE_INTERIOR else ar + br) - dist, ar + br + dist)]
    if kind == O.DISTANCE:  # :565-574
        d = mp.hypot(X[0] - X[2], X[1] - X[3])
        return [(d - param, d + A(param))]
    if kind == O.DISTANCE_VAR:  # :575-583
        d = mp.sqrt((X[0] - X[2]) ** 2 + (X[1] - X[3]) ** 2)
        return [(-X[4] + d, A(X[4]) + d)]
    if kind == O.VERTICAL_DISTANCE:  # :584-591
        return [(X[1] - X[3] - param, A(X[1]) + A(X[3]) + A(param))]
    if kind == O.HORIZONTAL_DISTANCE:  # :592-596
        return [(X[0] - X[2] - param, A(X[0]) + A(X[2]) + A(param))]
    if kind == O.VERTICAL:  # :597-601
        return [(X[0] - X[2], A(X[0]) + A(X[2]))]
    if kind == O.HORIZONTAL:  # :602-606
        return [(X[1] - X[3], A(X[1]) + A(X[3]))]
    if kind == O.FIXED:  # :607-610
        return [(X[0] - param, A(X[0]) + A(param))]
    if kind == O.SCALAR_EQUAL:  # :611-616
        return [(X[0] - X[1], A(X[0]) + A(X[1]))]
    if kind == O.LINES_AT_ANGLE:  # :617-640
        return _mp_lines_at_angle((X[2] - X[0], X[3] - X[1]), (X[6] - X[4], X[7] - X[5]), tag, float(rec["param"]))
    if kind == O.POINTS_COINCIDENT:  # :641-648
        return [(X[0] - X[2], A(X[0]) + A(X[2])), (X[1] - X[3], A(X[1]) + A(X[3]))]
    if kind == O.CIRCLE_RADIUS:  # :649-652
        return [(X[2] - param, A(X[2]) + A(param))]
    if kind == O.LINES_EQUAL_LENGTH:  # :653-658
        l0, l1 = mp.hypot(X[0] - X[2], X[1] - X[3]), mp.hypot(X[4] - X[6], X[5] - X[7])
        return [(l0 - l1, l0 + l1)]
    if kind == O.ARC_RADIUS:  # :659-682
        d0, d1 = mp.hypot(X[0] - X[2], X[1] - X[3]), mp.hypot(X[0] - X[4], X[1] - X[5])
        return [(d0 - param, d0 + A(param)), (d1 - param, d1 + A(param))]
    if kind == O.ARC:  # :683-696
        d0, d1 = mp.hypot(X[2] - X[0], X[3] - X[1]), mp.hypot(X[4] - X[0], X[5] - X[1])
        return [(d0 - d1, d0 + d1)]
    if kind == O.MIDPOINT:  # :697-711
        return [(X[4] - X[0] / 2 - X[2] / 2, A(X[4]) + A(X[0]) / 2 + A(X[2]) / 2),
                (X[5] - X[1] / 2 - X[3] / 2, A(X[5]) + A(X[1]) / 2 + A(X[3]) / 2)]
    if kind == O.POINT_LINE_DISTANCE:  # :712-740, equation_of_line :2625-2639
        px, py, lpx, lpy, lqx, lqy = X[:6]
        a, b = lpy - lqy, lqx - lpx
        den = mp.hypot(a, b)
        terms = (a * px, b * py, lpx * lqy, -lqx * lpy)
        return [(sum(terms) / den - param, sum(A(t) for t in terms) / den + A(param))]
    if kind in (O.VERTICAL_POINT_LINE_DISTANCE, O.HORIZONTAL_POINT_LINE_DISTANCE):  # :741-785
        ax, ay, px, py, qx, qy = X[:6]
        if kind == O.HORIZONTAL_POINT_LINE_DISTANCE:
            ax, ay, px, py, qx, qy = ay, ax, py, px, qy, qx
        t = (qy - py) / (qx - px) * (ax - px)
        return [(ay - py - t - param, A(ay) + A(py) + A(t) + A(param))]
    if kind == O.SYMMETRIC:  # :786-808, reflect: vector.rs:58-69
        p, q, a, b = X[0:2], X[2:4], X[4:6], X[6:8]
        w, d = (a[0] - p[0], a[1] - p[1]), (q[0] - p[0], q[1] - p[1])
        k = (w[0] * d[0] + w[1] * d[1]) / (d[0] * d[0] + d[1] * d[1])
        refl = (2 * k * d[0] - w[0], 2 * k * d[1] - w[1])
        return [(refl[i] - b[i] + p[i], A(2 * k * d[i]) + A(w[i]) + A(b[i]) + A(p[i])) for i in range(2)]
    if kind == O.POINT_ARC_COINCIDENT:  # :809-858, classify :2593-2606
        c = X[0:2]
        s, e, p = [(X[i] - c[0], X[i + 1] - c[1]) for i in (2, 4, 6)]
        r, r_e, r_p = mp.hypot(*s), mp.hypot(*e), mp.hypot(*p)
        ep = (e[0] * r / r_e, e[1] * r / r_e)
        ang = lambda a, b: mp.atan2(a[0] * b[1] - a[1] * b[0], a[0] * b[0] + a[1] * b[1]) % (2 * mp.pi)
        if ang(s, p) < ang(s, ep):
            return [(p[i] * (r / r_p - 1), A(p[i]) * (r / r_p + 1)) for i in range(2)]
        near = ep if (ep[0] - p[0]) ** 2 + (ep[1] - p[1]) ** 2 < (s[0] - p[0]) ** 2 + (s[1] - p[1]) ** 2 else s
        return [(near[i] - p[i], A(near[i]) + A(p[i])) for i in range(2)]
    if kind == O.ARC_LENGTH:  # :859-896
        ux, uy = X[2] - X[0], X[3] - X[1]
        alpha = param / mp.hypot(ux, uy)
        ca, sa = mp.cos(alpha), mp.sin(alpha)
        return [((X[4] - X[0]) - (ca * ux - sa * uy), A(X[4]) + A(X[0]) + A(ca * ux) + A(sa * uy)),
                ((X[5] - X[1]) - (sa * ux + ca * uy), A(X[5]) + A(X[1]) + A(sa * ux) + A(ca * uy))]
    if kind == O.ARC_ANGLE:  # :897-915
        return _mp_lines_at_angle((X[2] - X[0], X[3] - X[1]), (X[4] - X[0], X[5] - X[1]), tag, float(rec["param"]))
    if kind == O.POINTS_AT_ANGLE:  # :916-948
        u, v = (X[2] - X[0], X[3] - X[1]), (X[4] - X[0], X[5] - X[1])
        lu, lv = mp.hypot(*u), mp.hypot(*v)
        c, s = _mp_rot(tag, float(rec["param"]))
        ru = (c * u[0] - s * u[1], s * u[0] + c * u[1])
        mean = (lu + lv) / 2
        return [((v[i] * lu - ru[i] * lv) / mean, (A(v[i]) * lu + A(ru[i]) * lv) / mean) for i in range(2)]
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", range(O.NUM_KINDS), ids=O.KIND_NAMES)
def test_oracle_against_the_50_digit_restatement(kind):
    worst_r = worst_j = 0.0
    for case in T.by_kind(("scale",))[kind]:
        xm = [mp.mpf(float(v)) for v in case.x]
        r, deg = O.residual(case.rec, case.x)
        assert not deg
        want = mp_residual(case.rec, xm)
        assert len(want) == len(r)
        for got, (val, mag) in zip(r, want):
            err = float(abs(mp.mpf(got) - val) / max(mp.mpf(1), mag))
            worst_r = max(worst_r, err)
            assert err <= 1e-13, (case.name, got, val)
        J, deg = _dense_rows(case.rec, case.x)
        assert not deg
        for var in sorted({int(i) for i in case.rec["ids"][: O.KIND_NUM_IDS[kind]]}):
            for row in range(len(r)):
                def f(t, row=row, var=var):
                    y = list(xm)
                    y[var] = t
                    return mp_residual(case.rec, y)[row][0]

                d = mp.diff(f, xm[var])
                err = float(abs(mp.mpf(J[row, var]) - d) / (abs(d) + mp.mpf("1e-3")))  # 1e-9 relative + 1e-12
                worst_j = max(worst_j, err)
                assert abs(mp.mpf(J[row, var]) - d) <= 1e-9 * abs(d) + 1e-12, (case.name, row, var, J[row, var], d)
    T.log(f"mpmath  {O.KIND_NAMES[kind]:28s} residual {worst_r:.2e} of 1e-13   jacobian {worst_j:.2e} of 1e-9")
    print(f"{O.KIND_NAMES[kind]}: largest residual error {worst_r:.2e} (x max(1, sum|terms|)), largest Jacobian error {worst_j:.2e} (relative)")


def test_the_entries_the_reference_does_not_differentiate():
    """NOT_A_DERIVATIVE at the branch cases that reach them: the oracle gives the reference's value."""
    assert len(NOT_A_DERIVATIVE) == 3
    by_name = {c.name: c for c in T.BRANCH}
    for tag in ("left", "right"):
        for rname, want in (("+r", -1.0), ("-r", 1.0), ("+0", -1.0), ("-0", 1.0)):  # -signum(radius), :1057
            J, deg = _dense_rows(by_name[f"LineTangent/{tag}/radius{rname}"].rec, by_name[f"LineTangent/{tag}/radius{rname}"].x)
            assert not deg and J[0, 6] == want
    for an, bn, tag, want in (("+0", "+r", "exterior", (1.0, 1.0)), ("-0", "+r", "exterior", (-1.0, 1.0)), ("+r", "-0", "exterior", (1.0, -1.0)),
                              ("+0", "+r", "interior", (-1.0, 1.0)), ("-0", "-r", "interior", (1.0, -1.0))):
        c = by_name[f"CircleTangent/{tag}/a{an}/b{bn}"]
        J, deg = _dense_rows(c.rec, c.x)
        assert not deg and (J[0, 2], J[0, 5]) == want, (c.name, J[0])
    for signs, want in (("++", (1.0, -1.0)), ("+-", (1.0, 1.0)), ("-+", (-1.0, -1.0)), ("--", (-1.0, 1.0))):  # inner = signum(+0.0) = 1
        c = by_name[f"CircleTangent/interior/equal_radii{signs}"]
        J, deg = _dense_rows(c.rec, c.x)
        assert not deg and (J[0, 2], J[0, 5]) == want, (c.name, J[0])


# ---- the scale property on the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", T.SCALE_EXPONENTS)
def test_oracle_scales_exactly_by_powers_of_two(k):
    s = math.ldexp(1.0, k)
    exact = guarded = 0
    for case in T.SCALE:
        r1, _ = O.residual(case.rec, case.x)
        J1, _ = _dense_rows(case.rec, case.x)
        rec, x = T.scaled(case, k)
        rs, d0 = O.residual(rec, x)
        Js, d1 = _dense_rows(rec, x)
        if d0:
            assert all(v == 0.0 for v in rs), case.name
        if d1 and case.kind != O.ARC_RADIUS:
            assert np.all(Js == 0.0), case.name
        if d0 or d1:
            guarded += 1
            assert k < 0, (case.name, k)  # only shrinking moves a generic point into a guard
            continue
        if k == 520:  # the squares overflow while hypot does not: non-finite or not, checked on the device against the oracle
            continue
        assert np.array_equal(np.asarray(rs), s * np.asarray(r1)), (case.name, rs, r1)
        assert np.array_equal(Js, J1), (case.name, Js, J1)
        exact += 1
    T.log(f"oracle scale 2^{k}: {exact} of {len(T.SCALE)} cases bitwise in residual and Jacobian, {guarded} crossed into a guard")
    assert exact + guarded > 0 or k == 520
