"""The table of edge cases for the constraint evaluators (con_residual / con_jacobian of csrc/constraint_eval.hip.hpp and the two
hand copies of their guards, constraint_dparam.hip.hpp and constraint_measure.hip.hpp).  Data only: this module loads no device
code; tests/test_edge_cases_cpu.py and tests/test_gpu_edge_cases.py evaluate it.

Every case is one record over 8 variables and one value vector.  Three groups:

  (a) GUARD  one case per guarded quantity of each of the reference's guard sites, one ulp below the threshold, at it (where it is
      representable) and one ulp above.  `expect` = (residual fires, Jacobian fires) comes from a plain-Python restatement of the
      reference's comparison (constraints.rs line in `sites`), never from the oracle.  Python floats are IEEE doubles and the
      libraries are built without fused multiply-add, so the expressions reproduce the reference's arithmetic bit for bit.  A
      quantity that goes through hypot is axis-aligned from the origin (hypot(d, 0) == d and d - 0 == d whatever the libm); one
      formed by plain arithmetic is also taken oblique and off the origin, by searching the neighbouring doubles of a coordinate.
  (b) BRANCH  signs of zero, branch cuts, large arguments, duplicate ids.  A decision that compares two libm results is either a
      tie by construction (`margin` == 0: identical or power-of-two scaled arguments) or clear by `margin` >= 1e-9 (angles in
      rad, squared distances relative); `margin_of` names the quantity.  DROPPED lists what the margin rule removed.
  (c) SCALE  8 generic (record, x) pairs per kind, unguarded at scale 1, to be taken at s = 2^k for k in SCALE_EXPONENTS.
"""
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

import gen
from oracle import oracle as O

EPS = 1e-4  # lib.rs:43
EPS2 = EPS * EPS
N_VARS = 8
SCALE_EXPONENTS = (-30, -8, 10, 40, 200, 520)
SCALED_PARAM_KINDS = {O.DISTANCE, O.VERTICAL_DISTANCE, O.HORIZONTAL_DISTANCE, O.FIXED, O.CIRCLE_RADIUS, O.ARC_RADIUS, O.ARC_LENGTH,
                      O.POINT_LINE_DISTANCE, O.VERTICAL_POINT_LINE_DISTANCE, O.HORIZONTAL_POINT_LINE_DISTANCE}
MARGIN = 1e-9
WEIGHTS = (1.0, 2.5, 0.5)

hyp = math.hypot


@dataclass
class Case:
    name: str
    rec: np.ndarray
    x: np.ndarray
    group: str                                   # "guard" | "branch" | "scale"
    sites: Tuple[str, ...] = ()                  # guard: "R:531", "J:1032", ... (constraints.rs lines)
    quantity: str = ""                           # guard: the guarded quantity this case walks
    side: str = ""                               # guard: "below" | "at" | "above" the threshold of `quantity`
    expect: Optional[Tuple[bool, bool]] = None   # guard: (residual fires, Jacobian fires)
    jac_rows: Optional[Tuple[bool, ...]] = None  # guard: per Jacobian row "this row is zeroed" (default: every row = expect[1])
    margin: Optional[float] = None               # branch: 0.0 = tie by construction, else >= MARGIN
    margin_of: str = ""
    finite: bool = True                          # False: non-finite values appear (kept away from the solve routes)
    tags: Tuple[str, ...] = field(default_factory=tuple)

    @property
    def kind(self) -> int:
        return int(self.rec["kind"])


CASES = []
DROPPED = []  # (name, reason): branch cases the margin rule removed


def _x(*vals):
    v = np.zeros(N_VARS)
    v[: len(vals)] = vals
    return v


def _around(t):
    """(side, value) one ulp below, at and one ulp above the representable threshold t."""
    return (("below", float(np.nextafter(t, -np.inf))), ("at", float(t)), ("above", float(np.nextafter(t, np.inf))))


def _search(f, lo, steps=4000):
    """Walks the doubles upward from lo until the predicate f flips from True to False: (last True, first False)."""
    a = float(lo)
    assert f(a), lo
    for _ in range(steps):
        b = float(np.nextafter(a, np.inf))
        if not f(b):
            return a, b
        a = b
    raise AssertionError("no flip within the searched doubles")


def _bisect(f, lo, hi):
    """f(lo) True, f(hi) False, f monotone: the adjacent doubles (last True, first False)."""
    assert f(lo) and not f(hi)
    while float(np.nextafter(lo, np.inf)) < hi:
        mid = lo + (hi - lo) / 2.0
        if f(mid):
            lo = mid
        else:
            hi = mid
    return float(lo), float(hi)


def _guard(name, rec, sites, quantity, side, x, expect, jac_rows=None, finite=True):
    CASES.append(Case(f"{name}/{quantity}/{side}", rec, np.asarray(x, dtype=np.float64), "guard", tuple(sites), quantity, side,
                      (bool(expect[0]), bool(expect[1])), jac_rows, finite=finite))


P = lambda i: (2 * i, 2 * i + 1)
DEG30 = ("deg", 30.0)


# ---- (a) guard cases ---------------------------------------------------------------------------------------------------------
def _guards():
    # LineTangentToCircle: mag_u <= EPS in both (:531, :1032)
    rec = O.line_tangent_to_circle(P(0), P(1), P(2), 6, side=O.LINE_LEFT)
    for side, q in _around(EPS):
        for axis in ("x", "y"):
            x = _x(0, 0, q, 0, 0.3, 0.7, 0.5) if axis == "x" else _x(0, 0, 0, q, 0.3, 0.7, 0.5)
            mag_u = hyp(x[2] - x[0], x[3] - x[1])
            _guard("LineTangent", rec, ("R:531", "J:1032"), "mag_u_" + axis, side, x, (mag_u <= EPS, mag_u <= EPS))

    # CircleTangentToCircle: mag_d <= EPS, Jacobian only (:1107)
    rec = O.circle_tangent_to_circle(P(0), 2, (3, 4), 5, side=O.CIRCLE_EXTERIOR)
    for side, q in _around(EPS):
        x = _x(0, 0, 0.5, q, 0, 0.25)
        mag_d = hyp(x[3] - x[0], x[4] - x[1])
        _guard("CircleTangent", rec, ("J:1107",), "mag_d", side, x, (False, mag_d <= EPS))

    # Distance: dist < EPS, Jacobian only (:1174); each row of ArcRadius
    rec = O.distance(P(0), P(1), 0.75)
    for side, q in _around(EPS):
        x = _x(0, 0, q, 0)
        dist = hyp(x[0] - x[2], x[1] - x[3])
        _guard("Distance", rec, ("J:1174",), "dist", side, x, (False, dist < EPS))
    rec = O.arc_radius(P(0), P(1), P(2), 0.75)
    for side, q in _around(EPS):
        for row, x in ((0, _x(0, 0, q, 0, 0.6, 0.8)), (1, _x(0, 0, 0.6, 0.8, 0, q))):
            d0, d1 = hyp(x[0] - x[2], x[1] - x[3]), hyp(x[0] - x[4], x[1] - x[5])
            _guard("ArcRadius", rec, ("J:1174",), f"dist_row{row}", side, x, (False, d0 < EPS or d1 < EPS), jac_rows=(d0 < EPS, d1 < EPS))

    # DistanceVar: dist < EPS, Jacobian only (:1217)
    rec = O.distance_var(P(0), P(1), 4)
    for side, q in _around(EPS):
        x = _x(0, 0, 0, q, 0.3)
        dist = hyp(x[0] - x[2], x[1] - x[3])
        _guard("DistanceVar", rec, ("J:1217",), "dist", side, x, (False, dist < EPS))

    # LinesAtAngle / ArcAngle: len_u <= EPS || len_v <= EPS in both (:632, :1373)
    for name, rec, arc in (("LinesAtAngle", O.lines_at_angle(P(0), P(1), P(2), P(3), DEG30), False),
                           ("ArcAngle", O.arc_angle(P(0), P(1), P(2), ("rad", 0.5)), True)):
        for side, q in _around(EPS):
            for quantity in ("len_u", "len_v"):
                if arc:  # u = start - center, v = end - center
                    x = _x(0, 0, q, 0, 0.6, 0.8) if quantity == "len_u" else _x(0, 0, 0.6, 0.8, 0, q)
                    lu, lv = hyp(x[2] - x[0], x[3] - x[1]), hyp(x[4] - x[0], x[5] - x[1])
                else:    # u = l0.p1 - l0.p0, v = l1.p1 - l1.p0
                    x = _x(0, 0, q, 0, 0, 0, 0.6, 0.8) if quantity == "len_u" else _x(0, 0, 0.6, 0.8, 0, 0, 0, q)
                    lu, lv = hyp(x[2] - x[0], x[3] - x[1]), hyp(x[6] - x[4], x[7] - x[5])
                fires = lu <= EPS or lv <= EPS
                _guard(name, rec, ("R:632", "J:1373"), quantity, side, x, (fires, fires))

    # LinesEqualLength: len0 < EPS || len1 < EPS, Jacobian only (:1437)
    rec = O.lines_equal_length(P(0), P(1), P(2), P(3))
    for side, q in _around(EPS):
        for quantity, x in (("len0", _x(0, 0, q, 0, 0.1, 0.2, 0.7, 1.0)), ("len1", _x(0.1, 0.2, 0.7, 1.0, 0, 0, 0, q))):
            l0, l1 = hyp(x[0] - x[2], x[1] - x[3]), hyp(x[4] - x[6], x[5] - x[7])
            _guard("LinesEqualLength", rec, ("J:1437",), quantity, side, x, (False, l0 < EPS or l1 < EPS))

    # Arc: dist0 <= EPS || dist1 <= EPS, Jacobian only (:1559)
    rec = O.arc(P(0), P(1), P(2))
    for side, q in _around(EPS):
        for quantity, x in (("dist0", _x(0, 0, q, 0, 0.6, 0.8)), ("dist1", _x(0, 0, 0.6, 0.8, 0, q))):
            d0, d1 = hyp(x[2] - x[0], x[3] - x[1]), hyp(x[4] - x[0], x[5] - x[1])
            _guard("Arc", rec, ("J:1559",), quantity, side, x, (False, d0 <= EPS or d1 <= EPS))

    # PointLineDistance: den < EPS in the residual (:729); no guard in the Jacobian (pds_for_point_line divides unguarded)
    rec = O.point_line_distance(P(0), P(1), P(2), 0.25)
    for side, q in _around(EPS):
        x = _x(0.3, 0.4, 0, 0, q, 0)
        den = hyp(x[3] - x[5], x[4] - x[2])
        _guard("PointLineDistance", rec, ("R:729", "J:none"), "den", side, x, (den < EPS, False))
    x = _x(0.3, 0.4, 0.5, 0.5, 0.5, 0.5)  # the line's points coincide: 0 / 0 in the Jacobian is part of the contract
    _guard("PointLineDistance", rec, ("R:729", "J:none"), "den_zero", "below", x, (hyp(x[3] - x[5], x[4] - x[2]) < EPS, False), finite=False)

    # Vertical / HorizontalPointLineDistance (:756 / :1692 both `<=`; :778 `<=` but :1750 `<`)
    def vpld(x):
        dx, dy = x[4] - x[2], x[5] - x[3]
        f = abs(dx) <= EPS or dx * dx + dy * dy <= EPS * EPS  # :756 and :1692
        return f, f

    def hpld(x):
        dx, dy = x[4] - x[2], x[5] - x[3]
        return (abs(dy) <= EPS or dx * dx + dy * dy <= EPS * EPS,  # :778
                abs(dy) < EPS or dx * dx + dy * dy < EPS * EPS)    # :1750

    for name, rec, sites, ev, swap in (
            ("VerticalPointLineDistance", O.vertical_point_line_distance(P(0), P(1), P(2), 0.25), ("R:756", "J:1692"), vpld, False),
            ("HorizontalPointLineDistance", O.horizontal_point_line_distance(P(0), P(1), P(2), 0.25), ("R:778", "J:1750"), hpld, True)):
        def line(px, py, d_guarded, d_other):  # q = p + (dx, dy); the guarded difference is dx (vertical) or dy (horizontal)
            return _x(0.3, 0.4, px, py, px + d_other, py + d_guarded) if swap else _x(0.3, 0.4, px, py, px + d_guarded, py + d_other)

        for side, q in _around(EPS):
            for sign in (1.0, -1.0):  # |d|: both signs
                x = line(0.0, 0.0, sign * q, 0.5)
                _guard(name, rec, sites, "abs_d" + ("+" if sign > 0 else "-"), side, x, ev(x))
        # the same difference off the origin: 1.25 + d is searched among the doubles next to 1.25 + EPS (the difference of two
        # doubles this close is exact); EPS is no multiple of their spacing, so there are two sides only
        g = 3 if swap else 2
        below, above = _search(lambda v: (v - 1.25) <= EPS, 1.25 + EPS - 64 * np.spacing(1.25))
        for side, v in (("below", below), ("above", above)):
            x = line(-0.5, 1.25, 0.0, 0.5) if swap else line(1.25, -0.5, 0.0, 0.5)
            x[g + 2] = v
            assert (abs(x[g + 2] - x[g]) <= EPS) == (side == "below")
            _guard(name, rec, sites, "abs_d_off_origin", side, x, ev(x))
        # the sum of squares with the other difference 0: d * d against EPS * EPS.  (No vector has the sum of squares inside its
        # threshold and |d| outside, beyond rounding: the clause is shadowed by the first; these cases pin its operator at the tie.)
        for side, q in _around(EPS):
            x = line(0.0, 0.0, q, 0.0)
            _guard(name, rec, sites, "sum_sq", side, x, ev(x))
        # oblique, both differences inside EPS: the sum of squares alone is searched across EPS^2 (|d| fires on both sides)
        f = lambda d: (6e-5 * 6e-5 + d * d) <= EPS * EPS
        below, above = _bisect(f, 7.9e-5, 8.1e-5)
        for side, d in (("below", below), ("above", above)):
            x = line(0.0, 0.0, 6e-5, d)
            _guard(name, rec, sites, "sum_sq_oblique", side, x, ev(x))

    # Symmetric: (dx^2 + dy^2)^2 < EPS, Jacobian only (:2381); |p - q| ~ 0.1 is not representable: two sides
    rec = O.symmetric(P(0), P(1), P(2), P(3))

    def sym(x):
        dx, dy = x[0] - x[2], x[1] - x[3]
        r = dx * dx + dy * dy
        return False, r * r < EPS

    below, above = _bisect(lambda d: sym(_x(0, 0, d, 0))[1], 0.0999, 0.1001)
    for side, d in (("below", below), ("above", above)):
        x = _x(0, 0, d, 0, 0.7, -0.2, 0.1, 0.9)
        _guard("Symmetric", rec, ("J:2381",), "r2_axis", side, x, sym(x))
    below, above = _bisect(lambda d: sym(_x(1.5, -0.25, 1.5 + 0.06, -0.25 + d))[1], 0.0799, 0.0801)
    for side, d in (("below", below), ("above", above)):
        x = _x(1.5, -0.25, 1.5 + 0.06, -0.25 + d, 0.7, -0.2, 0.1, 0.9)
        _guard("Symmetric", rec, ("J:2381",), "r2_oblique_off_origin", side, x, sym(x))

    # PointArcCoincident: r < EPS || r_e < EPS || r_p < EPS in both (:829, :1908)
    rec = O.point_arc_coincident(P(0), P(1), P(2), P(3))
    for side, q in _around(EPS):
        for quantity, x in (("r", _x(0, 0, q, 0, 0, 1, 0.5, 0.5)), ("r_e", _x(0, 0, 1, 0, 0, q, 0.5, 0.5)), ("r_p", _x(0, 0, 1, 0, 0, 1, q, 0))):
            r, r_e, r_p = hyp(x[2] - x[0], x[3] - x[1]), hyp(x[4] - x[0], x[5] - x[1]), hyp(x[6] - x[0], x[7] - x[1])
            fires = r < EPS or r_e < EPS or r_p < EPS
            _guard("PointArcCoincident", rec, ("R:829", "J:1908"), quantity, side, x, (fires, fires))

    # ArcLength: r2 = ux^2 + uy^2 <= EPS^2 in both (:879, :2079)
    rec = O.arc_length(P(0), P(1), P(2), 1e-4)

    def arclen(x):
        ux, uy = x[2] - x[0], x[3] - x[1]
        f = ux * ux + uy * uy <= EPS * EPS
        return f, f

    for side, q in _around(EPS):
        x = _x(0, 0, q, 0, 0.3, 0.4)
        _guard("ArcLength", rec, ("R:879", "J:2079"), "r2_axis", side, x, arclen(x))
    below, above = _bisect(lambda d: arclen(_x(0, 0, 6e-5, d))[0], 7.9e-5, 8.1e-5)
    for side, d in (("below", below), ("above", above)):
        x = _x(0, 0, 6e-5, d, 0.3, 0.4)
        _guard("ArcLength", rec, ("R:879", "J:2079"), "r2_oblique", side, x, arclen(x))
    below, above = _search(lambda v: arclen(_x(0.5, -0.25, 0.5 + 6e-5, v))[0], -0.25 + 8e-5 - 200 * np.spacing(0.25))
    for side, v in (("below", below), ("above", above)):
        x = _x(0.5, -0.25, 0.5 + 6e-5, v, 0.3, 0.4)
        _guard("ArcLength", rec, ("R:879", "J:2079"), "r2_off_origin", side, x, arclen(x))
    # between EPS^2 and EPS: an evaluator that compared r2 with EPS instead of EPS^2 would fire here
    x = _x(0, 0, 3e-3, 4e-3, 0.3, 0.4)
    _guard("ArcLength", rec, ("R:879", "J:2079"), "r2_between_eps2_and_eps", "above", x, arclen(x))

    # PointsAtAngle: len_u <= EPS || len_v <= EPS in both (:935, :2195)
    rec = O.points_at_angle(P(0), P(1), P(2), DEG30)
    for side, q in _around(EPS):
        for quantity, x in (("len_u", _x(0, 0, q, 0, 0.6, 0.8)), ("len_v", _x(0, 0, 0.6, 0.8, 0, q))):
            lu, lv = hyp(x[2] - x[0], x[3] - x[1]), hyp(x[4] - x[0], x[5] - x[1])
            fires = lu <= EPS or lv <= EPS
            _guard("PointsAtAngle", rec, ("R:935", "J:2195"), quantity, side, x, (fires, fires))


# ---- (b) branch and sign cases -------------------------------------------------------------------------------------------------
def _branch(name, rec, x, margin=None, margin_of="", tags=(), finite=True):
    if margin is not None and margin != 0.0 and margin < MARGIN:
        DROPPED.append((name, f"{margin_of} = {margin:.3g} < {MARGIN:g}"))
        return
    CASES.append(Case(name, rec, np.asarray(x, dtype=np.float64), "branch", margin=margin, margin_of=margin_of, tags=tuple(tags), finite=finite))


def _rem_two_pi(a):
    r = math.fmod(a, 2.0 * math.pi)
    return r + 2.0 * math.pi if r < 0.0 else r


def pac_margins(x):
    """The two libm-dependent decisions of classify_point_arc_coincident (:2593-2606) at x (center, start, end, point):
    |a_sp - a_se| in rad and, where the exterior branch is taken, the relative gap of the two squared distances."""
    c = x[0:2]
    s, e, p = x[2:4] - c, x[4:6] - c, x[6:8] - c
    r, r_e = hyp(*s), hyp(*e)
    ep = e * (r / r_e)
    ang = lambda a, b: math.atan2(a[0] * b[1] - a[1] * b[0], a[0] * b[0] + a[1] * b[1])
    a_sp, a_se = _rem_two_pi(ang(s, p)), _rem_two_pi(ang(s, ep))
    d_e = (ep[0] - p[0]) ** 2 + (ep[1] - p[1]) ** 2
    d_s = (s[0] - p[0]) ** 2 + (s[1] - p[1]) ** 2
    interior = a_sp < a_se
    return abs(a_sp - a_se), (None if interior else abs(d_e - d_s) / max(d_e, d_s, 1e-300))


def _branches():
    # tangent kinds: the radius variable +r, -r, +0.0, -0.0; both tags
    for tag, tname in ((O.LINE_LEFT, "left"), (O.LINE_RIGHT, "right")):
        rec = O.line_tangent_to_circle(P(0), P(1), P(2), 6, side=tag)
        for rname, r in (("+r", 0.5), ("-r", -0.5), ("+0", 0.0), ("-0", -0.0)):
            _branch(f"LineTangent/{tname}/radius{rname}", rec, _x(0, 0, 2, 1, 0.7, 1.9, r), tags=("signum",))
    for tag, tname in ((O.CIRCLE_EXTERIOR, "exterior"), (O.CIRCLE_INTERIOR, "interior")):
        rec = O.circle_tangent_to_circle(P(0), 2, (3, 4), 5, side=tag)
        for an, ar in (("+r", 0.75), ("-r", -0.75), ("+0", 0.0), ("-0", -0.0)):
            for bn, br in (("+r", 0.5), ("-r", -0.5), ("+0", 0.0), ("-0", -0.0)):
                if an[1] == "0" and bn[1] == "0" and an != bn:
                    continue
                _branch(f"CircleTangent/{tname}/a{an}/b{bn}", rec, _x(0.25, -0.5, ar, 1.5, 0.75, br), tags=("signum",))
        for an, ar, br in (("++", 0.5, 0.5), ("+-", 0.5, -0.5), ("-+", -0.5, 0.5), ("--", -0.5, -0.5)):  # |a_r| == |b_r|: signum(+0.0) = 1
            _branch(f"CircleTangent/{tname}/equal_radii{an}", rec, _x(0.25, -0.5, ar, 1.5, 0.75, br), tags=("signum",))

    # the three angle kinds
    def angle_rec(kind, angle_kind):
        if kind == O.LINES_AT_ANGLE:
            return O.lines_at_angle(P(0), P(1), P(2), P(3), angle_kind)
        if kind == O.ARC_ANGLE:
            return O.arc_angle(P(0), P(1), P(2), angle_kind)
        return O.points_at_angle(P(0), P(1), P(2), angle_kind)

    def angle_x(kind, u, v):  # arms u, v from base points at the origin (so that a coordinate of -0.0 gives a component of -0.0)
        return _x(0, 0, u[0], u[1], 0, 0, v[0], v[1]) if kind == O.LINES_AT_ANGLE else _x(0, 0, u[0], u[1], v[0], v[1])

    def angle_tags(kind):
        return (("deg", "rad") if kind == O.ARC_ANGLE else ("parallel", "perpendicular", "deg", "rad"))

    # exactly (anti)parallel arms with the cross product u.x v.y - u.y v.x = +0.0 and -0.0
    GEOMETRIES = (("parallel/cross+0", (1.0, 0.0), (2.0, 0.0), False, False),
                  ("parallel/cross-0", (1.0, 0.0), (2.0, -0.0), False, True),
                  ("antiparallel/cross+0", (1.0, 0.0), (-2.0, 0.0), True, False),
                  ("antiparallel/cross-0", (1.0, -0.0), (-2.0, -0.0), True, True),
                  ("parallel/oblique", (3.0, 4.0), (6.0, 8.0), False, False),
                  ("antiparallel/oblique", (3.0, 4.0), (-6.0, -8.0), True, False))
    for kind in (O.LINES_AT_ANGLE, O.ARC_ANGLE, O.POINTS_AT_ANGLE):
        for gname, u, v, anti, neg in GEOMETRIES:
            cross = u[0] * v[1] - u[1] * v[0]
            assert cross == 0.0 and bool(np.signbit(cross)) == neg, (gname, cross)
            for t in angle_tags(kind):
                ak = t if t in ("parallel", "perpendicular") else (t, (180.0 if anti else 0.0) if t == "deg" else (math.pi if anti else 0.0))
                _branch(f"{O.KIND_NAMES[kind]}/{gname}/{t}", angle_rec(kind, ak), angle_x(kind, u, v), tags=("cross_zero", gname))
        # parameters at multiples of 90 degrees, the nearest doubles of those in radians, large arguments; generic arms
        u, v = (1.25, 0.5), (-0.75, 1.5)
        for deg in (0.0, 90.0, -90.0, 180.0, -180.0, 270.0, 360.0):
            _branch(f"{O.KIND_NAMES[kind]}/deg{deg:g}", angle_rec(kind, ("deg", deg)), angle_x(kind, u, v), tags=("quadrant",))
            _branch(f"{O.KIND_NAMES[kind]}/rad_of_deg{deg:g}", angle_rec(kind, ("rad", math.radians(deg))), angle_x(kind, u, v), tags=("quadrant",))
        for rad in (1e6, 1e15):
            _branch(f"{O.KIND_NAMES[kind]}/rad{rad:g}", angle_rec(kind, ("rad", rad)), angle_x(kind, u, v), tags=("large_argument",))

    # PointArcCoincident: classify_point_arc_coincident (:2593-2606)
    rec = O.point_arc_coincident(P(0), P(1), P(2), P(3))

    def pac(name, c, s, e, p, tie=None):
        if c == O0:  # (0.0 + -0.0 would lose the sign of a zero component)
            x = _x(0.0, 0.0, s[0], s[1], e[0], e[1], p[0], p[1])
        else:
            x = _x(c[0], c[1], c[0] + s[0], c[1] + s[1], c[0] + e[0], c[1] + e[1], c[0] + p[0], c[1] + p[1])
        gap_a, gap_d = pac_margins(x)
        if tie == "angle":    # a_sp == a_se by construction; the distances decide, with a margin
            assert gap_a == 0.0, (name, gap_a)
            _branch("PointArcCoincident/" + name, rec, x, margin=0.0, margin_of="a_sp - a_se (identical up to a power of two)", tags=("pac", "tie_angle"))
            assert gap_d is not None and gap_d >= MARGIN, (name, gap_d)
        elif tie == "distance":
            assert gap_d == 0.0 and gap_a >= MARGIN, (name, gap_a, gap_d)
            _branch("PointArcCoincident/" + name, rec, x, margin=0.0, margin_of="|e - p|^2 - |s - p|^2 (exact arithmetic, no libm)", tags=("pac", "tie_distance"))
        else:
            m, of = (gap_a, "a_sp - a_se") if gap_d is None or gap_a < gap_d else (gap_d, "|e - p|^2 - |s - p|^2 (relative)")
            _branch("PointArcCoincident/" + name, rec, x, margin=m, margin_of=of, tags=("pac",))

    rot = lambda v, t: (math.cos(t) * v[0] - math.sin(t) * v[1], math.sin(t) * v[0] + math.cos(t) * v[1])
    O0 = (0.0, 0.0)
    s, e = (2.0, 0.0), (3.0, 4.0)  # r = 2, r_e = 5 (exact), e_proj = e * 0.4; the arc runs counter-clockwise from 0 to atan2(4, 3)
    e_proj = (e[0] * (2.0 / 5.0), e[1] * (2.0 / 5.0))
    pac("p_on_start_ray", O0, s, e, (1.0, 0.0))
    pac("p_on_start_ray_outside", O0, s, e, (3.0, 0.0))
    for k in (-1, 1, 3):  # p = 2^k e_proj: both atan2 calls see the same arguments up to a power of two
        pac(f"p_on_end_ray_2^{k}", O0, s, e, (e_proj[0] * 2.0 ** k, e_proj[1] * 2.0 ** k), tie="angle")
    pac("p_on_axis_end_ray", O0, s, (0.0, 3.0), (0.0, 1.0), tie="angle")
    for dname, d in (("1e-6", 1e-6), ("1e-3", 1e-3)):
        pac(f"p_inside_start_ray_{dname}", O0, s, e, rot((1.5, 0.0), d))
        pac(f"p_outside_start_ray_{dname}", O0, s, e, rot((1.5, 0.0), -d))
        pac(f"p_inside_end_ray_{dname}", O0, s, e, rot((0.9, 1.2), -d))
        pac(f"p_outside_end_ray_{dname}", O0, s, e, rot((0.9, 1.2), d))
    for aname, a in (("0+", 1e-6), ("0-", -1e-6), ("pi-", math.pi - 1e-6), ("pi+", math.pi + 1e-6), ("2pi-", 2.0 * math.pi - 1e-6)):
        ee = rot((1.5, 0.0), a)  # arcs whose sweep a_se is near 0, pi and 2 pi
        pac(f"a_se_{aname}/p_at_1rad", (0.5, -0.25), s, ee, rot((1.0, 0.0), 1.0))
        pac(f"a_se_{aname}/p_at_4rad", (0.5, -0.25), s, ee, rot((1.0, 0.0), 4.0))
    pac("p_exactly_opposite_the_start", O0, s, e, (-1.0, 0.0))   # cross = 2 * 0 - 0 * -1 = +0.0: a_sp = +pi
    assert np.signbit(2.0 * -0.0 - (-0.0) * -1.0)
    pac("p_exactly_opposite_the_start_cross-0", O0, (2.0, -0.0), e, (-1.0, -0.0))  # cross = -0.0: atan2 gives -pi, rem_euclid pi again
    pac("exterior_equidistant", O0, (2.0, 0.0), (0.0, 2.0), (-1.0, -1.0), tie="distance")  # strict `<`: start
    pac("exterior_nearer_start", O0, (2.0, 0.0), (0.0, 2.0), (1.5, -1.0))
    pac("exterior_nearer_end", O0, (2.0, 0.0), (0.0, 2.0), (-1.0, 1.5))

    # ArcLength: parameter 0, negative, and param / r = 1e6
    for pname, param in (("0", 0.0), ("-0", -0.0), ("negative", -1.75), ("1e6_radians", 2.0e6)):
        _branch(f"ArcLength/param_{pname}", O.arc_length(P(0), P(1), P(2), param), _x(0.5, -0.25, 2.5, -0.25, 1.0, 1.5), tags=("arc_length",))

    # linear kinds: -0.0 inputs, operands that cancel exactly
    lin = (("VerticalDistance", O.vertical_distance(P(0), P(1), 1.5), _x(0.3, 2.0, 0.7, 0.5), _x(-0.0, -0.0, 0.0, -0.0)),
           ("HorizontalDistance", O.horizontal_distance(P(0), P(1), 1.5), _x(2.0, 0.3, 0.5, 0.7), _x(-0.0, -0.0, -0.0, 0.0)),
           ("Vertical", O.vertical(P(0), P(1)), _x(1.75, 0.3, 1.75, 0.9), _x(-0.0, 1.0, 0.0, 2.0)),
           ("Horizontal", O.horizontal(P(0), P(1)), _x(0.3, 1.75, 0.9, 1.75), _x(1.0, -0.0, 2.0, -0.0)),
           ("Fixed", O.fixed(0, 1.5), _x(1.5), _x(-0.0)),
           ("ScalarEqual", O.scalar_equal(0, 1), _x(-2.25, -2.25), _x(-0.0, 0.0)),
           ("PointsCoincident", O.points_coincident(P(0), P(1)), _x(1.5, -2.5, 1.5, -2.5), _x(-0.0, 0.0, 0.0, -0.0)),
           ("CircleRadius", O.circle_radius(P(0), 2, 0.75), _x(0.1, 0.2, 0.75), _x(0.0, 0.0, -0.0)),
           ("Midpoint", O.midpoint(P(0), P(1), P(2)), _x(1.0, 3.0, 2.0, -1.0, 1.5, 1.0), _x(-0.0, -0.0, -0.0, 0.0, -0.0, 0.0)))
    for name, rec, x_cancel, x_negzero in lin:
        _branch(f"{name}/cancels_exactly", rec, x_cancel, tags=("linear",))
        _branch(f"{name}/negative_zero", rec, x_negzero, tags=("linear",))
    _branch("Fixed/negative_zero_param", O.fixed(0, -0.0), _x(0.0), tags=("linear",))

    # duplicate ids (the accumulate path of JacWriter::put, code & 0x80): all ids one variable; ids equal in pairs
    rng = np.random.default_rng(20260)
    for kind in range(O.NUM_KINDS):
        n_ids = O.KIND_NUM_IDS[kind]
        if n_ids < 4:
            continue
        base = gen.arb_constraint(np.random.default_rng(4000 + kind), kind, hi=N_VARS)
        x = np.round(rng.uniform(-8.0, 8.0, N_VARS) * 64.0) / 64.0
        for dname, ids in (("all_ids_one_variable", [3] * n_ids), ("ids_equal_in_pairs", [i // 2 for i in range(n_ids)])):
            rec = O._mk(kind, ids, float(base["param"]), tag=int(base["tag"]))
            if kind == O.POINT_ARC_COINCIDENT and dname == "ids_equal_in_pairs":
                # centre, start, end and point on the diagonal: every cross product is x * y - y * x = 0 exactly, so a_sp and a_se are
                # exactly 0 or pi whatever the libm.  Start and point on one side of the centre, the end on the other: interior, by pi.
                xd = _x(0.5, 2.5, -1.5, 1.0, *x[4:])
                gap_a, gap_d = pac_margins(xd[ids])
                assert gap_d is None and abs(gap_a - math.pi) < 1e-12, (gap_a, gap_d)
                _branch(f"{O.KIND_NAMES[kind]}/{dname}", rec, xd, margin=gap_a, margin_of="a_sp - a_se (exactly 0 and pi: all arms on the diagonal)",
                        tags=("duplicate_ids", "pac"))
                continue
            _branch(f"{O.KIND_NAMES[kind]}/{dname}", rec, x, tags=("duplicate_ids",))


# ---- (c) scale cases: generic pairs, unguarded at scale 1 ------------------------------------------------------------------------
def _scales():
    for kind in range(O.NUM_KINDS):
        rng = np.random.default_rng(5000 + kind)
        found = 0
        while found < 8:
            rec = gen.arb_constraint(rng, kind, hi=N_VARS)
            x = rng.uniform(-8.0, 8.0, N_VARS)
            if O.residual(rec, x)[1] or O.jacobian_rows(rec, x)[1]:
                continue  # (repeated ids make e.g. a Distance between one point: not generic)
            if kind == O.POINT_ARC_COINCIDENT:  # (start == end by repeated ids is a tie of the classification: not generic)
                gap_a, gap_d = pac_margins(x[list(rec["ids"])])
                if gap_a < 1e-6 or (gap_d is not None and gap_d < 1e-6):
                    continue
            r, _ = O.residual(rec, x)
            rows, _ = O.jacobian_rows(rec, x)
            if not (np.all(np.isfinite(r)) and all(math.isfinite(pd) for row in rows for _, pd in row)):
                continue
            CASES.append(Case(f"{O.KIND_NAMES[kind]}/generic{found}", rec, x, "scale"))
            found += 1


def scaled(case, k):
    """(record, x) of a scale case at s = 2^k: x scaled, and the parameter for the ten kinds whose parameter is a length."""
    s = math.ldexp(1.0, k)
    rec = case.rec.copy()
    if case.kind in SCALED_PARAM_KINDS:
        rec["param"] = float(case.rec["param"]) * s
    return rec, case.x * s


_guards()
_branches()
_scales()

GUARD = [c for c in CASES if c.group == "guard"]
BRANCH = [c for c in CASES if c.group == "branch"]
SCALE = [c for c in CASES if c.group == "scale"]
assert len({c.name for c in CASES}) == len(CASES)

# every guard site of the reference: (site, kinds that reach it)
RESIDUAL_SITES = ("R:531", "R:632", "R:729", "R:756", "R:778", "R:829", "R:879", "R:935")
JACOBIAN_SITES = ("J:1032", "J:1107", "J:1174", "J:1217", "J:1373", "J:1437", "J:1559", "J:1692", "J:1750", "J:2381", "J:1908", "J:2079",
                  "J:2195", "J:none")


def by_kind(group=None):
    out = {}
    for c in CASES:
        if group is None or c.group in group:
            out.setdefault(c.kind, []).append(c)
    return out


def site_counts():
    """{site: {side: cases}} over the guard cases."""
    out = {}
    for c in GUARD:
        for s in c.sites:
            d = out.setdefault(s, {"below": 0, "at": 0, "above": 0})
            d[c.side] += 1
    return out


_LOG_STARTED = False


def log(line):
    """sensitivity_ref.log's rule, into $EZPZ_PROFILE_DIR/edge_cases.txt: written only when that variable names a directory; the
    first line of a process starts the file anew."""
    import os

    global _LOG_STARTED
    out = os.environ.get("EZPZ_PROFILE_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "edge_cases.txt"), "a" if _LOG_STARTED else "w") as f:
            f.write(line + "\n")
        _LOG_STARTED = True
