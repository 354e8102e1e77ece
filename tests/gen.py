"""Seeded generators shared by the CPU and GPU test suites (distributions follow
/root/reference/ezpz/src/tests/proptests.rs:25-147)."""
import numpy as np

from oracle import oracle as O


def arb_ids(rng, k, hi=32):
    return [int(v) for v in rng.integers(0, hi, size=k)]


def arb_scalar(rng):
    return float(rng.integers(-1000, 1000)) / 10.0


def arb_angle_kind(rng, other_only=False):
    c = 2 if other_only else int(rng.integers(0, 3))
    if c == 0:
        return "parallel"
    if c == 1:
        return "perpendicular"
    return ("deg" if rng.integers(0, 2) else "rad", float(rng.integers(-360, 361)))


def arb_constraint(rng, kind, hi=32):
    """One random constraint of `kind` with ids drawn from [0, hi) (duplicates allowed, like arb_id())."""
    ids = arb_ids(rng, O.KIND_NUM_IDS[kind], hi)
    param, tag = 0.0, 0
    if kind == O.LINE_TANGENT_TO_CIRCLE:
        tag = int(rng.integers(1, 3))
    elif kind == O.CIRCLE_TANGENT_TO_CIRCLE:
        tag = int(rng.integers(1, 3))
    elif kind in (O.DISTANCE, O.VERTICAL_DISTANCE, O.HORIZONTAL_DISTANCE, O.FIXED, O.CIRCLE_RADIUS, O.ARC_RADIUS,
                  O.POINT_LINE_DISTANCE, O.VERTICAL_POINT_LINE_DISTANCE, O.HORIZONTAL_POINT_LINE_DISTANCE,
                  O.ARC_LENGTH):
        param = arb_scalar(rng)
    elif kind in (O.LINES_AT_ANGLE, O.POINTS_AT_ANGLE):
        tag, param = O._angle(arb_angle_kind(rng))
    elif kind == O.ARC_ANGLE:
        tag, param = O._angle(arb_angle_kind(rng, other_only=True))
    return O._mk(kind, ids, param, tag=tag)


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


from ezpz_amd.synthetic import keyed_uniform  # noqa: E402,F401  (the product's keyed PRNG; bench.py uses the same)


def connected_sketch(npts, seed):
    """One connected, fully determined component of mixed kinds: a random polyline-like sketch in which every point
    is tied to its predecessors by two scalar conditions consistent with a hidden true layout.  Returns the constraint
    records and guesses near the true layout."""
    rng = np.random.default_rng(seed)
    pt = lambda i: (2 * i, 2 * i + 1)
    cons = [O.fixed(0, 0.0), O.fixed(1, 0.0)]
    true = [np.zeros(2)]
    for i in range(1, npts):
        # a point is placed by two scalar conditions relative to earlier points, consistent with a hidden true layout
        p = true[-1] + rng.uniform(0.5, 2.0, 2) * rng.choice([-1.0, 1.0], 2)
        true.append(p)
        a = i - 1
        b = max(0, i - int(rng.integers(2, 4)))
        choice = int(rng.integers(0, 5))
        if choice == 0:
            cons += [O.horizontal_distance(pt(i), pt(a), float(p[0] - true[a][0])),
                     O.vertical_distance(pt(i), pt(a), float(p[1] - true[a][1]))]
        elif choice == 1:
            cons += [O.distance(pt(i), pt(a), float(np.hypot(*(p - true[a])))),
                     O.distance(pt(i), pt(b), float(np.hypot(*(p - true[b])))) if b != a else
                     O.horizontal_distance(pt(i), pt(a), float(p[0] - true[a][0]))]
        elif choice == 2:
            cons += [O.distance(pt(i), pt(a), float(np.hypot(*(p - true[a])))),
                     O.vertical_distance(pt(i), pt(a), float(p[1] - true[a][1]))]
        elif choice == 3:
            cons += [O.fixed(2 * i, float(p[0])), O.distance(pt(i), pt(a), float(np.hypot(*(p - true[a]))))]
        else:
            cons += [O.horizontal_distance(pt(i), pt(b), float(p[0] - true[b][0])),
                     O.distance(pt(i), pt(a), float(np.hypot(*(p - true[a]))))]
    recs = O.stack(cons)
    g = np.concatenate(true) + rng.uniform(-0.05, 0.05, 2 * npts)
    return recs, g


def graph_sketch(family, npts, rng):
    """A consistent, fully determined sketch of one of four graph families -- random tree with chords, wide band, hub,
    comb (a spine with teeth) -- built around a hidden true layout.  Returns the records and the true values."""
    pt = lambda i: (2 * i, 2 * i + 1)
    true = np.zeros((npts, 2))
    cons = [O.fixed(0, 0.0), O.fixed(1, 0.0)]
    for i in range(1, npts):
        if family == "tree":
            a, b = int(rng.integers(0, i)), int(rng.integers(0, i))
        elif family == "band":
            a, b = i - 1, max(0, i - int(rng.integers(2, 13)))
        elif family == "hub":
            a, b = 0, max(0, i - 1)
        else:  # comb
            a, b = (i - 1, max(0, i - 2)) if i % 5 else (max(0, i - 5), max(0, i - 10))
        true[i] = true[a] + rng.uniform(0.6, 2.0, 2) * rng.choice([-1.0, 1.0], 2)
        cons.append(O.distance(pt(i), pt(a), float(np.hypot(*(true[i] - true[a])))))
        if b != a:
            cons.append(O.distance(pt(i), pt(b), float(np.hypot(*(true[i] - true[b])))) if rng.random() < 0.5
                        else O.horizontal_distance(pt(i), pt(b), float(true[i][0] - true[b][0])))
        else:
            cons.append(O.vertical_distance(pt(i), pt(a), float(true[i][1] - true[a][1])))
    return O.stack(cons), true.reshape(-1)


def _rot(v, t):
    c, s = np.cos(t), np.sin(t)
    return np.asarray([c * v[0] - s * v[1], s * v[0] + c * v[1]])


def mixed_sketch(npts, seed):
    """connected_sketch(npts, 1000 + npts) at the oracle's solution (the true layout), with a decoration on every second point a
    (b = a + 1) that cycles through ten types consistent with that layout, so that all 13 kinds with a parameter occur -- the
    two-row ones (ArcRadius, ArcLength, PointsAtAngle) and both angle units among them; the tenth type is a second Distance at
    1.002 x the true length: inconsistent on purpose, so that weights change the answer.  Every weight is then drawn from
    default_rng(seed + 1).uniform(0.5, 2.0).  The sign of an angle and the parameter of a kind that subtracts it are read off
    the oracle's own residual at the true layout.  (mixed_sketch(40, 77): 118 variables, 116 constraints.)  Returns the records and
    the true values."""
    recs, g = connected_sketch(npts, 1000 + npts)
    rc, x, _, conv, _ = O.solve_batch(recs, g[None, :], O.Config(max_iterations=60, residual_tolerance=1e-12), linsolve=O.LINSOLVE_SPARSE)
    assert rc == 0 and conv[0]
    rng = np.random.default_rng(seed)
    vals = [float(v) for v in x[0]]
    cons = [recs[i] for i in range(len(recs))]
    pt = lambda i: (2 * i, 2 * i + 1)
    xy = lambda i: np.asarray(vals[2 * i: 2 * i + 2])

    def new_point(p):
        vals.extend([float(p[0]), float(p[1])])
        return (len(vals) - 2, len(vals) - 1)

    def subtracting(make):
        """make(param) of a kind whose residual is f(x) - param in every row: the parameter that makes it zero."""
        r, deg = O.residual(make(0.0), np.asarray(vals))
        assert not deg and np.ptp(r) <= 1e-9 * max(1.0, abs(r[0])), r
        cons.append(make(float(r[0])))

    def signed(make, value):
        for v in (value, -value):
            r, deg = O.residual(make(v), np.asarray(vals))
            if not deg and np.abs(r).max() < 1e-9:
                cons.append(make(v))
                return
        raise AssertionError("neither sign of the angle fits the layout")

    for n_dec, a in enumerate(range(0, npts - 1, 2)):
        b = a + 1
        pa, pb = xy(a), xy(b)
        u = pb - pa
        unit = "deg" if (n_dec // 10) % 2 == 0 else "rad"
        theta = float(rng.uniform(0.4, 1.2))
        angle = lambda t: (unit, float(np.degrees(t)) if unit == "deg" else t)
        kind = n_dec % 10
        if kind == 0:
            r = float(rng.uniform(0.5, 2.0))
            t0, t1 = np.radians(rng.uniform(15.0, 45.0)), np.radians(rng.uniform(135.0, 165.0))
            s = new_point(pa + r * np.asarray([np.cos(t0), np.sin(t0)]))
            e = new_point(pa + r * np.asarray([np.cos(t1), np.sin(t1)]))
            subtracting(lambda p: O.arc_radius(pt(a), s, e, p))
            subtracting(lambda p: O.vertical_distance(s, pt(a), p))
            subtracting(lambda p: O.vertical_distance(e, pt(a), p))
        elif kind == 1:
            e = new_point(pa + _rot(u, theta))
            signed(lambda p: O.arc_length(pt(a), pt(b), e, p), theta * float(np.hypot(*u)))
        elif kind == 2:
            q = new_point(pa + _rot(u, theta) * float(rng.uniform(0.6, 1.5)))
            signed(lambda p: O.points_at_angle(pt(a), pt(b), q, angle(p)), theta)
            subtracting(lambda p: O.distance(pt(a), q, p))
        elif kind == 3:
            q = new_point(pb + _rot(u, theta) * float(rng.uniform(0.6, 1.5)))
            signed(lambda p: O.lines_at_angle(pt(a), pt(b), pt(b), q, angle(p)), theta)
            subtracting(lambda p: O.distance(pt(b), q, p))
        elif kind == 4:
            q = new_point(pa + _rot(u, theta) * float(rng.uniform(0.6, 1.5)))
            signed(lambda p: O.arc_angle(pt(a), pt(b), q, angle(p)), theta)
            subtracting(lambda p: O.distance(pt(a), q, p))
        elif kind in (5, 6, 7):
            q = new_point(pa + _rot(u, theta) * float(rng.uniform(0.6, 1.5)))
            if kind == 5:
                subtracting(lambda p: O.point_line_distance(q, pt(a), pt(b), p))
                subtracting(lambda p: O.distance(q, pt(a), p))
            elif kind == 6:
                subtracting(lambda p: O.vertical_point_line_distance(q, pt(a), pt(b), p))
                subtracting(lambda p: O.horizontal_distance(q, pt(a), p))
            else:
                subtracting(lambda p: O.horizontal_point_line_distance(q, pt(a), pt(b), p))
                subtracting(lambda p: O.vertical_distance(q, pt(a), p))
        elif kind == 8:
            vals.append(float(rng.uniform(0.5, 2.0)))
            subtracting(lambda p: O.circle_radius(pt(a), len(vals) - 1, p))
        else:
            cons.append(O.distance(pt(a), pt(b), 1.002 * float(np.hypot(*u))))
    out = O.stack(cons)
    out["weight"] = np.random.default_rng(seed + 1).uniform(0.5, 2.0, len(out))
    return out, np.asarray(vals)


def linear_chain(npts):
    """Fixed, HorizontalDistance and VerticalDistance only (tests/test_gpu_front_params.py: test_linear_only_system)."""
    cons = [O.fixed(0, 0.5), O.fixed(1, -0.5)]
    for k in range(1, npts):
        a, b = (2 * (k - 1), 2 * k - 1), (2 * k, 2 * k + 1)
        cons += [O.horizontal_distance(b, a, 1.0 + 0.01 * k), O.vertical_distance(b, a, 0.5)]
    return O.stack(cons), np.zeros(2 * npts)
