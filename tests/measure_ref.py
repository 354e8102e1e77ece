"""Reference dimensions in numpy (include/ezpz_amd.h, "Reference dimensions"): the definition of m(record, x) as the
header's table has it, and the response, the stack-up and the vector-Jacobian product as sequential Python-float loops in the
orders the header states.  What the device computes is checked against these; these are checked against the ORACLE's residual
and Jacobian in tests/test_measure_cpu.py."""
import math

import numpy as np

from oracle import oracle as O

EPS = 1e-4
N_IDS = O.KIND_NUM_IDS
SUBTRACTING = (O.DISTANCE, O.VERTICAL_DISTANCE, O.HORIZONTAL_DISTANCE, O.FIXED, O.CIRCLE_RADIUS, O.ARC_RADIUS, O.POINT_LINE_DISTANCE,
               O.VERTICAL_POINT_LINE_DISTANCE, O.HORIZONTAL_POINT_LINE_DISTANCE)
CURVED = (O.ARC_LENGTH, O.LINES_AT_ANGLE, O.ARC_ANGLE, O.POINTS_AT_ANGLE)
ANGLES = (O.LINES_AT_ANGLE, O.ARC_ANGLE, O.POINTS_AT_ANGLE)
NO_LIBM = (O.FIXED, O.CIRCLE_RADIUS, O.VERTICAL_DISTANCE, O.HORIZONTAL_DISTANCE, O.VERTICAL_POINT_LINE_DISTANCE,
           O.HORIZONTAL_POINT_LINE_DISTANCE)  # the kinds whose evaluator calls no libm function: bitwise on host and device


def measurable(rec):
    k, t = int(rec["kind"]), int(rec["tag"])
    return k in SUBTRACTING or k == O.ARC_LENGTH or (k in ANGLES and t in (O.ANGLE_OTHER_DEG, O.ANGLE_OTHER_RAD))


def _theta(ux, uy, vx, vy):
    return math.atan2((ux * vy - uy * vx) + 0.0, ux * vx + uy * vy)  # (-pi, pi]: a cross product of -0.0 counts as +0.0


def measure_ref(rec, x):
    """(m, flags) of one record at the values x (indexed by the record's ids): bit 0 = the residual's guard."""
    k, t = int(rec["kind"]), int(rec["tag"])
    X = [float(x[int(i)]) for i in rec["ids"][: N_IDS[k]]]
    unit = 180.0 / math.pi if t == O.ANGLE_OTHER_DEG else 1.0
    if k == O.FIXED:
        return X[0], 0
    if k == O.CIRCLE_RADIUS:
        return X[2], 0
    if k == O.VERTICAL_DISTANCE:
        return X[1] - X[3], 0
    if k == O.HORIZONTAL_DISTANCE:
        return X[0] - X[2], 0
    if k == O.DISTANCE:
        return math.hypot(X[0] - X[2], X[1] - X[3]), 0
    if k == O.ARC_RADIUS:
        return (math.hypot(X[0] - X[2], X[1] - X[3]) + math.hypot(X[0] - X[4], X[1] - X[5])) / 2.0, 0
    if k == O.POINT_LINE_DISTANCE:
        px, py, lpx, lpy, lqx, lqy = X
        a, b, c = lpy - lqy, lqx - lpx, lpx * lqy - lqx * lpy
        den = math.hypot(a, b)
        return (0.0, 1) if den < EPS else ((a * px + b * py + c) / den, 0)
    if k in (O.VERTICAL_POINT_LINE_DISTANCE, O.HORIZONTAL_POINT_LINE_DISTANCE):
        ax, ay, px, py, qx, qy = X
        dx, dy = qx - px, qy - py
        if dx * dx + dy * dy <= EPS * EPS:
            return 0.0, 1
        if k == O.VERTICAL_POINT_LINE_DISTANCE:
            return (0.0, 1) if abs(dx) <= EPS else (ay - py - dy * (1.0 / dx) * (ax - px), 0)
        return (0.0, 1) if abs(dy) <= EPS else (ax - px - dx * (1.0 / dy) * (ay - py), 0)
    if k in ANGLES:
        if k == O.LINES_AT_ANGLE:
            ux, uy, vx, vy = X[2] - X[0], X[3] - X[1], X[6] - X[4], X[7] - X[5]
        else:
            ux, uy, vx, vy = X[2] - X[0], X[3] - X[1], X[4] - X[0], X[5] - X[1]
        if math.hypot(ux, uy) <= EPS or math.hypot(vx, vy) <= EPS:
            return 0.0, 1
        return _theta(ux, uy, vx, vy) * unit, 0
    if k == O.ARC_LENGTH:
        ux, uy, wx, wy = X[2] - X[0], X[3] - X[1], X[4] - X[0], X[5] - X[1]
        r2 = ux * ux + uy * uy
        if r2 <= EPS * EPS:
            return 0.0, 1
        phi = math.fmod(_theta(ux, uy, wx, wy), 2.0 * math.pi)
        if phi < 0.0:
            phi += 2.0 * math.pi
        return math.sqrt(r2) * phi, 0
    raise ValueError(f"kind {k} is not measurable")


def central_grad(rec, x, h):
    """Central differences of measure_ref by the record's ids, step h (a variable listed twice moves once)."""
    k = int(rec["kind"])
    x = np.asarray(x, dtype=np.float64)
    g = np.zeros(N_IDS[k])
    for s in range(N_IDS[k]):
        up, dn = x.copy(), x.copy()
        up[int(rec["ids"][s])] += h
        dn[int(rec["ids"][s])] -= h
        g[s] = (measure_ref(rec, up)[0] - measure_ref(rec, dn)[0]) / (2.0 * h)
    return g


def response_ref(recs, grad, S):
    """D [n_meas][n_param] of one system: grad [n_meas][8], S [n_param][n_vars]; (D, the sum of |terms|)."""
    D = np.zeros((len(recs), S.shape[0]))
    A = np.zeros_like(D)
    for i, rec in enumerate(recs):
        n_ids = N_IDS[int(rec["kind"])]
        for j in range(S.shape[0]):
            acc = float(grad[i][0]) * float(S[j][int(rec["ids"][0])])
            mag = abs(acc)
            for s in range(1, n_ids):
                term = float(grad[i][s]) * float(S[j][int(rec["ids"][s])])
                acc = acc + term
                mag += abs(term)
            D[i, j], A[i, j] = acc, mag
    return D, A


def worst_ref(D, tol):
    """(worst [n_meas], rss [n_meas]) of one system's D [n_meas][n_param]: ascending j from +0.0."""
    worst, rss = np.zeros(D.shape[0]), np.zeros(D.shape[0])
    for i in range(D.shape[0]):
        w, q = 0.0, 0.0
        for j in range(D.shape[1]):
            w = w + abs(float(D[i, j])) * float(tol[j])
            vt = float(D[i, j]) * float(tol[j])
            q = q + vt * vt
        worst[i], rss[i] = w, math.sqrt(q)
    return worst, rss


def vjp_ref(recs, grad, grad_m, n_vars):
    """grad_x [n_vars] of one system: ascending (i, slot) from +0.0; (grad_x, the sum of |terms|)."""
    gx, mag = [0.0] * n_vars, [0.0] * n_vars
    for i, rec in enumerate(recs):
        for s in range(N_IDS[int(rec["kind"])]):
            v = int(rec["ids"][s])
            term = float(grad_m[i]) * float(grad[i][s])
            gx[v] = gx[v] + term
            mag[v] += abs(term)
    return np.asarray(gx), np.asarray(mag)
