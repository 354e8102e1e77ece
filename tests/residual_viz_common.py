"""Shared by tests/test_residual_viz_cpu.py and tests/test_gpu_residual_viz.py: the five scenes of the reference's
residual_viz tests (ezpz/src/residual_viz.rs:536-580), the oracle evaluated per pixel, and the seeded scenes of all 25
kinds."""
import ctypes as C
import math
import os

import numpy as np

from oracle import oracle as O

BASELINES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "residual_viz_baselines")
VIEWPORT = (-5.0, 5.0, -5.0, 5.0, 256, 256)

# name -> (constraint, base values, example point, solution point: the reference's closed forms at these arguments)
_D = math.hypot(4.5, 3.0)
_A, _B, _C0 = -2.0 - 2.0, 4.0 - -4.0, -4.0 * 2.0 - 4.0 * -2.0
_DEN = math.hypot(_A, _B)
_ACT = (_A * -2.0 + _B * 5.0 + _C0) / _DEN
SCENES = {
    "points_coincident": (O.points_coincident((0, 1), (2, 3)), [0.0, 0.0, 0.0, 0.0], (3.0, 2.0), (0.0, 0.0)),
    "distance": (O.distance((0, 1), (2, 3), 3.0), [0.0, 0.0, 0.0, 0.0], (4.5, 3.0), (4.5 / _D * 3.0, 3.0 / _D * 3.0)),
    "point_line_distance": (O.point_line_distance((0, 1), (2, 3), (4, 5), 2.0), [0.0, 0.0, -4.0, -2.0, 4.0, 2.0], (-2.0, 5.0),
                            (-2.0 + _A / _DEN * (2.0 - _ACT), 5.0 + _B / _DEN * (2.0 - _ACT))),
    "vertical": (O.vertical((0, 1), (2, 3)), [0.0, 0.0, 0.0, 0.0], (3.0, 2.0), (0.0, 2.0)),
    "horizontal": (O.horizontal((0, 1), (2, 3)), [0.0, 0.0, 0.0, 0.0], (3.0, 2.0), (3.0, 0.0)),
}


def pixel_centres(viewport):
    """pixel_center_to_world (residual_viz.rs:58-62) in its operation order."""
    x_min, x_max, y_min, y_max, w, h = viewport
    xs = x_min + (x_max - x_min) * (np.arange(w, dtype=np.float64) + 0.5) / float(w)
    ys = y_min + (y_max - y_min) * (np.arange(h, dtype=np.float64) + 0.5) / float(h)
    return xs, ys


def oracle_magnitude(rec, values):
    """(magnitude, degenerate) of one constraint at one value vector: |r0|, or sqrt(r0*r0 + r1*r1) for two rows."""
    a = O.stack([rec])
    r = np.zeros(3)
    deg = C.c_int(0)
    O.lib().orc_residual(a.ctypes.data, values.ctypes.data, r.ctypes.data, C.byref(deg))
    if O.lib().orc_residual_dim(a.ctypes.data) == 1:
        return abs(r[0]), bool(deg.value)
    return math.sqrt(r[0] * r[0] + r[1] * r[1]), bool(deg.value)


def oracle_field(rec, x_base, var_x, var_y, viewport):
    """The oracle's field: (mag (H, W), degenerate (H, W) bool)."""
    xs, ys = pixel_centres(viewport)
    v = np.array(x_base, dtype=np.float64)
    mag = np.zeros((len(ys), len(xs)))
    deg = np.zeros((len(ys), len(xs)), bool)
    for r, y in enumerate(ys):
        v[var_y] = y
        for c, x in enumerate(xs):
            v[var_x] = x
            mag[r, c], deg[r, c] = oracle_magnitude(rec, v)
    return mag, deg


BAR = 1e-11  # relative to max(1, |want|): what tests/test_gpu_parity.py holds device residuals to


def moves_under_one_ulp(rec, x_base, var_x, var_y, x, y, want):
    """Whether the oracle's own magnitude at (x, y) moves by more than the bar when a swept coordinate moves by one ulp:
    a discontinuity of the kind (an angle wrap, a guard), where two correct evaluators may disagree."""
    v = np.array(x_base, dtype=np.float64)
    bar = BAR * max(1.0, abs(want))
    for nx, ny in ((np.nextafter(x, np.inf), y), (np.nextafter(x, -np.inf), y), (x, np.nextafter(y, np.inf)), (x, np.nextafter(y, -np.inf))):
        v[var_x], v[var_y] = nx, ny
        m, _ = oracle_magnitude(rec, v)
        if not abs(m - want) <= bar:
            return True
    return False


KIND_VIEW = (64, 48)  # width, height of the per-kind scenes


def kind_scene(kind, seed=20240607):
    """One constraint of `kind` on distinct ids 0 .. n_ids - 1, seeded base values, and a 64x48 viewport of 4 x 3 units around
    the swept point (ids 0 and 1: two of the constraint's own, except Fixed, which has one).  Returns
    (record, x_base, var_x, var_y, viewport)."""
    rng = np.random.default_rng(seed + 1000 * kind)
    n_ids = O.KIND_NUM_IDS[kind]
    ids = list(range(n_ids))
    param, tag = 0.0, 0
    if kind in (O.LINE_TANGENT_TO_CIRCLE, O.CIRCLE_TANGENT_TO_CIRCLE):
        tag = int(rng.integers(1, 3))
    elif kind in (O.LINES_AT_ANGLE, O.POINTS_AT_ANGLE, O.ARC_ANGLE):
        tag, param = O._angle(("deg" if rng.integers(0, 2) else "rad", float(rng.integers(-360, 361))))
    elif kind not in (O.DISTANCE_VAR, O.VERTICAL, O.HORIZONTAL, O.SCALAR_EQUAL, O.POINTS_COINCIDENT, O.LINES_EQUAL_LENGTH, O.ARC,
                      O.MIDPOINT, O.SYMMETRIC, O.POINT_ARC_COINCIDENT):
        param = float(rng.uniform(0.5, 3.0))
    rec = O._mk(kind, ids, param, tag=tag)
    n_vars = max(n_ids, 2)
    x_base = rng.uniform(-3.0, 3.0, n_vars)
    w, h = KIND_VIEW
    viewport = (float(x_base[0] - 2.0), float(x_base[0] + 2.0), float(x_base[1] - 1.5), float(x_base[1] + 1.5), w, h)
    return rec, x_base, 0, 1, viewport
