"""The synthetic samples and edges tests/test_effects_cpu.py and tests/test_gpu_effects.py share: every cause of a sample that
does not count (those of test_gpu_contributors.samples_of: ok = 0, flag bit 0, NaN, +inf) and every special place of an edge -- a
value exactly on one, an edge at -0.0 beside values of both zeros, a dimension whose edges are all +inf, a bin that stays empty --
with the reference's answer computed once per shape."""
import numpy as np

import effects_ref as R

SHAPES = [(k, m, B, s) for (k, m, B) in ((1, 1, 2), (2, 1, 4)) for s in (1, 255, 256, 257, 1000)] + [(8, 8, 64, 257), (32, 32, 4, 257)]
_CACHE = {}


def case(k, m, B, samples):
    """(params, m, flags, ok, nominal_m, edges)."""
    key = ("case", k, m, B, samples)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(100000 * k + 1000 * m + 10 * samples + B)
    nominal_p, nominal_m = rng.uniform(-5.0, 5.0, k), rng.uniform(-5.0, 5.0, m)
    scale = rng.uniform(0.01, 0.3, k)
    if k >= 2:
        nominal_p[k - 1] = 0.0  # (the last dimension straddles zero)
    p = nominal_p + rng.normal(size=(samples, k)) * scale
    if k >= 2 and samples >= 3:
        p[1, k - 1], p[2, k - 1] = 0.0, -0.0
    A = rng.normal(size=(m, k))
    y = nominal_m + (p - nominal_p) @ A.T + 0.05 * rng.normal(size=(samples, m)) + ((p - nominal_p) ** 2) @ np.abs(A.T)
    flags = (rng.integers(0, 2, (samples, m)) * 2).astype(np.uint8)  # (bit 1: not the guard's)
    ok = np.ones(samples, np.uint8)
    for b in range(samples):
        cause, i = b % 11, b % m  # (causes 4 .. 10: a sample that counts)
        if cause == 0:
            ok[b] = 0
        elif cause == 1:
            flags[b, i] |= 1
        elif cause == 2:
            y[b, i] = np.nan
        elif cause == 3:
            y[b, i] = np.inf
    edges = nominal_p[:, None] + scale[:, None] * np.linspace(-1.2, 1.2, B - 1)[None, :]
    # dimension 0: its first edge is a drawn value itself (which goes to the upper bin); with three bins or more the second edge
    # repeats the first, and bin 1 stays empty
    on = p[min(5, samples - 1), 0]
    edges[0] = on + scale[0] * np.linspace(0.0, 1.5, B - 1)
    if B >= 3:
        edges[0, 1] = edges[0, 0]
    if k >= 2:  # the last dimension: an edge at -0.0, the rest +inf
        edges[k - 1] = np.inf
        edges[k - 1, 0] = -0.0
    if k >= 3:  # a dimension in one bin
        edges[1] = np.inf
    _CACHE[key] = (p, y, flags, ok, nominal_m, edges)
    return _CACHE[key]


def reference(k, m, B, samples):
    key = ("ref", k, m, B, samples)
    if key not in _CACHE:
        _CACHE[key] = R.effects(*case(k, m, B, samples))
    return _CACHE[key]
