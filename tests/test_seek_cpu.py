"""Dimension targets, what can be checked without a device: the host entry ezpz_seek_step against the reference restated from the
header (tests/seek_ref.py) on seeded random cases, the hold rule and the step's end tests at their exact thresholds, a step that
solves a linear problem exactly, the symbols with their layouts and defaults, and the step's argument errors.

Bars.  Everything about a step is bytes: it is made of + - * /, comparisons and fabs in an order the header fixes, none
contracted, and Python floats are the same IEEE doubles.  The linear problem's answer: 1e-9 -- the damping mu = 1e-12 perturbs the solution
of the normal equations by at most mu * cond(A) relative (every diagonal entry is raised by at most mu * amax), cond(A) is asserted
below 1e3 for the matrix used, and rounding is far below that."""
import ctypes as C
import math
import os

import numpy as np

import ezpz_amd as E
import seek_ref as R
from ezpz_amd._lib import EXPORTS, CSeekConfig

ERR_INVALID_ARGUMENT, ERR_TOO_LARGE = -103, -102
KINDS = {"TRIAL": R.TRIAL, "MINIMUM": R.STEP_MINIMUM, "PIVOT": R.PIVOT}


def both(p, m, D, t, mu, **policy):
    """(the library's step, the reference's) with the kinds as numbers."""
    cfg = E.SeekConfig(**{k: v for k, v in policy.items()})
    kind, pt, delta, held = E.seek_step(p, m, D, t, mu, cfg)
    pol = R.Policy(len(p), len(m), **policy)
    return (KINDS[kind], pt, delta, held), R.step(p, m, np.asarray(D, dtype=np.float64).reshape(len(m), len(p)), t, pol, mu)


def assert_same(got, want, what=""):
    assert got[0] == want[0], (what, got, want)
    assert got[1].tobytes() == np.array(want[1], dtype=np.float64).tobytes(), (what, got, want)
    assert got[2].tobytes() == np.array(want[2], dtype=np.float64).tobytes(), (what, got, want)
    assert got[3] == want[3], (what, got, want)


def random_case(rng, case):
    """A step's inputs: the shapes sweep n_param 1 .. 16 and n_meas 1 .. 64; the flavour by `case`."""
    n = 1 + case % 16
    k = [1, 2, n, 64, int(rng.integers(1, 65))][(case // 16) % 5]
    D = rng.normal(size=(k, n))
    flavour = case % 11
    scale = 10.0 ** rng.uniform(-3, 3, n) if case % 3 == 0 else np.ones(n)
    weight = rng.uniform(0.2, 3.0, k)
    p = rng.normal(size=n) * 3.0
    lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
    mu = 10.0 ** rng.uniform(-12, 12)
    if flavour == 1:  # a zero column
        D[:, rng.integers(n)] = 0.0
    if flavour == 2 and n > 1:  # a duplicated column: singular without the damping
        a, b = rng.choice(n, 2, replace=False)
        D[:, a] = D[:, b]
        mu = [1e-12, 1e-3, 1.0][case % 3]
    if flavour == 3:  # zero weights
        weight[rng.random(k) < 0.5] = 0.0
    if flavour in (4, 5, 6):  # bounds: on them from either side, frozen, or just ahead
        for r in range(n):
            u = rng.random()
            if u < 0.25:
                lo[r] = p[r]
            elif u < 0.5:
                hi[r] = p[r]
            elif u < 0.65:
                lo[r] = hi[r] = p[r]
            elif u < 0.8:
                lo[r], hi[r] = p[r] - 10.0 ** rng.uniform(-6, 0), p[r] + 10.0 ** rng.uniform(-6, 0)
    if flavour == 7:  # a pivot that fails: a column that overflows the normal matrix, or cancels in it
        D[:, rng.integers(n)] *= 1e160
    if flavour == 8:  # a non-finite entry
        D[rng.integers(k), rng.integers(n)] = [np.nan, np.inf, -np.inf][case % 3]
    if flavour == 9:  # all zero: nothing to learn from D
        D[:] = 0.0
    m = rng.normal(size=k)
    t = m + rng.normal(size=k) * 10.0 ** rng.uniform(-8, 1)
    return p, m, D, t, mu, dict(weight=weight, lo=lo, hi=hi, scale=scale)


def test_step_is_the_reference_bytes():
    rng = np.random.default_rng(20261020)
    kinds, held_seen, sizes = [0, 0, 0], 0, set()
    for case in range(2200):
        p, m, D, t, mu, policy = random_case(rng, case)
        got, want = both(p, m, D, t, mu, **policy)
        assert_same(got, want, case)
        kinds[got[0]] += 1
        held_seen += got[3] != 0
        sizes.add((len(p), len(m)))
    # the cases reach every outcome, and every n_param with the ends of n_meas
    assert min(kinds) >= 50 and held_seen >= 200, (kinds, held_seen)
    assert {n for n, _ in sizes} == set(range(1, 17)) and {1, 64} <= {k for _, k in sizes}


def test_a_failed_pivot_and_a_non_finite_entry():
    # two equal columns and (almost) no damping: the second pivot cancels to zero or below
    D = np.array([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]])
    got, want = both([0.0, 0.0], [0.0, 0.0, 0.0], D, [1.0, 2.0, 3.0], 1e-30)
    assert_same(got, want)
    assert got[0] == R.PIVOT and got[1].tobytes() == np.zeros(2).tobytes() and got[2].tobytes() == np.zeros(2).tobytes()
    for bad in (np.nan, np.inf):
        D2 = np.array([[1.0, 0.5], [bad, 2.0]])
        got, want = both([0.0, 0.0], [0.0, 0.0], D2, [1.0, 2.0], 1e-3)
        assert_same(got, want)
        assert got[0] == R.PIVOT


def test_hold_rule_at_its_thresholds():
    # one dimension, one record, D = 1: g = t - m.  On the lower bound, a gradient that points outside holds it ...
    for bound, sign, held in (("lo", -1.0, True), ("lo", 1.0, False), ("hi", 1.0, True), ("hi", -1.0, False)):
        policy = {bound: [2.0]}
        got, want = both([2.0], [0.0], [[1.0]], [sign], 1e-3, **policy)
        assert_same(got, want, (bound, sign))
        assert (got[3] == 1) == held and (got[0] == R.STEP_MINIMUM) == held, (bound, sign, got)
    # ... a zero gradient does not (nothing to hold against), and one ulp inside the bound is free
    got, want = both([2.0], [0.0], [[1.0]], [0.0], 1e-3, lo=[2.0])
    assert_same(got, want)
    assert got[3] == 0 and got[0] == R.STEP_MINIMUM  # (free, and the step is zero)
    got, want = both([np.nextafter(2.0, 3.0)], [0.0], [[1.0]], [-1.0], 1e-3, lo=[2.0])
    assert_same(got, want)
    assert got[3] == 0 and got[0] == R.TRIAL and got[1][0] == 2.0  # clamped onto the bound
    # lo == hi freezes whatever the gradient says
    got, want = both([2.0, 1.0], [0.0], [[1.0, 1.0]], [1.0], 1e-3, lo=[2.0, -np.inf], hi=[2.0, np.inf])
    assert_same(got, want)
    assert got[3] == 1 and got[1][0] == 2.0 and got[2][0] == 0.0 and got[1][1] > 1.0


def test_end_test_at_its_threshold():
    # delta = (t - m) / (1 + mu) with D = 1, scale = 1; p = 0: MINIMUM iff |delta| <= step_tol^2
    step_tol, mu = 2.0 ** -20, 2.0 ** -1
    bar = step_tol * (0.0 + step_tol)
    for dev, kind in ((bar * 1.5, R.STEP_MINIMUM), (np.nextafter(bar * 1.5, 1.0), R.TRIAL)):
        got, want = both([0.0], [0.0], [[1.0]], [dev], mu, step_tol=step_tol)
        assert_same(got, want, dev)
        assert got[0] == kind and (got[2][0] <= bar) == (kind == R.STEP_MINIMUM), (dev, got)
    # a step that the clamp takes back entirely: p_trial == p although the dimension was free (it was not ON the bound's far side)
    got, want = both([1.0], [0.0], [[1.0]], [1e-30], 1e-3, step_tol=0.0)
    assert_same(got, want)
    assert got[0] == R.STEP_MINIMUM and got[2][0] != 0.0 and got[1][0] == 1.0  # 1 + 1e-30 == 1


def test_a_linear_problem_is_solved_in_one_step():
    rng = np.random.default_rng(5)
    D = rng.normal(size=(6, 3)) + np.eye(6, 3) * 3.0
    p, want_p = rng.normal(size=3), rng.normal(size=3)
    m = D @ p
    assert np.linalg.cond(D.T @ D) < 1e3
    kind, pt, delta, held = E.seek_step(p, m, D, D @ want_p, 1e-12, E.SeekConfig())
    assert kind == "TRIAL" and held == 0
    assert np.allclose(pt, want_p, rtol=1e-9, atol=1e-9) and np.array_equal(pt, p + delta)


def test_symbols_layouts_defaults_and_errors():
    L = E.lib()
    for name in ("ezpz_default_seek_config", "ezpz_seek_step", "ezpz_system_seek_targets", "ezpz_system_seek_targets_device"):
        assert name in EXPORTS and hasattr(L, name)
    c = CSeekConfig()
    L.ezpz_default_seek_config(C.byref(c))
    assert [c.weight, c.tol, c.lo, c.hi, c.scale] == [None] * 5
    assert (c.max_iterations, c.chunk, c.mu0, c.mu_up, c.mu_down, c.mu_min, c.mu_max, c.step_tol) == (40, 0, 1e-3, 10.0, 0.1, 1e-12, 1e12, 1e-12)
    assert c.sens_lambda == c.inner.initial_lambda == 1e-9 and c.inner.max_iterations == 35
    d = E.SeekConfig()._c(3, 2)[0]
    assert bytes(c) == bytes(d)  # the Python defaults are the library's
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ezpz_amd.h")).read()
    assert "POLICY DEFAULTS, not measurements" in header and "EzpzSeekInfo { /* one per system; 48 bytes */" in header

    def rc(n, k, mu=1e-3, **policy):
        try:
            E.seek_step(np.zeros(n), np.zeros(k), np.ones((k, n)), np.ones(k), mu, E.SeekConfig(**policy))
        except E.NonLinearSystemError as e:
            return e.code
        return 0

    assert rc(2, 2) == 0
    assert rc(17, 2) == ERR_TOO_LARGE and rc(2, 65) == ERR_TOO_LARGE
    for policy in (dict(lo=[1.0, 0.0], hi=[0.0, 1.0]), dict(lo=[math.nan, 0.0]), dict(weight=[-1.0, 1.0]), dict(weight=[math.inf, 1.0]),
                   dict(tol=[-1e-6, 1.0]), dict(tol=[math.nan, 1.0]), dict(scale=[0.0, 1.0]), dict(scale=[math.inf, 1.0]),
                   dict(scale=[-1.0, 1.0]), dict(mu_up=1.0), dict(mu_down=1.0), dict(mu_down=0.0), dict(mu_min=0.0),
                   dict(mu0=1e13), dict(mu0=1e-13), dict(step_tol=-1.0), dict(sens_lambda=math.nan)):
        assert rc(2, 2, **policy) == ERR_INVALID_ARGUMENT, policy
    assert L.ezpz_seek_step(2, 2, None, None, None, None, None, 1e-3, None, None, None) == ERR_INVALID_ARGUMENT
