"""Tolerance contributors, what can be checked without a device: the closing step (ezpz_mc_contributors, host only) against
tests/contrib_ref.py bit for bit, its meaning against numpy's least squares and covariance, exactly linear data, and the ABI -- the
symbols with their signatures and layouts, the defaults, every argument error by its return code.

Bars.  The closing step against the restatement: bytes.  Against numpy.linalg.lstsq (with an intercept) and numpy.cov: 1e-9 of the
largest magnitude of the array compared.  Derivation: the inputs are independent uniform draws, so the input block of the
covariance is close to diagonal with a condition number below 10 (the variances differ by less than 9x; asserted); the normal
equations then lose about cond x epsilon x sqrt(samples) ~ 1e-13 at worst, and forming the centred moments from raw sums of
deviations from the nominal (|mean| <= the spread) loses no more.  1e-9 leaves some four to five digits of margin; numpy's own
normal-equations route is held to the same bar against lstsq in the same test.  Exactly linear data: r2 = 1 to 1e-12 (the same
error model, two more digits of margin than needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import contrib_ref as R
import ezpz_amd as E
from ezpz_amd._lib import EXPORTS, CMcContribConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARGUMENT, ERR_NO_DEVICE = -103, -100

RUN_ARGS = ["sys", "x0", "positions", "n_param", "dist", "nominal", "records", "n_meas", "lim_lo", "lim_hi", "hist_lo", "hist_hi", "samples",
            "mc", "cfg", "stats", "totals", "hist", "keep_params", "keep_m", "keep_flags", "keep_ok", "cc", "moments", "info", "cov", "beta",
            "contrib", "r2", "dropped"]
RUN_ARGS_DEV = ["sys", "x0_dev", "positions", "n_param", "dist", "nominal", "records", "n_meas", "lim_lo", "lim_hi", "hist_lo", "hist_hi",
                "samples", "mc", "cfg", "stats_dev", "totals_dev", "hist_dev", "keep_params_dev", "keep_m_dev", "keep_flags_dev", "keep_ok_dev",
                "cc", "moments_dev", "info_dev", "cov_dev", "beta_dev", "contrib_dev", "r2_dev", "dropped_dev", "stream"]
SIGNATURES = {
    "ezpz_mc_contributors": ["moments", "n_complete", "n_param", "n_meas", "cc", "cov", "beta", "contrib", "r2", "dropped"],
    "ezpz_mc_moments": ["params", "m", "flags", "ok", "nominal_p", "nominal_m", "samples", "n_param", "n_meas", "chunk", "moments", "info"],
    "ezpz_mc_moments_device": ["params_dev", "m_dev", "flags_dev", "ok_dev", "nominal_p_dev", "nominal_m_dev", "samples", "n_param", "n_meas",
                               "chunk", "moments_dev", "info_dev", "stream"],
    "ezpz_system_tolerance_mc_contrib": RUN_ARGS,
    "ezpz_system_tolerance_mc_contrib_device": RUN_ARGS_DEV,
}


def test_symbols_signatures_layouts_and_defaults():
    L = E.lib()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ezpz_amd.h")).read())
    for name, params in SIGNATURES.items():
        assert name in EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(params), name
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl, name
        assert [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")] == params, name
    assert "ezpz_default_mc_contrib_config" in EXPORTS and re.search(r"void ezpz_default_mc_contrib_config\(EzpzMcContribConfig\* cc\);", header)
    for text in ("typedef struct EzpzMcContribConfig { /* 16 bytes */", "typedef struct EzpzMcMomentsInfo { /* 16 bytes */",
                 "#define EZPZ_MC_MOMENT_MAX 64u"):
        assert text in header, text
    assert C.sizeof(CMcContribConfig) == 16 and E.MC_MOMENTS_INFO_DTYPE.itemsize == 16 and R.MOMENT_MAX == 64
    assert E.MC_MOMENTS_INFO_DTYPE.names == ("samples", "n_complete")
    cc = CMcContribConfig(7.0, 7)
    L.ezpz_default_mc_contrib_config(C.byref(cc))
    assert (cc.pivot_rel, cc.reserved) == (2.0 ** -26, 0)
    assert callable(E.mc_moments) and callable(E.mc_contributors) and isinstance(E.McResult.corr, property)
    import inspect

    for method in (E.System.tolerance_mc, E.System.tolerance_mc_device):
        assert "pivot_rel" in inspect.signature(method).parameters
    assert inspect.signature(E.System.tolerance_mc).parameters["contributors"].default is False


# ---- the closing step against the restatement, bytes ------------------------------------------------------------------------------
def raw_moments(z):
    """moments of complete samples z [n, K] by numpy's sums: the closing step takes whatever sums it is given."""
    K = z.shape[1]
    G = z.T @ z
    return np.concatenate([z.sum(axis=0), np.concatenate([G[a, a:] for a in range(K)])])


def degenerate_samples(k, m, n, seed):
    """z [n, k + m] of random samples with what the shape has room for: dimension 1 FIXED, dimension 2 a copy of dimension 0, the
    last reference dimension constant; the others respond linearly with a little curvature."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (n, k)) * rng.uniform(0.05, 0.3, k)
    if k >= 3:
        p[:, 1] = 0.0
        p[:, 2] = p[:, 0]
    A = rng.normal(size=(m, k))
    y = p @ A.T + 0.3 * (p * p) @ np.abs(A).T + 0.01 * rng.normal(size=(n, m))
    if m >= 2:
        y[:, -1] = 0.0
    return np.concatenate([p, y], axis=1)


def assert_closing_step_is_the_reference(mom, n_complete, k, m, pivot_rel=None):
    got = E.mc_contributors(mom, n_complete, k, m, pivot_rel)
    cov, beta, contrib, r2, dropped = R.contributors(mom, n_complete, k, m, *(() if pivot_rel is None else (pivot_rel,)))
    for name, want in (("cov", cov), ("beta", beta), ("contrib", contrib), ("r2", r2)):
        assert getattr(got, name).tobytes() == want.tobytes(), (name, k, m, n_complete, getattr(got, name), want)
    assert got.dropped == dropped
    return got


@pytest.mark.parametrize("k,m", [(0, 1), (1, 1), (3, 2), (32, 32)])
def test_closing_step_is_the_restatement_bit_for_bit(k, m):
    z = degenerate_samples(k, m, 500, 100 * k + m)
    got = assert_closing_step_is_the_reference(raw_moments(z), 500, k, m)
    assert got.cov.tobytes() == got.cov.T.copy().tobytes()
    if k >= 3:
        assert got.dropped == 0b110 and got.dropped_mask.tolist() == [False, True, True] + [False] * (k - 3)  # FIXED; the later of two equals
        assert not got.beta[:, 1:3].any() and np.all(got.beta[:-1, 0] != 0.0)
        assert not got.contrib[:-1, 1:3].any()
    else:
        assert got.dropped == 0
    if m >= 2:  # the constant reference dimension
        assert np.isnan(got.r2[-1]) and np.isnan(got.contrib[-1]).all() and np.isfinite(got.r2[:-1]).all()
        assert np.all(got.r2[:-1] > 0.9) and np.all(got.r2[:-1] <= 1.0 + 1e-12)
    # other thresholds: 0 keeps whatever has a positive pivot, one half drops what an earlier dimension half explains
    assert_closing_step_is_the_reference(raw_moments(z), 500, k, m, 0.0)
    assert_closing_step_is_the_reference(raw_moments(z), 500, k, m, 0.5)
    # n_complete of 0, 1 and 2
    for n in (0, 1):
        few = assert_closing_step_is_the_reference(raw_moments(z[:n]), n, k, m)
        assert few.dropped == R.UINT64_MAX and all(np.isnan(a).all() for a in (few.cov, few.beta, few.contrib, few.r2))
    two = assert_closing_step_is_the_reference(raw_moments(z[:2]), 2, k, m)
    assert np.isfinite(two.cov).all() and two.dropped != R.UINT64_MAX
    if k >= 3:  # two samples span one direction: every input behind the first is a combination of it
        assert two.dropped == (1 << k) - 2


def test_a_fixed_single_dimension_is_dropped():
    z = degenerate_samples(1, 1, 100, 5)
    z[:, 0] = 0.0
    got = assert_closing_step_is_the_reference(raw_moments(z), 100, 1, 1)
    assert got.dropped == 1 and got.beta.tolist() == [[0.0]] and got.contrib.tolist() == [[0.0]] and got.r2.tolist() == [0.0]


# ---- the meaning: numpy's least squares and covariance -------------------------------------------------------------------------------
def close(got, want, bar):
    return np.max(np.abs(got - want)) <= bar * np.max(np.abs(want))


def synthetic(seed, quadratic):
    rng = np.random.default_rng(seed)
    k, m, n = 5, 3, 4096
    half = np.array([0.1, 0.15, 0.2, 0.25, 0.3])
    nominal_p = np.array([10.0, -3.0, 0.5, 7.0, 2.0])
    p = nominal_p + rng.uniform(-1.0, 1.0, (n, k)) * half
    A = np.array([[1.0, -1.0, 0.0, 0.5, 2.0], [0.0, 3.0, 1.0, -2.0, 0.25], [1.5, 0.0, 0.0, 0.0, -1.0]])
    c = np.array([4.0, -1.0, 0.0])
    y = p @ A.T + c + quadratic * ((p - nominal_p) ** 2) @ np.abs(A).T
    nominal_m = nominal_p @ A.T + c
    return k, m, n, p, y, nominal_p, nominal_m


def test_meaning_against_lstsq_and_cov():
    k, m, n, p, y, nominal_p, nominal_m = synthetic(2026, 0.5)
    z = np.concatenate([p - nominal_p, y - nominal_m], axis=1)
    got = E.mc_contributors(raw_moments(z), n, k, m)
    assert got.dropped == 0
    cov = np.cov(np.concatenate([p, y], axis=1).T)
    assert np.linalg.cond(cov[:k, :k]) < 10.0
    X = np.concatenate([p, np.ones((n, 1))], axis=1)
    coef, *_ = np.linalg.lstsq(X, y, rcond=None)
    beta = coef[:k].T
    r2 = 1.0 - ((y - X @ coef) ** 2).sum(axis=0) / ((y - y.mean(axis=0)) ** 2).sum(axis=0)
    # numpy's own normal-equations route stays inside the bar: the bar is about the method, not about this library
    assert close(np.linalg.solve(cov[:k, :k], cov[:k, k:]).T, beta, 1e-9)
    assert close(got.cov, cov, 1e-9) and close(got.beta, beta, 1e-9) and close(got.r2, r2, 1e-9)
    assert np.all(got.r2 < 1.0 - 1e-6) and np.all(got.r2 > 0.99)  # (the curvature is seen, and is small)
    assert close(got.corr, np.corrcoef(np.concatenate([p, y], axis=1).T), 1e-9)
    assert close(got.contrib, beta * beta * np.diag(cov)[:k] / np.diag(cov)[k:, None], 1e-9)


def test_exactly_linear_data():
    # values on a grid of 2^-10 and coefficients that are small integers or halves: m is exactly linear in p, to the last bit
    rng = np.random.default_rng(7)
    k, m, n = 4, 2, 1000
    p = rng.integers(-512, 513, (n, k)) / 1024.0
    A = np.array([[1.0, -2.0, 0.5, 3.0], [0.0, 1.0, 1.0, -0.5]])
    y = p @ A.T
    z = np.concatenate([p, y], axis=1)
    got = E.mc_contributors(raw_moments(z), n, k, m)
    assert got.dropped == 0 and np.all(np.abs(got.r2 - 1.0) <= 1e-12) and np.all(np.abs(got.beta - A) <= 1e-12 * np.abs(A).max())
    # the header's identity: r2 - sum_j contrib = sum_{j != l} beta_j beta_l cov[j][l] / var(m)
    cpp, vm = got.cov[:k, :k], np.diag(got.cov)[k:]
    cross = np.array([sum(got.beta[i, j] * got.beta[i, l] * cpp[j, l] for j in range(k) for l in range(k) if j != l) for i in range(m)]) / vm
    assert np.all(np.abs(got.r2 - got.contrib.sum(axis=1) - cross) <= 1e-12)
    assert np.all(np.abs(cross) > 1e-6)  # (the term is there: independent draws are uncorrelated only to 1 / sqrt(n))
    assert np.all(np.abs(cross) < 0.2)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def _contributors_rc(n_param, n_meas, pivot_rel=2.0 ** -26, moments=True, missing=None):
    K = min(n_param + n_meas, 130)  # (the buffers of a request that is declined are never touched, whatever it asks for)
    out = {"cov": np.full(K * K + 1, 7.0), "beta": np.full(K * K + 1, 7.0), "contrib": np.full(K * K + 1, 7.0), "r2": np.full(K + 1, 7.0),
           "dropped": np.full(1, 7, np.uint64)}
    mom = np.ones(R.entries(K) + 1)
    cc = CMcContribConfig(pivot_rel, 0)
    rc = E.lib().ezpz_mc_contributors(mom.ctypes.data if moments else None, 10, n_param, n_meas, C.byref(cc),
                                      *(None if name == missing else a.ctypes.data for name, a in out.items()))
    return rc, all(np.all(a == 7) for a in out.values())


def test_closing_step_argument_errors():
    assert _contributors_rc(2, 2) == (0, False)
    for bad in (dict(n_param=0, n_meas=0), dict(n_param=33, n_meas=32), dict(n_param=65, n_meas=0), dict(n_param=0, n_meas=65),
                dict(n_param=2 ** 63, n_meas=2 ** 63), dict(n_param=2, n_meas=2, pivot_rel=-1e-30), dict(n_param=2, n_meas=2, pivot_rel=np.nan),
                dict(n_param=2, n_meas=2, pivot_rel=np.inf), dict(n_param=2, n_meas=2, moments=False), dict(n_param=2, n_meas=2, missing="cov"),
                dict(n_param=2, n_meas=2, missing="beta"), dict(n_param=2, n_meas=2, missing="contrib"), dict(n_param=2, n_meas=2, missing="r2"),
                dict(n_param=2, n_meas=2, missing="dropped")):
        assert _contributors_rc(**bad) == (ERR_INVALID_ARGUMENT, True), bad
    # K = 64 is legal, and so are absent outputs that have no elements
    assert _contributors_rc(32, 32)[0] == 0 and _contributors_rc(64, 0, missing="r2")[0] == 0 and _contributors_rc(0, 3, missing="beta")[0] == 0
    with pytest.raises(ValueError):
        E.mc_contributors(np.zeros(4), 10, 1, 1)
    with pytest.raises(E.NonLinearSystemError):
        E.mc_contributors(np.zeros(5), 10, 2, 0, pivot_rel=-1.0)


def _moments_rc(samples=4, n_param=2, n_meas=1, missing=None, device=False):
    k, m = min(n_param, 65) + 1, min(n_meas, 65) + 1  # (as above: a declined request touches nothing)
    a = {"params": np.zeros((4, k)), "m": np.zeros((4, m)), "flags": np.zeros((4, m), np.uint8), "ok": np.ones(4, np.uint8),
         "nominal_p": np.zeros(k), "nominal_m": np.zeros(m)}
    out = {"moments": np.full(R.entries(k + m), 7.0), "info": np.full(2, 7, np.uint64)}
    ptr = lambda name, v: None if name == missing else v.ctypes.data  # noqa: E731
    args = [ptr(n, v) for n, v in a.items()] + [samples, n_param, n_meas, 0] + [ptr(n, v) for n, v in out.items()]
    fn = E.lib().ezpz_mc_moments_device if device else E.lib().ezpz_mc_moments
    rc = fn(*args, *([None] if device else []))
    return rc, all(np.all(v == 7) for v in out.values())


def test_moments_argument_errors_come_before_the_device():
    for device in (False, True):
        for bad in (dict(n_param=0, n_meas=0), dict(n_param=64, n_meas=1), dict(n_param=2 ** 63, n_meas=2 ** 63), dict(missing="params"),
                    dict(missing="m"), dict(missing="nominal_p"), dict(missing="nominal_m"), dict(missing="moments"), dict(missing="info")):
            assert _moments_rc(device=device, **bad) == (ERR_INVALID_ARGUMENT, True), (device, bad)
        # samples == 0: EZPZ_OK, nothing written -- but still an error where the request is wrong
        assert _moments_rc(samples=0, device=device) == (0, True) and _moments_rc(samples=0, missing="moments", device=device) == (0, True)
        assert _moments_rc(samples=0, n_param=60, n_meas=5, device=device) == (ERR_INVALID_ARGUMENT, True)


def test_moments_without_a_device_fail_loudly():
    # no CPU fallback: the reduction is the device's (tests/test_gpu_contributors.py); here the host form either has a device or says so
    rc, untouched = _moments_rc()
    if E.device_count() == 0:
        assert rc == ERR_NO_DEVICE and untouched
        with pytest.raises(E.NonLinearSystemError):
            E.mc_moments(np.zeros((4, 2)), np.zeros((4, 1)), None, None, np.zeros(2), np.zeros(1))
    else:
        assert rc == 0 and not untouched
