"""Monte-Carlo tolerance analysis, what can be checked without a device: the generator's known answers on the reference
(tests/mc_ref.py), the host sampler ezpz_mc_sample against that reference, the independence of a draw from its neighbours, the
moments of 65 536 draws, the corners, the symbols with their signatures and layouts, and the sampler's argument errors.

Bars.  FIXED, UNIFORM and CORNER: bitwise (integer arithmetic, then products and sums of doubles in a stated order, none contracted).
NORMAL: 1e-13 * sigma + 2^-52 * |p| -- the argument of cos and the operand of log are bit-identical on both sides, so only the last
bits of log, cos and sqrt differ: a few ulp of a z of magnitude <= 8.6, near 1e-14, given a tenfold margin, plus the rounding of the
last sum.  Moments: six standard errors of the estimator (failure probability below 1e-8 for a correct sampler)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ezpz_amd as E
import mc_ref as R
from ezpz_amd._lib import EXPORTS, CMcConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARGUMENT = -103

SIGNATURES = {
    "ezpz_mc_sample": ["seed", "dist", "nominal", "n_param", "first", "count", "params_out"],
    "ezpz_system_tolerance_mc": ["sys", "x0", "positions", "n_param", "dist", "nominal", "records", "n_meas", "lim_lo", "lim_hi", "hist_lo",
                                 "hist_hi", "samples", "mc", "cfg", "stats", "totals", "hist", "keep_params", "keep_m", "keep_flags", "keep_ok"],
    "ezpz_system_tolerance_mc_device": ["sys", "x0_dev", "positions", "n_param", "dist", "nominal", "records", "n_meas", "lim_lo", "lim_hi",
                                        "hist_lo", "hist_hi", "samples", "mc", "cfg", "stats_dev", "totals_dev", "hist_dev",
                                        "keep_params_dev", "keep_m_dev", "keep_flags_dev", "keep_ok_dev", "stream"],
}


def _dists(tuples):
    return [E.McDist(*t) for t in tuples]


def test_philox_known_answers():
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in cases:
        assert " ".join("%08x" % w for w in R.philox4x32_10(counter, key)) == want


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
    assert "ezpz_default_mc_config" in EXPORTS and re.search(r"void ezpz_default_mc_config\(EzpzMcConfig\* mc\);", header)
    assert E.MC_DIST_DTYPE.itemsize == 24 and E.MC_STATS_DTYPE.itemsize == 88 and E.MC_TOTALS_DTYPE.itemsize == 24
    assert E.MC_STATS_DTYPE == R.STATS_DTYPE and E.MC_TOTALS_DTYPE == R.TOTALS_DTYPE
    assert C.sizeof(CMcConfig) == 16
    for text in ("typedef struct EzpzMcDist { /* 24 bytes */", "88 bytes */", "typedef struct EzpzMcTotals { /* 24 bytes */"):
        assert text in header
    mc = CMcConfig(7, 7, 7)
    L.ezpz_default_mc_config(C.byref(mc))
    assert (mc.seed, mc.chunk, mc.hist_bins) == (0, 0, 0)
    for method in ("tolerance_mc", "tolerance_mc_device"):
        assert callable(getattr(E.System, method))
    assert (E.McDist.fixed().kind, E.McDist.uniform(-1, 1).kind, E.McDist.normal(1.0).kind, E.McDist.corner(0, 1).kind) == (0, 1, 2, 3)
    assert (R.FIXED, R.UNIFORM, R.NORMAL, R.CORNER) == (0, 1, 2, 3)
    for k, name in enumerate(("FIXED", "UNIFORM", "NORMAL", "CORNER")):
        assert "#define EZPZ_MC_%s %du" % (name, k) in header


# (kind, a, b) per dimension: every kind, a truncation of 1.0 (several attempts), of 2.5, and none
MIXED = [(R.UNIFORM, -0.25, 0.5), (R.NORMAL, 0.125, 0.0), (R.FIXED, 0.0, 0.0), (R.NORMAL, 2.0, 1.0), (R.CORNER, -0.5, 0.75),
         (R.NORMAL, 0.01, 2.5), (R.UNIFORM, 0.0, 0.0), (R.CORNER, 1.0, 1.5), (R.NORMAL, 0.0, 0.0)]
NOMINAL = np.array([1.0, -2.5, 3.25, 100.0, 0.0, -7.0, 1e-3, 12.0, 5.0])
SEED = 0x5EED0123456789AB


def assert_draws_equal_reference(got, want, dists):
    """The bars of this module's docstring, per kind."""
    kinds = np.array([d[0] for d in dists])
    exact = kinds != R.NORMAL
    assert got[:, exact].tobytes() == want[:, exact].tobytes()
    sigma = np.array([d[1] if d[0] == R.NORMAL else 0.0 for d in dists])
    assert np.all(np.abs(got - want) <= 1e-13 * sigma + 2.0 ** -52 * np.abs(want))


def test_sample_equals_the_reference():
    first, count = (1 << 32) - 100, 200  # (the sample index crosses 2^32: both counter words are in play)
    # no reference z within 1e-9 of its truncation: an accept / reject decision cannot flip on the last bits of log, cos, sqrt
    for j, (kind, _, trunc) in enumerate(MIXED):
        if kind == R.NORMAL and trunc:
            for s in range(count):
                assert all(abs(abs(z) - trunc) > 1e-9 for z in R.normal_attempts(SEED, first + s, j, trunc)[1])
    got = E.mc_sample(SEED, _dists(MIXED), NOMINAL, first, count)
    assert_draws_equal_reference(got, R.sample(SEED, MIXED, NOMINAL, first, count), MIXED)
    assert got[:, 2].tobytes() == np.full(count, 3.25).tobytes() and got[:, 8].tobytes() == np.full(count, 5.0).tobytes()


def test_truncation_takes_several_attempts():
    dists, nominal, count = [(R.NORMAL, 1.5, 1.0)], np.array([10.0]), 2000
    tried = [R.normal_attempts(SEED, s, 0, 1.0) for s in range(count)]
    assert all(abs(abs(z) - 1.0) > 1e-9 for _, zs in tried for z in zs)
    assert sum(len(zs) > 1 for _, zs in tried) >= 0.2 * count
    got = E.mc_sample(SEED, _dists(dists), nominal, 0, count)
    assert_draws_equal_reference(got, R.sample(SEED, dists, nominal, 0, count), dists)
    assert np.all(np.abs(got - 10.0) <= 1.5)


def test_a_draw_does_not_depend_on_its_neighbours():
    all100 = E.mc_sample(SEED, _dists(MIXED), NOMINAL, 0, 100)
    assert E.mc_sample(SEED, _dists(MIXED), NOMINAL, 37, 5).tobytes() == all100[37:42].tobytes()
    other = list(MIXED)
    other[0], other[2], other[5] = (R.NORMAL, 1.0, 0.0), (R.UNIFORM, -1.0, 1.0), (R.FIXED, 0.0, 0.0)
    got = E.mc_sample(SEED, _dists(other), NOMINAL, 0, 100)
    for j in (1, 3, 4, 6, 7, 8):  # (4 and 7 keep their ranks among the CORNER dimensions)
        assert got[:, j].tobytes() == all100[:, j].tobytes(), j
    assert got[:, 0].tobytes() != all100[:, 0].tobytes()
    assert E.mc_sample(SEED + 1, _dists(MIXED), NOMINAL, 0, 100)[:, 0].tobytes() != all100[:, 0].tobytes()


def test_moments_of_65536_draws():
    n, a, b, sigma = 65536, -0.3, 0.9, 0.7
    p = E.mc_sample(2024, _dists([(R.UNIFORM, a, b), (R.NORMAL, sigma, 0.0)]), np.zeros(2), 0, n)
    assert abs(p[:, 0].mean() - (a + b) / 2) <= 6 * (b - a) / math.sqrt(12) / math.sqrt(n)
    assert p[:, 0].min() >= a and p[:, 0].max() < b
    assert abs(p[:, 1].mean()) <= 6 * sigma / math.sqrt(n)
    assert abs(p[:, 1].var(ddof=1) - sigma ** 2) <= 6 * sigma ** 2 * math.sqrt(2 / n)


def test_corners_in_index_order():
    dists = [(R.CORNER, -1.0, 1.0), (R.FIXED, 0.0, 0.0), (R.CORNER, -2.0, 2.0), (R.CORNER, 0.25, 0.5)]
    got = E.mc_sample(9, _dists(dists), np.array([10.0, 20.0, 30.0, 40.0]), 0, 8)
    want = [[10.0 + (1.0 if s & 1 else -1.0), 20.0, 30.0 + (2.0 if s & 2 else -2.0), 40.0 + (0.5 if s & 4 else 0.25)] for s in range(8)]
    assert got.tobytes() == np.array(want).tobytes()
    assert E.mc_sample(9, _dists(dists), np.array([10.0, 20.0, 30.0, 40.0]), 8, 8).tobytes() == got.tobytes()  # (bit 3 is nobody's)


BAD = {
    "unknown kind": ([(4, 0.0, 1.0)], [0.0]),
    "a not finite": ([(R.UNIFORM, -math.inf, 1.0)], [0.0]),
    "b not finite": ([(R.NORMAL, 1.0, math.nan)], [0.0]),
    "b of a FIXED not finite": ([(R.FIXED, 0.0, math.inf)], [0.0]),
    "nominal not finite": ([(R.FIXED, 0.0, 0.0), (R.UNIFORM, 0.0, 1.0)], [math.nan, 0.0]),
    "uniform a > b": ([(R.UNIFORM, 1.0, 0.5)], [0.0]),
    "sigma < 0": ([(R.NORMAL, -1e-3, 0.0)], [0.0]),
    "truncation in (0, 1)": ([(R.NORMAL, 1.0, 0.999)], [0.0]),
    "21 corners": ([(R.CORNER, 0.0, 1.0)] * 21, [0.0] * 21),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_sample_argument_errors(what):
    dists, nominal = BAD[what]
    d, nominal = E.api.mc_dists(_dists(dists)), np.array(nominal)
    out = np.full((3, len(d)), 1234.5)
    rc = E.lib().ezpz_mc_sample(1, d.ctypes.data, nominal.ctypes.data, len(d), 0, 3, out.ctypes.data)
    assert rc == ERR_INVALID_ARGUMENT and np.all(out == 1234.5), what


def test_sample_null_arguments_and_the_legal_edges():
    L = E.lib()
    d, nominal, out = E.api.mc_dists(_dists([(R.CORNER, 0.0, 1.0)] * 20)), np.zeros(20), np.full((2, 20), 1234.5)
    assert L.ezpz_mc_sample(1, None, nominal.ctypes.data, 20, 0, 2, out.ctypes.data) == ERR_INVALID_ARGUMENT
    assert L.ezpz_mc_sample(1, d.ctypes.data, None, 20, 0, 2, out.ctypes.data) == ERR_INVALID_ARGUMENT
    assert L.ezpz_mc_sample(1, d.ctypes.data, nominal.ctypes.data, 20, 0, 2, None) == ERR_INVALID_ARGUMENT
    assert np.all(out == 1234.5)
    assert L.ezpz_mc_sample(1, d.ctypes.data, nominal.ctypes.data, 20, (1 << 20) - 1, 2, out.ctypes.data) == 0  # 20 corners are legal
    assert out[0].tolist() == [1.0] * 20 and out[1].tolist() == [0.0] * 20
    assert L.ezpz_mc_sample(1, None, None, 0, 0, 5, None) == 0 and L.ezpz_mc_sample(1, d.ctypes.data, nominal.ctypes.data, 20, 0, 0, None) == 0
    assert E.mc_sample(3, _dists([(R.NORMAL, 1.0, 1.0)]), [0.0], 0, 4).shape == (4, 1)  # a truncation of exactly 1 is legal
