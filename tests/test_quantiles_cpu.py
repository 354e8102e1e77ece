"""Monte-Carlo quantiles, what can be checked without a device: the host form (ezpz_mc_quantiles) against tests/quantile_ref.py
byte for byte, its order statistics against numpy.sort of the valid keys, the ABI -- symbols, signatures, the record's layout, the
defaults, every argument error by its return code with the output untouched -- and the band's meaning on host draws.

Bars.  Against the restatement and numpy.sort: bytes.  Meaning: the band at z = 6, the six-standard-error convention of
tests/test_tolerance_mc_cpu.py.  The band [x_k_lo, x_k_hi] holds the true quantile t exactly when the number B of draws below t --
binomial (n, p), mean n p, standard deviation s = sqrt(n p (1 - p)) -- has k_lo <= B - 1 and B <= k_hi, which a deviation of B below
6 s guarantees, and so does B >= 1 where the rule clamps k_lo to 0 (at p = 0.00135 and n = 20000: n p = 27, so B = 0 has probability
e^-27).  That needs 0 < p < 1 and n p of some size: at p = 0, p = 1 and p = 1e-12 the rule's band is the extreme order statistic itself
(s = 0, or both ranks clamped to 0 and 1), which a draw from a continuous distribution never puts ON the end of the range; those three
are asserted for what the rule says about them -- ranks 0 or n - 1 -- and the seven probabilities inside for the band."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ezpz_amd as E
import mc_ref
import quantile_ref as R
from ezpz_amd._lib import EXPORTS, CMcQuantileConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARGUMENT = -103

MC_ARGS = ["sys", "x0", "positions", "n_param", "dist", "nominal", "records", "n_meas", "lim_lo", "lim_hi", "hist_lo", "hist_hi", "samples", "mc",
           "cfg", "stats", "totals", "hist", "keep_params", "keep_m", "keep_flags", "keep_ok"]
MC_ARGS_DEV = ["sys", "x0_dev", "positions", "n_param", "dist", "nominal", "records", "n_meas", "lim_lo", "lim_hi", "hist_lo", "hist_hi", "samples",
               "mc", "cfg", "stats_dev", "totals_dev", "hist_dev", "keep_params_dev", "keep_m_dev", "keep_flags_dev", "keep_ok_dev"]
SIGNATURES = {
    "ezpz_mc_quantiles": ["m", "flags", "ok", "samples", "n_meas", "probs", "n_q", "qc", "out"],
    "ezpz_mc_quantiles_device": ["m_dev", "flags_dev", "ok_dev", "samples", "n_meas", "probs", "n_q", "qc", "out_dev", "stream"],
    "ezpz_system_tolerance_mc_quantiles": MC_ARGS + ["probs", "n_q", "qc", "out"],
    "ezpz_system_tolerance_mc_quantiles_device": MC_ARGS_DEV + ["probs", "n_q", "qc", "out_dev", "stream"],
}
FIELDS = [("n_valid", 0, "<u8"), ("rank", 8, "<u8"), ("rank_lo", 16, "<u8"), ("rank_hi", 24, "<u8"), ("frac", 32, "<f8"), ("lo", 40, "<f8"),
          ("hi", 48, "<f8"), ("value", 56, "<f8"), ("band_lo", 64, "<f8"), ("band_hi", 72, "<f8")]


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
    assert "ezpz_default_mc_quantile_config" in EXPORTS
    assert re.search(r"void ezpz_default_mc_quantile_config\(EzpzMcQuantileConfig\* qc\);", header)
    for text in ("typedef struct EzpzMcQuantileConfig { /* 16 bytes */", "typedef struct EzpzMcQuantile { /* one per (record, probability); 80 bytes */",
                 "uint64_t n_valid, rank, rank_lo, rank_hi; double frac, lo, hi, value, band_lo, band_hi; } EzpzMcQuantile;",
                 "#define EZPZ_MC_QUANTILE_MAX_PROBS 16u", "#define EZPZ_MC_QUANTILE_MAX_MEAS 64u"):
        assert text in header, text
    # the record's layout, pinned: the library's dtype, the restatement's, and the offsets
    assert E.MC_QUANTILE_DTYPE == R.DTYPE and E.MC_QUANTILE_DTYPE.itemsize == 80 and C.sizeof(CMcQuantileConfig) == 16
    assert [(n, E.MC_QUANTILE_DTYPE.fields[n][1], E.MC_QUANTILE_DTYPE.fields[n][0].str) for n in E.MC_QUANTILE_DTYPE.names] == FIELDS
    one = E.mc_quantiles(np.array([[2.0], [4.0]]), None, None, [0.25], 0.0)  # the library writes where the dtype says
    words = np.frombuffer(one.tobytes(), dtype="<u8")
    assert words[:4].tolist() == [2, 0, 0, 1] and np.frombuffer(one.tobytes(), dtype="<f8")[4:].tolist() == [0.25, 2.0, 4.0, 2.5, 2.0, 4.0]
    qc = CMcQuantileConfig(7.0, 7)
    L.ezpz_default_mc_quantile_config(C.byref(qc))
    assert (qc.z, qc.reserved) == (0.0, 0)
    L.ezpz_default_mc_quantile_config(None)
    assert "mc_quantiles" in E.__all__ and "MC_QUANTILE_DTYPE" in E.__all__ and hasattr(E, "mc_quantiles")
    import inspect
    for fn in (E.System.tolerance_mc, E.System.tolerance_mc_device):
        p = inspect.signature(fn).parameters
        assert p["quantiles"].default is None and p["quantile_z"].default == 0.0


# ---- the generator -------------------------------------------------------------------------------------------------------------------
PAIR_LOW = np.array([0x3FF4000000000010, 0x3FF4000000000011], np.uint64).view(np.float64)   # differ in the lowest key byte alone
PAIR_HIGH = np.array([0x3FFC000000000000, 0x3EFC000000000000], np.uint64).view(np.float64)  # ... in the highest (1.75, 1.75 * 2^-16)
FIRST_INVALID = 15  # the samples below hold the fixed values; the invalid ones are interleaved from here on


def kind_of(i, n_meas, seed):
    """'general', or one of the special records: records 1, 2 and 3 take 'same' (all one value), 'none' (no valid sample) and 'one'
    (exactly one), rotated by the seed, so that n_meas == 3 sees two of them per seed and n_meas >= 4 all three."""
    return ("same", "none", "one")[(i - 1 + seed) % 3] if 1 <= i <= 3 else "general"


def rows_of_q(n_meas, samples, seed):
    """(m, flags, ok), deterministic.  A general record i has, where `samples` reaches: -0.0 at sample 2, +0.0 at 3, a subnormal at
    4, a negative value at 7, a positive one at 8, PAIR_LOW at 9 and 12, PAIR_HIGH at 13 and 14; one value, 0.125 (i + 1), at every
    sample b < 15 with b % 5 < 2 and at every even b from there on (at least 40 % of the record from 20 samples on); normal draws of
    both signs elsewhere.  From sample 15 on: ok = 0 where b % 11 == 5, and
    where (b + 3 i) % 7 == 3 flag bit 0, NaN or +inf in turn.  Flag bit 1 is noise.  The special records: kind_of."""
    rng = np.random.default_rng(1000003 * seed + 1009 * n_meas + samples)
    b = np.arange(samples)
    m = rng.normal(size=(samples, n_meas)) * rng.uniform(1e-3, 1e3, n_meas)
    flags = (rng.integers(0, 2, (samples, n_meas)) * 2).astype(np.uint8)
    ok = np.where((b >= FIRST_INVALID) & (b % 11 == 5), 0, 1).astype(np.uint8)
    for i in range(n_meas):
        kind = kind_of(i, n_meas, seed)
        if kind == "same":
            m[:, i] = -3.25
            continue
        if kind == "none":
            flags[::2, i] |= 1
            m[1::2, i] = np.nan
            continue
        if kind == "one":
            flags[:, i] |= 1
            flags[min(samples - 1, 6), i] = 2
            continue
        m[np.where(b < FIRST_INVALID, b % 5 < 2, b % 2 == 0), i] = 0.125 * (i + 1)
        fixed = {2: -0.0, 3: 0.0, 4: 5e-324 * (i + 1), 7: -1.5 - i, 8: 2.5 + i, 9: PAIR_LOW[0], 12: PAIR_LOW[1], 13: PAIR_HIGH[0], 14: PAIR_HIGH[1]}
        for at, v in fixed.items():
            if at < samples:
                m[at, i] = v
        bad = (b >= FIRST_INVALID) & ((b + 3 * i) % 7 == 3)
        cause = ((b + 3 * i) // 7) % 3
        flags[bad & (cause == 0), i] |= 1
        m[bad & (cause == 1), i] = np.nan
        m[bad & (cause == 2), i] = np.inf
    return m, flags, ok


def test_the_generator_holds_what_it_promises():
    m, flags, ok = rows_of_q(64, 1000, 1)
    kinds = [kind_of(i, 64, 1) for i in range(64)]
    assert sorted(kinds[1:4]) == ["none", "one", "same"] and {kind_of(i, 3, s) for s in (0, 1) for i in range(3)} >= {"same", "none", "one"}
    valid = np.isfinite(m) & ((flags & 1) == 0) & (ok != 0)[:, None]
    key = R.keys(m)
    general = [i for i, kind in enumerate(kinds) if kind == "general"]
    assert len(general) == 61 and (key[9, general] ^ key[12, general]).max() < 256
    assert np.all((key[13, general] ^ key[14, general]) == np.uint64(1 << 56))
    for i, kind in enumerate(kinds):
        n = int(valid[:, i].sum())
        if kind == "none":
            assert n == 0
        elif kind == "one":
            assert n == 1
        elif kind == "same":
            assert n > 800 and len(set(m[valid[:, i], i].tolist())) == 1
        else:
            v = m[valid[:, i], i]
            assert np.all(valid[:15, i]) and v.min() < 0 < v.max() and np.signbit(m[2, i]) and m[2, i] == 0 and not np.signbit(m[3, i])
            assert 0 < m[4, i] < 2.3e-308 and (v == 0.125 * (i + 1)).sum() >= 0.4 * n
            for bad in (np.isnan(m[:, i]), np.isposinf(m[:, i]), (flags[:, i] & 1) != 0):
                assert bad[15:].sum() > 20 and not bad[:15].any()
    assert (ok == 0).sum() > 50 and (flags & 2).any()


# ---- the host form against the restatement -----------------------------------------------------------------------------------------
SAMPLES = (1, 2, 255, 256, 257, 1000)
SHAPES = ((1, 1), (3, 5), (64, 16))
PROBS16 = [0.0, 1.0, 0.5, 0.00135, 0.99865, 1e-12, 0.25, 0.75, 0.1, 0.9, 0.3333333333333333, 1.0 - 2.0 ** -53, 0.01, 0.99, 0.05, 0.6180339887498949]
_CACHE = {}


def probs_of(n_q):
    return PROBS16[:n_q] if n_q != 1 else [0.00135]


def reference(n_meas, n_q, samples, z, bare=False):
    """The restatement's records for rows_of_q(n_meas, samples, samples % 2), computed once."""
    key = (n_meas, n_q, samples, z, bare)
    if key not in _CACHE:
        m, flags, ok = rows_of_q(n_meas, samples, samples % 2)
        _CACHE[key] = R.quantiles(m, None if bare else flags, None if bare else ok, probs_of(n_q), z)
    return _CACHE[key]


@pytest.mark.parametrize("z", [0.0, 3.0])
@pytest.mark.parametrize("n_meas,n_q", SHAPES)
@pytest.mark.parametrize("samples", SAMPLES)
def test_the_host_form_is_the_stated_rule(samples, n_meas, n_q, z):
    m, flags, ok = rows_of_q(n_meas, samples, samples % 2)
    probs = probs_of(n_q)
    want = reference(n_meas, n_q, samples, z)
    got = E.mc_quantiles(m, flags, ok, probs, z)
    assert got.shape == (n_meas, n_q) and got.tobytes() == want.tobytes(), (got, want)
    # lo, hi and the band are numpy.sort of the valid keys at the stated ranks
    for i in range(n_meas):
        keys = np.sort(R.keys(m[np.isfinite(m[:, i]) & ((flags[:, i] & 1) == 0) & (ok != 0), i]))
        n = len(keys)
        assert np.all(got["n_valid"][i] == n)
        if n == 0:
            assert np.all(got["rank"][i] == R.NONE) and np.all(got["rank_lo"][i] == R.NONE) and np.all(got["rank_hi"][i] == R.NONE)
            assert all(np.isnan(got[f][i]).all() for f in ("frac", "lo", "hi", "value", "band_lo", "band_hi"))
            continue
        rank = got["rank"][i].astype(np.int64)
        assert np.all(got["rank_lo"][i] <= got["rank"][i]) and np.all(got["rank"][i] <= got["rank_hi"][i]) and np.all(got["rank_hi"][i] < n)
        for field, at in (("lo", rank), ("hi", np.minimum(rank + 1, n - 1)), ("band_lo", got["rank_lo"][i].astype(np.int64)),
                          ("band_hi", got["rank_hi"][i].astype(np.int64))):
            assert R.keys(got[field][i]).tolist() == keys[at].tolist(), (i, field)
        assert np.all(got["lo"][i] <= got["value"][i]) and np.all(got["value"][i] <= got["hi"][i])
    if samples == 257:  # flags == NULL: every bit clear; ok == NULL: every one set
        bare = E.mc_quantiles(m, None, None, probs, z)
        assert bare.tobytes() == reference(n_meas, n_q, samples, z, bare=True).tobytes() and np.all(bare["n_valid"] >= got["n_valid"])
    if z == 0.0 and n_q > 1 and samples > 2:
        general = [i for i in range(n_meas) if kind_of(i, n_meas, samples % 2) == "general"]
        assert np.all(got["rank_lo"][general] == got["rank"][general])
        assert np.signbit(got["lo"][general, 0]).all()  # (p = 0: the minimum is negative)


def test_minus_zero_sorts_before_plus_zero_and_ties_need_no_rule():
    m = np.array([[0.0], [-0.0], [0.0], [-0.0], [1.0], [1.0]])
    got = E.mc_quantiles(m, None, None, [0.0, 0.2, 0.4, 0.6, 0.3], 0.0)
    assert np.signbit(got["lo"][0]).tolist() == [True, True, False, False, True] and got["hi"][0, 3] == 1.0
    assert got.tobytes() == R.quantiles(m, None, None, [0.0, 0.2, 0.4, 0.6, 0.3], 0.0).tobytes()
    assert got["frac"][0, 4] == 0.5 and not np.signbit(got["value"][0, 4])  # (-0.0 + 0.5 * (+0.0 - -0.0) = -0.0 + +0.0 = +0.0)


def raw(m, flags, ok, samples, n_meas, probs, n_q, z, out):
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    qc = CMcQuantileConfig(z, 0)
    return E.lib().ezpz_mc_quantiles(ptr(m), ptr(flags), ptr(ok), samples, n_meas, ptr(probs), n_q, C.byref(qc), ptr(out))


def test_every_argument_error_leaves_the_output_untouched():
    m, flags, ok = rows_of_q(3, 10, 0)
    probs = np.array([0.1, 0.5, 0.9])
    many = np.full(17, 0.5)
    wide = np.zeros((10, 65))
    nan, inf = float("nan"), float("inf")
    cases = [
        dict(n_meas=0), dict(m=wide, flags=None, n_meas=65), dict(probs=many, n_q=17), dict(samples=1 << 32),
        dict(probs=np.array([0.1, -1e-300, 0.9])), dict(probs=np.array([0.1, 1.0000000000000002, 0.9])), dict(probs=np.array([nan, 0.5, 0.9])),
        dict(probs=np.array([0.1, 0.5, inf])), dict(z=-1.0), dict(z=nan), dict(z=inf), dict(probs=None), dict(m=None),
    ]
    for case in cases:
        out = np.full(65 * 17 * 80, 7, np.uint8)
        a = dict(m=m, flags=flags, ok=ok, samples=10, n_meas=3, probs=probs, n_q=3, z=0.0)
        a.update(case)
        assert raw(a["m"], a["flags"], a["ok"], a["samples"], a["n_meas"], a["probs"], a["n_q"], a["z"], out) == ERR_INVALID_ARGUMENT, case
        assert np.all(out == 7), case
    assert raw(m, flags, ok, 10, 3, probs, 3, 0.0, None) == ERR_INVALID_ARGUMENT
    # samples == 0 or n_q == 0: EZPZ_OK after the checks, nothing written
    out = np.full(3 * 3 * 80, 7, np.uint8)
    assert raw(None, None, None, 0, 3, probs, 3, 0.0, out) == 0 and raw(m, flags, ok, 10, 3, None, 0, 0.0, None) == 0 and np.all(out == 7)
    assert raw(None, None, None, 0, 3, probs, 3, -1.0, out) == ERR_INVALID_ARGUMENT and raw(m, flags, ok, 10, 0, None, 0, 0.0, None) == ERR_INVALID_ARGUMENT
    # qc == NULL: the default, z = 0
    got = np.zeros((3, 3), E.MC_QUANTILE_DTYPE)
    rc = E.lib().ezpz_mc_quantiles(m.ctypes.data, flags.ctypes.data, ok.ctypes.data, 10, 3, probs.ctypes.data, 3, None, got.ctypes.data)
    assert rc == 0 and got.tobytes() == E.mc_quantiles(m, flags, ok, probs, 0.0).tobytes()
    with pytest.raises(ValueError):
        E.System.tolerance_mc(None, None, None, None, None, 1, contributors=True, quantiles=[0.5])


# ---- the meaning -------------------------------------------------------------------------------------------------------------------
INSIDE = [0.00135, 0.01, 0.25, 0.5, 0.75, 0.99, 0.99865]
EDGES = [0.0, 1.0, 1e-12]


def test_the_band_holds_the_true_quantile_of_a_uniform_dimension():
    n, a, b, nominal = 20000, -0.3, 0.5, 2.0
    p = E.mc_sample(777, [E.McDist(mc_ref.UNIFORM, a, b)], np.array([nominal]), 0, n)
    got = E.mc_quantiles(p, None, None, INSIDE + EDGES, 6.0)[0]
    assert np.all(got["n_valid"] == n)
    for q, prob in enumerate(INSIDE):
        true = nominal + (a + prob * (b - a))
        print("p", prob, "true", true, "band", got["band_lo"][q], got["band_hi"][q], "value", got["value"][q], "ranks", got["rank_lo"][q], got["rank_hi"][q])
        assert got["band_lo"][q] <= true <= got["band_hi"][q], prob
        assert got["band_lo"][q] <= got["value"][q] <= got["band_hi"][q]
        assert abs(got["value"][q] - true) <= 6 * (b - a) * np.sqrt(prob * (1 - prob) / n) + (b - a) / n  # (the same bar, as a value)
    # the edges: the extreme order statistics themselves (the docstring says why the band cannot hold the end of the range)
    lo, hi = p.min(), p.max()
    assert (got["rank_lo"][7], got["rank_hi"][7], got["value"][7]) == (0, 0, lo) and (got["rank_lo"][8], got["rank_hi"][8], got["value"][8]) == (n - 1, n - 1, hi)
    assert (got["rank"][9], got["rank_lo"][9], got["rank_hi"][9]) == (0, 0, 1) and lo <= got["value"][9] <= got["band_hi"][9]
    assert nominal + a <= lo and hi < nominal + b
