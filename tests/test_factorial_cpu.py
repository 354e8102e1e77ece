"""Factorial effects of a corner run, what can be checked without a device: the host form (ezpz_mc_factorial) against
tests/factorial_ref.py byte for byte in every output, exact cases in dyadic values, Parseval against numpy.var, and the ABI -- symbols,
signatures, the record's layout, the limits, every argument error by its return code with the outputs untouched, the Python
signatures and refusals.

Bars.  Against the restatement: bytes.  The exact cases: equality (every value is a small dyadic number, so every butterfly, product
and sum is exact).  Parseval: |var - numpy.var(y)| <= (4 kc + N / 256 + 16) * 2^-53 * max(y^2), derived, not measured: a coefficient
carries at most kc roundings relative to max|y|, so its square at most 2 kc + 1; the tree and the left-to-right blocks add 8 + N / 256;
the rest is slack for numpy's own sum.  (The sum of the squared coefficients of order >= 1 is at most max(y^2), which is what the
relative roundings scale with.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import ezpz_amd as E
import factorial_ref as R
from ezpz_amd._lib import EXPORTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARGUMENT = -103

MC_ARGS = ["sys", "x0", "positions", "n_param", "dist", "nominal", "records", "n_meas", "lim_lo", "lim_hi", "hist_lo", "hist_hi", "samples", "mc",
           "cfg", "stats", "totals", "hist", "keep_params", "keep_m", "keep_flags", "keep_ok"]
MC_ARGS_DEV = ["sys", "x0_dev", "positions", "n_param", "dist", "nominal", "records", "n_meas", "lim_lo", "lim_hi", "hist_lo", "hist_hi", "samples",
               "mc", "cfg", "stats_dev", "totals_dev", "hist_dev", "keep_params_dev", "keep_m_dev", "keep_flags_dev", "keep_ok_dev"]
OUTS = ["info", "main", "pair", "ss_order", "ss_total", "first", "total", "coef"]
SIGNATURES = {
    "ezpz_mc_factorial": ["m", "flags", "ok", "nominal_m", "n_corner", "n_meas"] + OUTS,
    "ezpz_mc_factorial_device": ["m_dev", "flags_dev", "ok_dev", "nominal_m_dev", "n_corner", "n_meas"] + [o + "_dev" for o in OUTS] + ["stream"],
    "ezpz_system_tolerance_mc_factorial": MC_ARGS + OUTS,
    "ezpz_system_tolerance_mc_factorial_device": MC_ARGS_DEV + [o + "_dev" for o in OUTS] + ["stream"],
}
FIELDS = [("n_valid", 0, "<u8"), ("complete", 8, "<u4"), ("corner_hi", 12, "<u4"), ("corner_lo", 16, "<u4"), ("reserved", 20, "<u4"),
          ("mean_dev", 24, "<f8"), ("var", 32, "<f8"), ("m_hi", 40, "<f8"), ("m_lo", 48, "<f8")]
NAMES = ("info", "main", "pair", "ss_order", "ss_total", "first", "total", "coef")


def parts(f):
    """the eight outputs of an McFactorial, in the library's order"""
    return [getattr(f, n) for n in NAMES]


def same_bytes(got, want):
    return [n for n, g, w in zip(NAMES, got, want) if g.tobytes() != w.tobytes()] == []


def test_symbols_signatures_layout_and_limits():
    L = E.lib()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ezpz_amd.h")).read())
    for name, params in SIGNATURES.items():
        assert name in EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(params), name
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl, name
        assert [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")] == params, name
    for text in ("typedef struct EzpzMcFactorial { /* one per record; 56 bytes */",
                 "uint64_t n_valid; uint32_t complete, corner_hi, corner_lo, reserved; double mean_dev, var, m_hi, m_lo; } EzpzMcFactorial;",
                 "#define EZPZ_MC_FACTORIAL_MAX_CORNERS 20u", "#define EZPZ_MC_FACTORIAL_MAX_MEAS 32u"):
        assert text in header, text
    assert (R.MAX_CORNERS, R.MAX_MEAS) == (20, 32)
    # the record's layout, pinned: the library's dtype, the restatement's, and the offsets
    D = E.MC_FACTORIAL_DTYPE
    assert D == R.DTYPE and D.itemsize == 56
    assert [(n, D.fields[n][1], D.fields[n][0].str) for n in D.names] == FIELDS
    one = E.mc_factorial(np.array([[7.0], [5.0], [9.0], [11.0]]), None, None, [8.0])  # the library writes where the dtype says
    raw = one.info.tobytes()
    assert np.frombuffer(raw[:8], "<u8")[0] == 4 and np.frombuffer(raw[8:24], "<u4").tolist() == [1, 0b10, 0, 0]
    assert np.frombuffer(raw[24:], "<f8").tolist() == [0.0, 5.0, 9.0, 7.0]  # y = -1 -3 1 3 = 2 s_1 + s_0 s_1: mean 0, var 5, m[2] = 9, m[0] = 7
    for name in ("mc_factorial", "mc_corner_count", "McFactorial", "MC_FACTORIAL_DTYPE"):
        assert name in E.__all__ and hasattr(E, name), name
    for fn in (E.System.tolerance_mc, E.System.tolerance_mc_device):
        assert inspect.signature(fn).parameters["factorial"].default is False
    assert inspect.signature(E.System.tolerance_mc).parameters["keep_coef"].default is False
    dev = inspect.signature(E.System.tolerance_mc_device).parameters
    assert all(dev["factorial_%s_ptr" % o].default == 0 for o in OUTS)
    assert E.mc_corner_count([E.McDist.corner(-1, 1), E.McDist.fixed(), E.McDist.corner(0, 2), E.McDist.uniform(0, 1)]) == 4


# ---- the generator -------------------------------------------------------------------------------------------------------------------
CAUSES, PLACES = ("ok", "flag", "nan", "inf"), ("first", "middle", "last")


def rows_of_f(kc, n_meas, cause=None, place=None):
    """(m, flags, ok, nominal_m), deterministic: N = 2^kc rows of normal draws of both signs about a nominal per record, each record
    at a scale of its own.  Record 0 holds -0.0 at row 0, +0.0 at row 1 and, from 4 rows on, a subnormal at row 2.  Record 1 (n_meas >=
    2) is constant: nominal + 0.375.  Flag bit 1 is noise.  With a cause, record min(2, n_meas - 1) is made incomplete at the first, a
    middle or the last row by ok == 0 (every record with it), flag bit 0, NaN or +inf."""
    N = 1 << kc
    rng = np.random.default_rng(7919 * kc + n_meas)
    nominal = rng.uniform(-3.0, 3.0, n_meas)
    m = nominal + rng.normal(size=(N, n_meas)) * rng.uniform(1e-3, 1e2, n_meas)
    flags = (rng.integers(0, 2, (N, n_meas)) * 2).astype(np.uint8)
    ok = np.ones(N, np.uint8)
    m[0, 0], m[1, 0] = -0.0, 0.0
    if N >= 4:
        m[2, 0] = 5e-324 * 3
    if n_meas >= 2:
        m[:, 1] = nominal[1] + 0.375
    if cause is not None:
        i, b = min(2, n_meas - 1), {"first": 0, "middle": N // 2 - 1, "last": N - 1}[place]
        if cause == "ok":
            ok[b] = 0
        elif cause == "flag":
            flags[b, i] |= 1
        else:
            m[b, i] = np.nan if cause == "nan" else np.inf
    return m, flags, ok, nominal


_CACHE = {}


def reference(kc, n_meas, cause=None, place=None, bare=False):
    """The restatement's outputs for rows_of_f(kc, n_meas, cause, place), computed once; bare: flags == ok == NULL."""
    key = (kc, n_meas, cause, place, bare)
    if key not in _CACHE:
        m, flags, ok, nominal = rows_of_f(kc, n_meas, cause, place)
        _CACHE[key] = R.factorial(m, None if bare else flags, None if bare else ok, nominal)
    return _CACHE[key]


def test_the_generator_holds_what_it_promises():
    m, flags, ok, nominal = rows_of_f(5, 3)
    assert np.signbit(m[0, 0]) and m[0, 0] == 0 and not np.signbit(m[1, 0]) and 0 < m[2, 0] < 2.3e-308
    assert (m[:, 2] < nominal[2]).any() and (m[:, 2] > nominal[2]).any() and len(set(m[:, 1].tolist())) == 1 and (flags & 2).any()
    seen = set()
    for cause in CAUSES:
        for place in PLACES:
            m, flags, ok, _ = rows_of_f(5, 3, cause, place)
            bad = ~(np.isfinite(m[:, 2]) & ((flags[:, 2] & 1) == 0) & (ok != 0))
            assert bad.sum() == 1
            seen.add((cause, int(np.argmax(bad))))
    assert {b for _, b in seen} == {0, 15, 31} and len(seen) == 12
    assert int(np.argmax(rows_of_f(1, 1, "nan", "middle")[0][:, 0] != rows_of_f(1, 1)[0][:, 0])) == 0  # (N == 2: the middle is row 0)


# ---- the host form against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_meas", [1, 3, 32])
@pytest.mark.parametrize("kc", range(1, 13))
def test_the_host_form_is_the_stated_rule(kc, n_meas):
    N = 1 << kc
    m, flags, ok, nominal = rows_of_f(kc, n_meas)
    want = reference(kc, n_meas)
    got = E.mc_factorial(m, flags, ok, nominal, keep_coef=True)
    assert same_bytes(parts(got), want), (kc, n_meas)
    assert np.all(got.complete == 1) and np.all(got.n_valid == N)
    assert got.main.shape == (n_meas, kc) and got.pair.shape == (n_meas, kc, kc) and got.coef.shape == (n_meas, N)
    # what the outputs are to each other
    assert got.main.tobytes() == got.coef[:, [1 << c for c in range(kc)]].tobytes() and got.mean_dev.tobytes() == got.coef[:, 0].tobytes()
    assert got.pair.tobytes() == got.pair.transpose(0, 2, 1).tobytes()
    assert not np.signbit(got.pair[:, np.arange(kc), np.arange(kc)]).any() and np.all(got.pair[:, np.arange(kc), np.arange(kc)] == 0)
    assert got.main_effect.tobytes() == (2.0 * got.main).tobytes() and got.interaction.tobytes() == (got.total - got.first).tobytes()
    for i in range(n_meas):
        assert got.m_hi[i] == m[got.corner_hi[i], i] and got.m_lo[i] == m[got.corner_lo[i], i]
        assert got.corner_hi[i] & got.corner_lo[i] == 0
    if n_meas >= 2:  # the constant record: one coefficient, no variance, indices +0.0, masks 0
        assert got.var[1] == 0 and got.mean_dev[1] == (m[0, 1] - nominal[1]) and np.all(got.coef[1, 1:] == 0)
        assert got.first[1].tobytes() == got.total[1].tobytes() == np.zeros(kc).tobytes() and got.corner_hi[1] == got.corner_lo[1] == 0
    # without coef the other outputs are the same; flags == NULL: every bit clear; ok == NULL: every one set
    lean = E.mc_factorial(m, flags, ok, nominal)
    assert lean.coef is None and same_bytes(parts(lean)[:7], want[:7])
    bare = E.mc_factorial(m, None, None, nominal, keep_coef=True)
    assert same_bytes(parts(bare), reference(kc, n_meas, bare=True)) and same_bytes(parts(bare), want)
    # a record made incomplete by each cause in turn, at the first, a middle and the last row
    for cause in CAUSES:
        for place in PLACES:
            m2, flags2, ok2, _ = rows_of_f(kc, n_meas, cause, place)
            want2 = reference(kc, n_meas, cause, place)
            got2 = E.mc_factorial(m2, flags2, ok2, nominal, keep_coef=True)
            assert same_bytes(parts(got2), want2), (kc, n_meas, cause, place)
            i = min(2, n_meas - 1)
            hit = range(n_meas) if cause == "ok" else [i]
            for j in range(n_meas):
                if j in hit:
                    assert got2.n_valid[j] == N - 1 and got2.complete[j] == 0 and got2.corner_hi[j] == got2.corner_lo[j] == 0
                    for a in (got2.main[j], got2.pair[j], got2.ss_order[j], got2.ss_total[j], got2.first[j], got2.total[j], got2.coef[j],
                              got2.info[["mean_dev", "var", "m_hi", "m_lo"]][j].tolist()):
                        assert np.all(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == 0x7FF8000000000000)  # (THE NaN)
                else:  # the other records do not notice
                    assert all(g[j].tobytes() == w[j].tobytes() for g, w in zip(parts(got2), want))


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def signs(kc):
    """s [N, kc]: +1 where bit c of the row is set (the b end), -1 where not."""
    return np.where((np.arange(1 << kc)[:, None] >> np.arange(kc)) & 1, 1.0, -1.0)


def test_an_additive_record_has_mains_alone():
    a = np.array([1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 2.0])  # the squares sum to 16
    kc, nominal = len(a), 10.0
    y = signs(kc) @ a
    f = E.mc_factorial((nominal + y)[:, None], None, None, [nominal], keep_coef=True)
    assert f.main[0].tolist() == a.tolist() and f.mean_dev[0] == 0
    rest = np.ones(1 << kc, bool)
    rest[[1 << c for c in range(kc)]] = False
    assert np.all(f.coef[0, rest] == 0) and np.all(f.pair[0] == 0)
    assert f.var[0] == 16.0 and f.ss_order[0].tolist() == [0.0, 16.0] + [0.0] * (kc - 1)
    assert f.first[0].tolist() == (a * a / 16.0).tolist() and float(np.sum(f.first[0])) == 1.0
    assert f.total[0].tobytes() == f.first[0].tobytes() and np.all(f.interaction[0] == 0)
    assert f.corner_hi[0] == 0b1010101 and f.corner_lo[0] == 0b0101010
    assert f.m_hi[0] == nominal + 10.0 and f.m_lo[0] == nominal - 10.0  # the linear prediction is the truth
    assert same_bytes(parts(f), R.factorial((nominal + y)[:, None], None, None, [nominal]))
    assert [t[1] for t in f.largest(0, 3)] == [(4,), (5,), (6,)] and [abs(t[0]) for t in f.largest(0, 3)] == [2.0] * 3


def test_a_pure_product_has_one_pair_alone():
    s = signs(3)  # (the third dimension does nothing)
    y = s[:, 0] * s[:, 1]
    f = E.mc_factorial((4.0 + y)[:, None], None, None, [4.0], keep_coef=True)
    want = np.zeros(8)
    want[0b011] = 1.0
    assert f.coef[0].tolist() == want.tolist() and f.pair[0, 0, 1] == f.pair[0, 1, 0] == 1.0 and np.count_nonzero(f.pair[0]) == 2
    assert np.all(f.main[0] == 0) and np.all(f.first[0] == 0) and f.total[0].tolist() == [1.0, 1.0, 0.0] and f.var[0] == 1.0
    assert f.interaction[0].tolist() == [1.0, 1.0, 0.0] and f.corner_hi[0] == f.corner_lo[0] == 0
    assert f.largest(0, 1) == [(1.0, (0, 1))]


def test_the_linear_signs_can_point_at_the_wrong_corner():
    """y = s_0 + s_1 - 3 s_0 s_1: both mains are positive, so the linear stack-up calls corner 0b11 the maximum -- where the value
    is nominal - 1 -- while the maximum, nominal + 3, sits at corners 1 and 2.  The case the feature exists for."""
    s, nominal = signs(2), 20.0
    y = s[:, 0] + s[:, 1] - 3.0 * s[:, 0] * s[:, 1]
    assert y.tolist() == [-5.0, 3.0, 3.0, -1.0]
    f = E.mc_factorial((nominal + y)[:, None], None, None, [nominal], keep_coef=True)
    assert f.coef[0].tolist() == [0.0, 1.0, 1.0, -3.0] and f.corner_hi[0] == 0b11 and f.m_hi[0] == nominal - 1.0
    assert (nominal + y).max() == nominal + 3.0 and sorted(np.flatnonzero(y == y.max()).tolist()) == [1, 2]
    assert f.corner_lo[0] == 0 and f.m_lo[0] == nominal - 5.0 and f.var[0] == 11.0
    assert f.first[0].tolist() == [1.0 / 11.0] * 2 and f.total[0].tolist() == [10.0 / 11.0] * 2
    stats = np.zeros(1, E.MC_STATS_DTYPE)
    stats["max"], stats["argmax"], stats["min"], stats["argmin"] = nominal + 3.0, 1, nominal - 5.0, 0
    f.stats = stats
    w = f.worst_case(0)
    assert (w["max"], w["argmax"], w["m_hi"], w["corner_hi"], w["hi_is_linear"]) == (nominal + 3.0, 1, nominal - 1.0, 3, False)
    assert (w["min"], w["argmin"], w["m_lo"], w["corner_lo"], w["lo_is_linear"]) == (nominal - 5.0, 0, nominal - 5.0, 0, True)


# ---- Parseval -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", range(1, 13))
def test_var_is_the_population_variance_over_the_corners(kc):
    N = 1 << kc
    m, flags, ok, nominal = rows_of_f(kc, 3)
    got, want = E.mc_factorial(m, flags, ok, nominal), reference(kc, 3)
    for i in range(3):
        y = m[:, i] - nominal[i]
        bar = (4 * kc + N / 256 + 16) * 2.0 ** -53 * float(np.max(y * y))
        for name, var in (("restatement", float(want[0]["var"][i])), ("host", float(got.var[i]))):
            print(name, "kc", kc, "record", i, "var", var, "numpy", float(np.var(y)), "diff", abs(var - float(np.var(y))), "bar", bar)
            assert abs(var - float(np.var(y))) <= bar, (name, kc, i)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def raw(m, flags, ok, nominal, n_corner, n_meas, outs):
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    return E.lib().ezpz_mc_factorial(ptr(m), ptr(flags), ptr(ok), ptr(nominal), n_corner, n_meas, *(ptr(o) for o in outs))


def test_every_argument_error_leaves_the_outputs_untouched():
    m, flags, ok, nominal = rows_of_f(3, 3)
    fresh = lambda: [np.full(4096, 7, np.uint8) for _ in range(8)]  # noqa: E731
    cases = [dict(n_corner=0), dict(n_corner=21), dict(n_meas=0), dict(n_meas=33), dict(m=None), dict(nominal=None)]
    cases += [dict(missing=o) for o in range(7)]
    for case in cases:
        outs = fresh()
        a = dict(m=m, flags=flags, ok=ok, nominal=nominal, n_corner=3, n_meas=3)
        missing = case.pop("missing", None)
        a.update(case)
        given = [None if o == missing else v for o, v in enumerate(outs)]
        assert raw(a["m"], a["flags"], a["ok"], a["nominal"], a["n_corner"], a["n_meas"], given) == ERR_INVALID_ARGUMENT, (case, missing)
        assert all(np.all(o == 7) for o in outs), (case, missing)
    # flags, ok and coef may be NULL
    outs = fresh()
    assert raw(m, None, None, nominal, 3, 3, outs[:7] + [None]) == 0 and np.all(outs[7] == 7) and not np.all(outs[0] == 7)
    with pytest.raises(ValueError):
        E.mc_factorial(np.zeros((3, 1)), None, None, [0.0])  # (not a power of two)
    with pytest.raises(ValueError):
        E.mc_factorial(np.zeros((1, 1)), None, None, [0.0])  # (kc == 0)
    # the three refusals, in both forms, before anything else is looked at
    for other in (dict(contributors=True), dict(quantiles=[0.5]), dict(effects=E.EffectsConfig())):
        with pytest.raises(ValueError):
            E.System.tolerance_mc(None, None, None, None, None, 1, factorial=True, **other)
    for other in (dict(moments_ptr=1), dict(quantiles=[0.5]), dict(effects=E.EffectsConfig())):
        with pytest.raises(ValueError):
            E.System.tolerance_mc_device(None, 0, None, None, None, 1, 0, 0, factorial=True, **other)
