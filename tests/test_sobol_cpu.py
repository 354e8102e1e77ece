"""Sobol tolerance indices, what can be checked without a device: the closing step (ezpz_mc_sobol_indices) and the host reduction
(ezpz_mc_sobol_sums) against tests/sobol_ref.py bit for bit, a FIXED column's +0.0 entries, the indices' meaning on synthetic
functions whose indices are known in closed form, the ABI -- symbols, signatures, layouts, defaults, every argument error by its
return code -- and, through the oracle alone, the band of complete samples the GPU test's triangle is chosen for.

Bars.  Against the restatement: bytes.  Meaning: six standard errors, the convention of tests/test_tolerance_mc_cpu.py, the
standard error computed here from the leaves with numpy; first_var and total_var against this file's own value at 1e-9 relative
(the two differ by the order of a few sums of 2e4 terms: ~1e-13).

Closed forms.  X_j independent, uniform on [-h_j, h_j]: mean 0, variance s_j^2 = h_j^2 / 3.
  additive   Y = a_1 X_1 + a_2 X_2 + a_3 X_3:  V = sum a_j^2 s_j^2;  V_j = Var(E[Y | X_j]) = a_j^2 s_j^2;  first_j = total_j = V_j / V.
  product    Y = X_1 + X_2 + c X_1 X_2 + 0 X_3:  the three terms are uncorrelated (E[X_1^2 X_2] = 0 ..), so V = s_1^2 + s_2^2 + c^2 s_1^2
             s_2^2;  E[Y | X_1] = X_1, so first_1 = s_1^2 / V;  Var(Y | X_2, X_3) = (1 + c X_2)^2 s_1^2, whose mean is s_1^2 (1 + c^2
             s_2^2), so total_1 = s_1^2 (1 + c^2 s_2^2) / V;  symmetrically for 2;  first_3 = total_3 = 0 exactly (the leaves are 0)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ezpz_amd as E
import mc_ref
import sobol_ref as R
from ezpz_amd._lib import EXPORTS, CSobolConfig
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARGUMENT = -103

RUN_ARGS = ["sys", "x0", "positions", "n_param", "dist", "nominal", "records", "n_meas", "samples", "mc", "cfg", "sobol", "stats", "totals", "sums",
            "n_complete", "var", "first", "total", "first_var", "total_var", "keep_f", "keep_flags", "keep_ok"]
RUN_ARGS_DEV = ["sys", "x0_dev", "positions", "n_param", "dist", "nominal", "records", "n_meas", "samples", "mc", "cfg", "sobol", "stats_dev",
                "totals_dev", "sums_dev", "n_complete_dev", "var_dev", "first_dev", "total_dev", "first_var_dev", "total_var_dev", "keep_f_dev",
                "keep_flags_dev", "keep_ok_dev", "stream"]
SIGNATURES = {
    "ezpz_mc_sobol_indices": ["sums", "n_complete", "n_param", "n_meas", "var", "first", "total", "first_var", "total_var"],
    "ezpz_mc_sobol_sums": ["f", "flags", "ok", "nominal_m", "fixed_mask", "samples", "n_param", "n_meas", "chunk", "sums", "n_complete"],
    "ezpz_mc_sobol_sums_device": ["f_dev", "flags_dev", "ok_dev", "nominal_m_dev", "fixed_mask", "samples", "n_param", "n_meas", "chunk", "sums_dev",
                                  "n_complete_dev", "stream"],
    "ezpz_system_tolerance_sobol": RUN_ARGS,
    "ezpz_system_tolerance_sobol_device": RUN_ARGS_DEV,
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
    assert "ezpz_default_sobol_config" in EXPORTS and re.search(r"void ezpz_default_sobol_config\(EzpzSobolConfig\* sobol\);", header)
    for text in ("typedef struct EzpzSobolConfig { /* 16 bytes */", "#define EZPZ_SOBOL_MAX 32u"):
        assert text in header, text
    assert C.sizeof(CSobolConfig) == 16 and R.SOBOL_MAX == 32
    sc = CSobolConfig(7, 7)
    L.ezpz_default_sobol_config(C.byref(sc))
    assert (sc.seed_b, sc.reserved) == (0x9E3779B97F4A7C15, 0) and R.SEED_B == sc.seed_b
    L.ezpz_default_sobol_config(None)
    for name in ("SobolIndices", "SobolResult", "mc_sobol_sums", "mc_sobol_indices"):
        assert name in E.__all__ and hasattr(E, name)
    assert hasattr(E.System, "tolerance_sobol") and hasattr(E.System, "tolerance_sobol_device")
    assert R.width(3) == 16


# ---- synthetic rows with every cause of an incomplete sample, each in rows 0, 1 and 2 + j -------------------------------------------
CAUSES = [(cause, where) for cause in range(4) for where in range(3)]  # ok = 0 | flag bit 0 | NaN | +inf, in row 0 | 1 | 2 + j


def rows_of(k, m, samples, fixed_mask=0):
    """(f, flags, ok, nominal_m): measurements that answer to three matrices of draws; sample b has the cause CAUSES[b % 29] (none
    from 12 on) in record b % m and, for the third place, in row 2 + b % k."""
    rng = np.random.default_rng(10000 * k + 100 * m + samples)
    nominal_m = rng.uniform(-5.0, 5.0, m)
    f = nominal_m + rng.normal(size=(samples, k + 2, m)) * rng.uniform(0.01, 0.3, m)
    for j in range(k):
        if (fixed_mask >> j) & 1:
            f[:, 2 + j] = f[:, 0]
    flags = (rng.integers(0, 2, (samples, k + 2, m)) * 2).astype(np.uint8)  # (bit 1: not the guard's)
    ok = np.ones((samples, k + 2), np.uint8)
    for b in range(samples):
        if b % 29 >= len(CAUSES):
            continue
        cause, where = CAUSES[b % 29]
        r, i = (0, 1, 2 + b % k if k else 1)[where], b % m
        if cause == 0:
            ok[b, r] = 0
        elif cause == 1:
            flags[b, r, i] |= 1
        else:
            f[b, r, i] = np.nan if cause == 2 else np.inf
    return f, flags, ok, nominal_m


SUM_SHAPES = [(k, m, s, mask) for (k, m, mask) in ((0, 1, 0), (3, 2, 0b010)) for s in (1, 255, 256, 257, 1000)]


@pytest.mark.parametrize("k,m,samples,mask", SUM_SHAPES)
def test_the_host_reduction_is_the_stated_sums(k, m, samples, mask):
    f, flags, ok, nominal_m = rows_of(k, m, samples, mask)
    want, want_n = R.sums(f, flags, ok, nominal_m, mask)
    got, got_n = E.mc_sobol_sums(f, flags, ok, nominal_m, mask)
    assert got_n.tolist() == want_n.tolist() and got.tobytes() == want.tobytes(), (got, want)
    if samples >= 255:
        assert np.all(want_n > 0) and np.all(want_n < samples)  # (the causes are there, and do not take everything)
        # a cause in a FIXED dimension's row does not count: the same rows with that dimension solved lose more samples
        if mask:
            assert np.all(R.sums(f, flags, ok, nominal_m, 0)[1] < want_n)
    if samples == 257:  # flags == NULL: every bit clear; ok == NULL: every one set
        want2, n2 = R.sums(f, None, None, nominal_m, mask)
        got2, got_n2 = E.mc_sobol_sums(f, None, None, nominal_m, mask)
        assert got_n2.tolist() == n2.tolist() and np.all(n2 > want_n) and got2.tobytes() == want2.tobytes()


def test_a_fixed_column_is_written_as_plus_zero():
    rng = np.random.default_rng(5)
    k, m, samples = 3, 2, 300
    nominal_m = np.array([1.0, -2.0])
    f = nominal_m - rng.uniform(0.1, 0.5, (samples, k + 2, m))  # every dB is negative
    f[:, 2 + 1] = f[:, 0]  # dimension 1 is FIXED: its row is a copy of A's, t = +0.0, dB * t = -0.0
    assert np.all(f[:, 1] - nominal_m < 0.0)
    got, n = E.mc_sobol_sums(f, None, None, nominal_m, 0b010)
    want, _ = R.sums(f, None, None, nominal_m, 0b010)
    assert got.tobytes() == want.tobytes() and n.tolist() == [samples] * m
    zero = np.zeros(1).tobytes()
    for i in range(m):
        for c in range(4):
            assert got[i, 4 + c * k + 1:4 + c * k + 2].tobytes() == zero, (i, c)
    # summed instead (the dimension not declared FIXED) every leaf of that column of P is -0.0; the blocks are added from +0.0, so
    # the entry is +0.0 again -- and the restatement's bits either way
    summed, _ = E.mc_sobol_sums(f, None, None, nominal_m, 0)
    assert summed.tobytes() == R.sums(f, None, None, nominal_m, 0)[0].tobytes() and summed[0, 4 + 1:4 + 2].tobytes() == zero
    ind = E.mc_sobol_indices(got, n)
    assert ind.first[:, 1].tobytes() == ind.total[:, 1].tobytes() == ind.first_var[:, 1].tobytes() == np.zeros(m).tobytes()


# ---- the closing step against the restatement --------------------------------------------------------------------------------------
def closing_case(k, m, n_complete, constant=None, fixed=None, seed=0):
    rng = np.random.default_rng(seed + 100 * k + m)
    s = np.zeros((m, R.width(k)))
    n = np.full(m, n_complete, np.uint64)
    for i in range(m):
        nn = max(float(n[i]), 1.0)
        var = rng.uniform(0.01, 2.0)
        s[i, 0], s[i, 1] = rng.normal(size=2) * np.sqrt(var * nn)
        s[i, 2], s[i, 3] = var * nn + s[i, 0] ** 2 / nn, var * nn + s[i, 1] ** 2 / nn
        for j in range(k):
            share = rng.uniform(0.0, 1.0)
            s[i, 4 + j] = share * var * nn + rng.normal() * 0.01
            s[i, 4 + k + j] = 2.0 * rng.uniform(share, 1.0) * var * nn
            s[i, 4 + 2 * k + j] = 3.0 * var * var * nn
            s[i, 4 + 3 * k + j] = 20.0 * var * var * nn
        if fixed is not None and k:
            s[i, 4 + fixed::k] = 0.0
    if constant is not None:
        s[constant, :] = 0.0  # every deviation 0: a variance of exactly 0
    return s, n


@pytest.mark.parametrize("k,m", [(0, 1), (1, 1), (3, 2), (32, 32)])
def test_the_closing_step_is_the_stated_one(k, m):
    cases = [closing_case(k, m, 1000), closing_case(k, m, 1000, fixed=0 if k else None), closing_case(k, m, 500, constant=m - 1),
             closing_case(k, m, 0), closing_case(k, m, 1), closing_case(k, m, 2)]
    mixed_s, mixed_n = closing_case(k, m, 700, seed=9)
    mixed_n[0] = 1  # (per record: one with too few samples beside others with enough)
    cases.append((mixed_s, mixed_n))
    for which, (s, n) in enumerate(cases):
        want = R.indices(s, n)
        got = E.mc_sobol_indices(s, n)
        for name, w in zip(("var", "first", "total", "first_var", "total_var"), want):
            assert getattr(got, name).tobytes() == w.tobytes(), (which, name)
    s, n = cases[0]
    got = E.mc_sobol_indices(s, n)
    assert np.isfinite(got.var).all() and np.isfinite(got.first).all() and np.isfinite(got.total_var).all()
    for few in (3, 4, 5):  # n_complete of 0, 1, 2
        got = E.mc_sobol_indices(*cases[few])
        nan = few < 5
        assert np.isnan(got.var).all() == nan and (k == 0 or (np.isnan(got.first).all() == nan and np.isnan(got.total_var).all() == nan))
    got = E.mc_sobol_indices(*cases[2])  # the constant record: a variance of 0, NaN indices; the others untouched by it
    assert got.var[m - 1] == 0.0 and np.isnan(got.first[m - 1]).all() and np.isnan(got.total[m - 1]).all()
    assert np.isfinite(got.first[: m - 1]).all()
    if k:
        got = E.mc_sobol_indices(*cases[1])
        assert not got.first[:, 0].any() and not got.total[:, 0].any() and not got.first_var[:, 0].any()
    assert np.isnan(E.mc_sobol_indices(mixed_s, mixed_n).var[0]) and (m == 1 or np.isfinite(E.mc_sobol_indices(mixed_s, mixed_n).var[1:]).all())


# ---- meaning: functions whose indices are known in closed form ---------------------------------------------------------------------
H = np.array([0.3, 0.5, 0.2])  # X_j uniform on [-h_j, h_j]
COEF = np.array([1.0, -0.7, 2.0])
C_PROD = 3.0
N_SYN = 20000


def synthetic_rows():
    rng = np.random.default_rng(2026)
    A, B = rng.uniform(-H, H, (N_SYN, 3)), rng.uniform(-H, H, (N_SYN, 3))

    def y(X):
        return np.stack([X @ COEF, X[:, 0] + X[:, 1] + C_PROD * X[:, 0] * X[:, 1]], axis=1)

    rows = [y(A), y(B)]
    for j in range(3):
        AB = A.copy()
        AB[:, j] = B[:, j]
        rows.append(y(AB))
    nominal_m = np.array([0.25, -1.5])  # (the functions' values at X = 0, moved off 0)
    return np.stack(rows, axis=1) + nominal_m, nominal_m


def closed_forms():
    s2 = H * H / 3.0
    add = COEF ** 2 * s2
    V = s2[0] + s2[1] + C_PROD ** 2 * s2[0] * s2[1]
    first = np.array([add / add.sum(), [s2[0] / V, s2[1] / V, 0.0]])
    total = np.array([add / add.sum(), [s2[0] * (1 + C_PROD ** 2 * s2[1]) / V, s2[1] * (1 + C_PROD ** 2 * s2[0]) / V, 0.0]])
    return first, total


def test_meaning_on_functions_with_known_indices():
    f, nominal_m = synthetic_rows()
    sums, n = E.mc_sobol_sums(f, None, None, nominal_m)
    assert n.tolist() == [N_SYN, N_SYN]
    ind = E.mc_sobol_indices(sums, n)
    want_first, want_total = closed_forms()
    assert np.all(want_total[1, :2] > want_first[1, :2] + 0.05)  # (the product term is no small thing here)
    d = f - nominal_m
    dA, dB = d[:, 0], d[:, 1]
    both = np.concatenate([dA, dB])
    var = both.var(axis=0, ddof=1)
    assert np.max(np.abs(ind.var / var - 1.0)) <= 1e-9
    for j in range(3):
        t = d[:, 2 + j] - dA
        p, q = dB * t, t * t / 2.0
        for name, leaves, want in (("first", p, want_first[:, j]), ("total", q, want_total[:, j])):
            est, est_var = getattr(ind, name)[:, j], getattr(ind, name + "_var")[:, j]
            own_var = leaves.var(axis=0, ddof=1) / N_SYN / var ** 2
            se = np.sqrt(own_var)
            print(name, j, "estimate", est, "closed form", want, "standard error", se)
            assert np.all(np.abs(est - want) <= 6.0 * se), (name, j)
            assert np.all(np.abs(leaves.mean(axis=0) / var - est) <= 1e-9 * np.maximum(np.abs(est), 1e-3))
            live = own_var > 0.0
            assert np.all(np.abs(est_var[live] / own_var[live] - 1.0) <= 1e-9), (name, j)
            assert np.all(est_var[~live] == 0.0)
    assert not ind.first[1, 2] and not ind.total[1, 2] and np.all(ind.interaction[1, :2] > 0.05)
    assert np.allclose(ind.first_se ** 2, ind.first_var) and np.allclose(ind.total_se ** 2, ind.total_var)


# ---- every argument error: the return code, no output touched -----------------------------------------------------------------------
def test_argument_errors():
    L = E.lib()
    k, m, samples = 2, 2, 10
    f, flags, ok, nominal_m = rows_of(k, m, samples)
    sums, n = np.full((m, R.width(k)), 7.0), np.full(m, 7, np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731

    def reduce(f_=f, nominal_=nominal_m, mask=0, samples_=samples, k_=k, m_=m, sums_=sums, n_=n):
        return L.ezpz_mc_sobol_sums(None if f_ is None else p(f_), p(flags), p(ok), None if nominal_ is None else p(nominal_), mask, samples_, k_, m_,
                                    0, None if sums_ is None else p(sums_), None if n_ is None else p(n_))

    assert reduce(k_=33) == ERR_INVALID_ARGUMENT and reduce(m_=0) == ERR_INVALID_ARGUMENT and reduce(m_=33) == ERR_INVALID_ARGUMENT
    assert reduce(mask=0b100) == ERR_INVALID_ARGUMENT  # (a bit at or above k)
    for missing in ("f_", "nominal_", "sums_", "n_"):
        assert reduce(**{missing: None}) == ERR_INVALID_ARGUMENT, missing
        assert reduce(samples_=0, **{missing: None}) == 0, missing
    assert np.all(sums == 7.0) and np.all(n == 7)
    assert reduce(samples_=0) == 0 and np.all(sums == 7.0) and np.all(n == 7)  # samples == 0: nothing written
    assert reduce() == 0 and not np.any(sums == 7.0)
    with pytest.raises(E.NonLinearSystemError) as e:
        E.mc_sobol_sums(np.zeros((3, 35, 1)), None, None, np.zeros(1))
    assert e.value.code == ERR_INVALID_ARGUMENT
    # the closing step
    outs = [np.full(m, 7.0)] + [np.full((m, k), 7.0) for _ in range(4)]

    def close(sums_=sums, n_=n, k_=k, m_=m, missing=None):
        return L.ezpz_mc_sobol_indices(None if sums_ is None else p(sums_), None if n_ is None else p(n_), k_, m_,
                                       *(None if w == missing else p(a) for w, a in enumerate(outs)))

    assert close(k_=33) == ERR_INVALID_ARGUMENT and close(m_=0) == ERR_INVALID_ARGUMENT and close(m_=33) == ERR_INVALID_ARGUMENT
    assert close(sums_=None) == ERR_INVALID_ARGUMENT and close(n_=None) == ERR_INVALID_ARGUMENT
    for missing in range(5):
        assert close(missing=missing) == ERR_INVALID_ARGUMENT, missing
    assert all(np.all(a == 7.0) for a in outs)
    assert close() == 0 and not any(np.any(a == 7.0) for a in outs)
    one = np.full(1, 7.0)
    assert L.ezpz_mc_sobol_indices(p(np.zeros(4)), p(np.zeros(1, np.uint64)), 0, 1, p(one), None, None, None, None) == 0 and np.isnan(one[0])
    with pytest.raises(ValueError):
        E.mc_sobol_indices(np.zeros((2, 7)), np.zeros(2, np.uint64))


# ---- the triangle of tests/test_gpu_contributors.py: how many pick-freeze samples assemble, by the oracle alone ----------------------
# Its third side (1.9 +- 0.3) outgrows the other two (1 +- 0.05 each) for about a third of the draws.  Pick-freeze needs all k + 2 = 5
# variants of a sample to assemble: A and the two AB_j that keep A's third side (about 2 / 3), B and AB_2 with B's (about 2 / 3,
# independently): about 4 / 9 of the samples, inside the band of 10 % to 90 % with TRI_DISTS as they are.
A_, B_, C_ = (0, 1), (2, 3), (4, 5)
TRI_POS, TRI_NOMINAL = [3, 4, 5], np.array([1.0, 1.0, 1.9])
TRI_DISTS = [(mc_ref.UNIFORM, -0.05, 0.05), (mc_ref.UNIFORM, -0.05, 0.05), (mc_ref.UNIFORM, -0.3, 0.3)]
TRI_SAMPLES, TRI_SEED = 600, 0xC0FFEE1234
TRI_START = np.array([[0.0, 0.0, 1.0, 0.0, 0.9, 0.4]])


def triangle(sides):
    return O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(3, 0.0), O.distance(A_, B_, float(sides[0])), O.distance(B_, C_, float(sides[1])),
                    O.distance(C_, A_, float(sides[2]))])


def triangle_complete_by_the_oracle():
    """[samples] bool: all five variants of the sample assemble, each solved by the oracle from the nominal solution."""
    rc, x0, _, conv, nun = O.solve_batch(triangle(TRI_NOMINAL), TRI_START)
    assert rc == 0 and conv[0] and nun[0] == 0
    dists = [E.McDist(*t) for t in TRI_DISTS]
    PA = E.mc_sample(TRI_SEED, dists, TRI_NOMINAL, 0, TRI_SAMPLES)
    PB = E.mc_sample(TRI_SEED ^ R.SEED_B, dists, TRI_NOMINAL, 0, TRI_SAMPLES)
    assert PA.tobytes() == mc_ref.sample(TRI_SEED, TRI_DISTS, TRI_NOMINAL, 0, TRI_SAMPLES).tobytes()
    done = np.ones(TRI_SAMPLES, bool)
    for b in range(TRI_SAMPLES):
        variants = [PA[b], PB[b]] + [np.where(np.arange(3) == j, PB[b], PA[b]) for j in range(3)]
        for sides in variants:
            rc, _, _, conv, nun = O.solve_batch(triangle(sides), x0)
            done[b] = done[b] and rc == 0 and bool(conv[0]) and nun[0] == 0
            if not done[b]:
                break
    return done


def test_the_triangles_complete_samples_stay_inside_the_band():
    done = triangle_complete_by_the_oracle()
    share = done.sum() / TRI_SAMPLES
    print("complete pick-freeze samples of the triangle by the oracle:", int(done.sum()), "of", TRI_SAMPLES)
    assert 0.10 <= share <= 0.90
