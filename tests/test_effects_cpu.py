"""Monte-Carlo main effects, what can be checked without a device: the host reduction (ezpz_mc_effects) and the closing step
(ezpz_mc_effect_indices) against tests/effects_ref.py bit for bit, the bin rule at its special places, the cells' counts against
n_valid, the ABI -- symbols, signatures, layouts, defaults, every argument error by its return code with no output touched -- the
equiprobable edges, and the estimator's meaning on ezpz_mc_sample's own draws.

Bars.  Against the restatement: bytes.  Meaning: an all-fixed system answers x = p, so the record p_a - p_b is computed here from the
draws; the dimensions are uniform with widths 0.4 and 0.2 and a third the record does not read, 4096 samples, 8 equiprobable (equal-
width) bins.  The first-order indices are 0.8, 0.2 and 0, and equal-width bins keep 1 - 1 / 64 of a linear effect (include/ezpz_amd.h).
The bar is five standard deviations of each estimate, MEASURED over 64 seeds of ezpz_mc_sample's draws through effects_ref in the
test itself; measured when the test was written: 0.0038, 0.0115 and 0.0012 (a numpy simulation with its own generator had given
0.004, 0.011 and 0.001), the means over the seeds 0.7874, 0.1968 and 0.0003 against 0.7875, 0.1969 and 0."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import effects_cases as cases
import effects_ref as R
import ezpz_amd as E
from ezpz_amd._lib import EXPORTS, CMcEffectConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARGUMENT = -103

MC_ARGS = ["sys", "x0", "positions", "n_param", "dist", "nominal", "records", "n_meas", "lim_lo", "lim_hi", "hist_lo", "hist_hi", "samples", "mc", "cfg"]
RUN_ARGS = MC_ARGS + ["stats", "totals", "hist", "keep_params", "keep_m", "keep_flags", "keep_ok", "ec", "edges", "sums", "counts", "cond_mean",
                      "cond_var", "eta2", "first", "bins_used"]
RUN_ARGS_DEV = ["sys", "x0_dev"] + MC_ARGS[2:] + ["stats_dev", "totals_dev", "hist_dev", "keep_params_dev", "keep_m_dev", "keep_flags_dev", "keep_ok_dev",
                                                  "ec", "edges", "sums_dev", "counts_dev", "cond_mean_dev", "cond_var_dev", "eta2_dev", "first_dev",
                                                  "bins_used_dev", "stream"]
SIGNATURES = {
    "ezpz_mc_effect_indices": ["sums", "counts", "nominal_m", "n_param", "n_meas", "bins", "cond_mean", "cond_var", "eta2", "first", "bins_used"],
    "ezpz_mc_effects": ["params", "m", "flags", "ok", "nominal_m", "edges", "samples", "n_param", "n_meas", "bins", "chunk", "sums", "counts"],
    "ezpz_mc_effects_device": ["params_dev", "m_dev", "flags_dev", "ok_dev", "nominal_m_dev", "edges_dev", "samples", "n_param", "n_meas", "bins", "chunk",
                               "sums_dev", "counts_dev", "stream"],
    "ezpz_system_tolerance_mc_effects": RUN_ARGS,
    "ezpz_system_tolerance_mc_effects_device": RUN_ARGS_DEV,
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
    assert "ezpz_default_mc_effect_config" in EXPORTS and re.search(r"void ezpz_default_mc_effect_config\(EzpzMcEffectConfig\* ec\);", header)
    for text in ("typedef struct EzpzMcEffectConfig { /* 8 bytes */", "#define EZPZ_MC_EFFECT_MAX_BINS 64u", "#define EZPZ_MC_EFFECT_MAX_CELLS 4096u"):
        assert text in header, text
    assert C.sizeof(CMcEffectConfig) == 8 and (R.MAX_DIM, R.MAX_BINS, R.MAX_CELLS) == (32, 64, 4096)
    ec = CMcEffectConfig(7, 7)
    L.ezpz_default_mc_effect_config(C.byref(ec))
    assert (ec.bins, ec.reserved) == (8, 0) and E.EffectsConfig().bins == 8 and E.EffectsConfig().edges is None
    L.ezpz_default_mc_effect_config(None)
    for name in ("EffectsConfig", "McEffects", "mc_effects", "mc_effect_indices", "mc_effect_edges"):
        assert name in E.__all__ and hasattr(E, name)
    assert hasattr(E.System, "tolerance_mc") and "effects" in E.System.tolerance_mc.__code__.co_varnames
    assert "effect_sums_ptr" in E.System.tolerance_mc_device.__code__.co_varnames


# ---- the host reduction against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,B,samples", cases.SHAPES)
def test_the_host_reduction_is_the_stated_cells(k, m, B, samples):
    a = p, y, flags, ok, nominal_m, edges = cases.case(k, m, B, samples)
    want, want_n = cases.reference(k, m, B, samples)
    got, got_n = E.mc_effects(*a)
    assert got.shape == (k, B, m, 2) and got_n.shape == (k, B, m) and got_n.dtype == np.uint64
    assert got_n.tobytes() == want_n.tobytes() and got.tobytes() == want.tobytes()
    # for every dimension the bins' counts add up to the record's n_valid
    n_valid = R.valid(y, flags, ok).sum(axis=0)
    assert np.all(got_n.sum(axis=1) == n_valid[None, :])
    if samples >= 255:
        assert np.all(n_valid > 0) and np.all(n_valid < samples)  # (the causes are there, and do not take everything)
        if B >= 3:
            assert not got_n[0, 1].any() and got_n[0, 0].any() and got_n[0, 2].any()  # (the repeated edge: bin 1 stays empty)
        if k >= 2:
            assert not got_n[k - 1, 2:].any() and got_n[k - 1, 0].any() and got_n[k - 1, 1].any()  # (+inf edges: the upper bins stay empty)
        if k >= 3:
            assert np.all(got_n[1, 0] == n_valid) and not got_n[1, 1:].any()  # (all +inf: one bin)
    if samples == 257:  # flags == NULL: every bit clear; ok == NULL: every one set; the rounds of the host form change nothing
        want2, n2 = R.effects(p, y, None, None, nominal_m, edges)
        got2, got_n2 = E.mc_effects(p, y, None, None, nominal_m, edges, chunk=256)
        assert got_n2.tobytes() == n2.tobytes() and got2.tobytes() == want2.tobytes() and got_n2.sum() > got_n.sum()


def test_the_bin_rule_at_its_special_places():
    """One record that counts every sample (d = 1): the counts are the bins.  A value on an edge goes up; -0.0 and +0.0 are the same
    value to an edge at -0.0 and to one at +0.0; -inf and +inf edges; all +inf; a NaN value lands in bin 0; a repeated edge."""
    inf, nan = np.inf, np.nan
    edges = np.array([[-1.0, 0.5, 0.5], [-0.0, 0.0, inf], [inf, inf, inf], [-inf, -inf, 2.0]])
    values = [-2.0, -1.0, np.nextafter(-1.0, -inf), 0.5, np.nextafter(0.5, -inf), -0.0, 0.0, 5e-324, -5e-324, 2.0, inf, -inf, nan]
    p = np.repeat(np.array(values)[:, None], 4, axis=1)
    y, nominal_m = np.ones((len(values), 1)), np.zeros(1)
    sums, counts = E.mc_effects(p, y, None, None, nominal_m, edges)
    want, want_n = R.effects(p, y, None, None, nominal_m, edges)
    assert sums.tobytes() == want.tobytes() and counts.tobytes() == want_n.tobytes()
    assert R.bins_of(p, edges).T.tolist() == [[0, 1, 0, 3, 1, 1, 1, 1, 1, 3, 3, 0, 0], [0, 0, 0, 2, 2, 2, 2, 2, 0, 2, 3, 0, 0], [0] * 10 + [3, 0, 0],
                                              [2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 2, 0]]
    assert counts[:, :, 0].tolist() == [[4, 6, 0, 3], [6, 0, 6, 1], [12, 0, 0, 1], [1, 0, 10, 2]]
    assert sums[:, :, 0, 0].tolist() == counts[:, :, 0].astype(float).tolist() == sums[:, :, 0, 1].tolist()
    ind = E.mc_effect_indices(sums, counts, nominal_m, edges)
    assert ind.bins_used[0].tolist() == [3, 3, 2, 3]


# ---- the closing step against the restatement ----------------------------------------------------------------------------------------
def closing_cases():
    out = []
    for shape in ((2, 1, 4, 1000), (8, 8, 64, 257), (32, 32, 4, 257), (1, 1, 2, 1)):
        sums, counts = cases.reference(*shape)
        out.append((sums, counts, cases.case(*shape)[4]))
    # a constant record (every d the same: SST == 0 exactly), a record whose every cell holds one sample (N - used == 0), cells of one
    # and of two samples beside full ones, a dimension in one bin (used == 1) and a record without a valid sample (used == 0)
    k, B, m = 3, 4, 5
    rng = np.random.default_rng(3)
    counts = rng.integers(5, 50, (k, B, m)).astype(np.uint64)
    mean, spread = rng.normal(size=(k, B, m)), rng.uniform(0.1, 1.0, (k, B, m))
    n = counts.astype(float)
    sums = np.stack([n * mean, n * (mean * mean + spread)], axis=-1)
    counts[:, :, 0], sums[:, :, 0, 0], sums[:, :, 0, 1] = 8, 8 * 0.25, 8 * 0.0625
    counts[:, :, 1], sums[:, :, 1, 1] = 1, sums[:, :, 1, 0] ** 2
    counts[0, 1, 2], sums[0, 1, 2] = 1, (mean[0, 1, 2], mean[0, 1, 2] ** 2)
    counts[0, 2, 2], sums[0, 2, 2] = 2, (2 * mean[0, 2, 2], 2 * (mean[0, 2, 2] ** 2 + spread[0, 2, 2]))
    counts[1, 1:, :], sums[1, 1:, :, :] = 0, 0.0
    counts[:, :, 4], sums[:, :, 4, :] = 0, 0.0
    out.append((sums, counts, rng.normal(size=m)))
    return out


def test_the_closing_step_is_the_stated_one():
    names = ("cond_mean", "cond_var", "eta2", "first", "bins_used")
    for which, (sums, counts, nominal_m) in enumerate(closing_cases()):
        want = R.indices(sums, counts, nominal_m)
        got = E.mc_effect_indices(sums, counts, nominal_m)
        for name, w in zip(names, want):
            assert getattr(got, name).dtype == w.dtype and getattr(got, name).tobytes() == w.tobytes(), (which, name)
    got = E.mc_effect_indices(sums, counts, nominal_m)  # the crafted case
    zero, nan = np.zeros(1).tobytes(), lambda a: bool(np.isnan(a).all())  # noqa: E731
    assert got.eta2[0, 0] != got.eta2[0, 0] and nan(got.eta2[0, [0, 2]]) and nan(got.first[0, [0, 2]])  # SST == 0
    assert nan(got.eta2[1, [0, 2]]) and nan(got.cond_var[:, :, 1]) and np.isfinite(got.cond_mean[[0, 2], :, 1]).all()  # n_c == 1 everywhere
    assert got.bins_used[:, 1].tolist() == [1, 1, 1, 1, 0] and got.bins_used[4].tolist() == [0, 0, 0]
    for i in range(5):  # used < 2: +0.0, whatever the record
        assert got.eta2[i, 1:2].tobytes() == zero and got.first[i, 1:2].tobytes() == zero
    assert got.eta2[4].tobytes() == np.zeros(3).tobytes() and nan(got.cond_mean[:, :, 4])
    assert np.isnan(got.cond_var[0, 1, 2]) and np.isfinite(got.cond_var[0, 2, 2]) and np.isfinite(got.cond_mean[0, 1, 2])
    assert np.isfinite(got.eta2[2:4, [0, 2]]).all() and np.all(got.first[2:4, [0, 2]] < got.eta2[2:4, [0, 2]])


# ---- every argument error: the return code, no output touched -----------------------------------------------------------------------
def test_argument_errors():
    L = E.lib()
    k, m, B, samples = 2, 3, 4, 10
    prm, y, flags, ok, nominal_m, edges = cases.case(k, m, B, samples)
    sums, counts = np.full((k, B, m, 2), 7.0), np.full((k, B, m), 7, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def reduce(prm_=prm, y_=y, nominal_=nominal_m, edges_=edges, samples_=samples, k_=k, m_=m, B_=B, sums_=sums, counts_=counts):
        return L.ezpz_mc_effects(p(prm_), p(y_), p(flags), p(ok), p(nominal_), p(edges_), samples_, k_, m_, B_, 0, p(sums_), p(counts_))

    for bad in (dict(k_=0), dict(m_=0), dict(k_=33), dict(m_=33), dict(B_=1), dict(B_=0), dict(B_=65), dict(k_=32, m_=32, B_=5), dict(k_=8, m_=9, B_=64)):
        assert reduce(**bad) == ERR_INVALID_ARGUMENT and reduce(samples_=0, **bad) == ERR_INVALID_ARGUMENT, bad
    for name, e in (("NaN", [[0.0, np.nan, 1.0], [0.0, 1.0, 2.0]]), ("decreasing", [[0.0, 1.0, 2.0], [0.0, 1.0, 0.5]]), ("-inf last", [[0.0, 1.0, -np.inf]] * 2)):
        assert reduce(edges_=np.array(e)) == ERR_INVALID_ARGUMENT and reduce(edges_=np.array(e), samples_=0) == ERR_INVALID_ARGUMENT, name
    for missing in ("prm_", "y_", "nominal_", "edges_", "sums_", "counts_"):
        assert reduce(**{missing: None}) == ERR_INVALID_ARGUMENT, missing
        assert reduce(samples_=0, **{missing: None}) == 0, missing
    assert np.all(sums == 7.0) and np.all(counts == 7)
    assert reduce(samples_=0) == 0 and np.all(sums == 7.0) and np.all(counts == 7)  # samples == 0: nothing written
    assert reduce(edges_=np.array([[-np.inf, 0.0, 0.0], [1.0, np.inf, np.inf]])) == 0 and not np.any(sums == 7.0)
    with pytest.raises(E.NonLinearSystemError) as e:
        E.mc_effects(np.zeros((3, 33)), np.zeros((3, 1)), None, None, np.zeros(1), np.zeros((33, 1)))
    assert e.value.code == ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        E.mc_effects(np.zeros((3, 2)), np.zeros((3, 1)), None, None, np.zeros(1), np.zeros((3, 1)))
    # the closing step
    sums, counts = E.mc_effects(prm, y, flags, ok, nominal_m, edges)
    outs = [np.full((k, B, m), 7.0), np.full((k, B, m), 7.0), np.full((m, k), 7.0), np.full((m, k), 7.0), np.full((m, k), 7, np.uint32)]

    def close(sums_=sums, counts_=counts, nominal_=nominal_m, k_=k, m_=m, B_=B, missing=None):
        return L.ezpz_mc_effect_indices(p(sums_), p(counts_), p(nominal_), k_, m_, B_, *(None if w == missing else p(a) for w, a in enumerate(outs)))

    for bad in (dict(k_=0), dict(m_=0), dict(k_=33), dict(m_=33), dict(B_=1), dict(B_=65), dict(k_=32, m_=32, B_=5)):
        assert close(**bad) == ERR_INVALID_ARGUMENT, bad
    assert close(sums_=None) == ERR_INVALID_ARGUMENT and close(counts_=None) == ERR_INVALID_ARGUMENT and close(nominal_=None) == ERR_INVALID_ARGUMENT
    for missing in range(5):
        assert close(missing=missing) == ERR_INVALID_ARGUMENT, missing
    assert all(np.all(a == 7) for a in outs)
    assert close() == 0 and not any(np.any(a == 7) for a in outs)
    with pytest.raises(ValueError):
        E.mc_effect_indices(np.zeros((2, 4, 3)), np.zeros((2, 4, 3), np.uint64), np.zeros(3))


# ---- the equiprobable edges ------------------------------------------------------------------------------------------------------------
def test_equiprobable_edges_from_the_distributions():
    from statistics import NormalDist

    D = E.McDist
    dists = [D.uniform(-0.2, 0.6), D.normal(0.1), D.normal(0.2, 1.5), D.corner(-0.1, 0.3), D.fixed(), D.normal(0.0), D.uniform(0.1, 0.1), D.corner(0.2, 0.2)]
    nominal = np.arange(8) * 1.5 - 3.0
    B = 8
    edges = E.mc_effect_edges(dists, nominal, B)
    assert edges.shape == (8, B - 1) and np.all(np.diff(edges[:3], axis=1) > 0.0)
    assert edges[0].tolist() == [nominal[0] - 0.2 + 0.8 * c / B for c in range(1, B)]
    nd = NormalDist()
    assert edges[1].tolist() == [nominal[1] + 0.1 * nd.inv_cdf(c / B) for c in range(1, B)]
    lo, hi = nd.cdf(-1.5), nd.cdf(1.5)
    assert edges[2].tolist() == [nominal[2] + 0.2 * nd.inv_cdf(lo + (hi - lo) * c / B) for c in range(1, B)]
    assert np.all(np.abs(edges[2] - nominal[2]) < 0.2 * 1.5) and edges[2, 3] == nominal[2]
    assert edges[3].tolist() == [nominal[3] + 0.1] + [np.inf] * (B - 2)
    assert np.all(edges[4:] == np.inf)
    # equiprobable on the sampler's own draws: every bin of a varying dimension holds about samples / bins
    n = 8000
    p = E.mc_sample(11, dists[:3], nominal[:3], 0, n)
    which = R.bins_of(p, edges[:3])
    for j in range(3):
        got = np.bincount(which[:, j], minlength=B)
        assert np.all(np.abs(got - n / B) <= 6.0 * np.sqrt(n / B * (1 - 1 / B))), (j, got)  # (binomial: six standard deviations)


# ---- meaning: ezpz_mc_sample's draws through the rule ----------------------------------------------------------------------------------
MEAN_DISTS = [(E.McDist.UNIFORM, -0.2, 0.2), (E.McDist.UNIFORM, -0.1, 0.1), (E.McDist.UNIFORM, -0.15, 0.15)]
MEAN_NOMINAL = np.array([2.0, -1.25, 0.5])
MEAN_SAMPLES, MEAN_BINS, MEAN_SEEDS = 4096, 8, 64


def difference_run(seed, estimate):
    """first and eta2 [3] of the record p_0 - p_1 on the draws of `seed`: what an all-fixed system answers, x = p."""
    dists = [E.McDist(*t) for t in MEAN_DISTS]
    p = E.mc_sample(seed, dists, MEAN_NOMINAL, 0, MEAN_SAMPLES)
    y = (p[:, 0] - p[:, 1])[:, None]
    nominal_m = np.array([MEAN_NOMINAL[0] - MEAN_NOMINAL[1]])
    edges = E.mc_effect_edges(dists, MEAN_NOMINAL, MEAN_BINS)
    return estimate(p, y, nominal_m, edges)


def by_the_reference(p, y, nominal_m, edges):
    sums, counts = R.effects(p, y, None, None, nominal_m, edges)
    _, _, eta2, first, used = R.indices(sums, counts, nominal_m)
    assert used.tolist() == [[MEAN_BINS] * 3]
    return first[0], eta2[0]


def by_the_library(p, y, nominal_m, edges):
    ind = E.mc_effect_indices(*E.mc_effects(p, y, None, None, nominal_m, edges), nominal_m, edges)
    return ind.first[0], ind.eta2[0]


def test_meaning_on_the_samplers_own_draws():
    runs = [difference_run(1000 + s, by_the_reference) for s in range(MEAN_SEEDS)]
    first, eta2 = np.array([r[0] for r in runs]), np.array([r[1] for r in runs])
    sd, mean = first.std(axis=0, ddof=1), first.mean(axis=0)
    keep = 1.0 - 1.0 / MEAN_BINS ** 2
    want = np.array([0.8 * keep, 0.2 * keep, 0.0])
    print("first over", MEAN_SEEDS, "seeds: mean", mean, "standard deviation", sd, "expected", want)
    got_first, got_eta2 = difference_run(1000, by_the_library)
    assert got_first.tobytes() == first[0].tobytes() and got_eta2.tobytes() == eta2[0].tobytes()
    print("first of the library's run", got_first, "eta2", got_eta2)
    assert np.all(sd > 0.0) and np.all(np.abs(got_first - want) <= 5.0 * sd), (got_first, want, sd)
    assert np.all(np.abs(mean - want) <= 5.0 * sd / np.sqrt(MEAN_SEEDS)), (mean, want, sd)  # (the estimator itself, not one run)
    # the dimension the record does not read: the raw ratio is biased upward, the corrected one straddles zero
    assert np.all(eta2[:, 2] > 0.0) and first[:, 2].min() < 0.0 < first[:, 2].max()
    assert abs(eta2[:, 2].mean() - (MEAN_BINS - 1) / (MEAN_SAMPLES - 1)) <= 5.0 * eta2[:, 2].std(ddof=1) / np.sqrt(MEAN_SEEDS)


def test_the_curve_of_a_result():
    dists = [E.McDist(*t) for t in MEAN_DISTS]
    p = E.mc_sample(5, dists, MEAN_NOMINAL, 0, 2048)
    y = (1.0 + (p[:, 0] - MEAN_NOMINAL[0]) ** 2)[:, None]
    nominal_m = np.ones(1)
    edges = E.mc_effect_edges(dists, MEAN_NOMINAL, 8)
    sums, counts = E.mc_effects(p, y, None, None, nominal_m, edges)
    bounds = np.array([[n + a, n + b] for (_, a, b), n in zip(MEAN_DISTS, MEAN_NOMINAL)])
    inner = E.mc_effect_indices(sums, counts, nominal_m, edges)
    whole = E.mc_effect_indices(sums, counts, nominal_m, edges, bounds=bounds)
    centres, means, n = inner.curve(0, 0)
    assert len(centres) == 6 and centres.tolist() == ((edges[0, :-1] + edges[0, 1:]) / 2).tolist() and n.tolist() == counts[0, 1:7, 0].tolist()
    centres, means, n = whole.curve(0, 0)
    assert len(centres) == 8 and n.sum() == 2048 and means.tolist() == whole.cond_mean[0, :, 0].tolist()
    assert np.all(np.abs(means - (1.0 + (centres - MEAN_NOMINAL[0]) ** 2)) <= 0.05 ** 2)  # (a parabola: the bin mean lies within width^2 / 4 ..)
    assert means[0] > means[3] and means[7] > means[4] and whole.first[0, 0] > 0.8 and abs(whole.first[0, 1]) < 0.05
