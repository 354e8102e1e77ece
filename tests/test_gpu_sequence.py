"""GPU tests (-m gpu) of the low-discrepancy draws (include/ezpz_amd.h: THE SEQUENCE; csrc/mc_sequence.hip.hpp and the walking
sampler kernel of csrc/tolerance_mc.hip.hpp): a run with flagged dimensions draws what ezpz_mc_sample and tests/sequence_ref.py
draw, cutting it into rounds changes no byte -- the walk restarts at every round and at every grid stride and must give the bits
of the direct evaluation -- every reduction downstream takes the flagged samples as it takes plain ones, the Sobol indices refuse
them, and the solution branches start from them.  A 16-variable system, all Fixed, every parameter driven; every case is small.

The samples here start at 0: a flagged dimension's last samples, near 2^32, can only be reached on the host (a run that far would
be 2^32 solves) -- tests/test_sequence_cpu.py draws them through ezpz_mc_sample, whose body is the device's.

Bars.  keep_params against ezpz_mc_sample and the reference: bitwise for everything but the NORMAL draws off the central branch of
the inverse (and the plain NORMAL draws); those: 1e-13 * sigma + 2^-52 * |p|, the bar of tests/test_tolerance_mc_cpu.py (log and sqrt
differ in their last bits between the host and the device).  Everything else: bytes."""
import ctypes as C

import numpy as np
import pytest

import branch_ref
import mc_ref as R
import sequence_ref as Q
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
N16 = 16
SEED = 0x5E0B01C0FFEE
_rng = np.random.default_rng(7)
X16 = _rng.uniform(0.5, 3.0, N16) * _rng.choice([-1.0, 1.0], N16) + np.arange(N16) * 0.37  # the nominal values, and the nominal solution
POS16 = list(range(N16))
# (kind, a, b, flagged) per dimension: flagged UNIFORM, flagged NORMAL without and with a truncation, and every kind unflagged
DISTS16 = [[(R.UNIFORM, -0.2, 0.2, 1), (R.NORMAL, 0.1, 0.0, 1), (R.NORMAL, 0.15, 1.5, 1), (R.UNIFORM, -0.1, 0.3, 0), (R.NORMAL, 0.1, 2.0, 0),
            (R.CORNER, -0.1, 0.1, 0), (R.FIXED, 0.0, 0.0, 0)][j % 7] for j in range(N16)]
RECORDS12 = O.stack([
    O.vertical_distance((0, 1), (2, 6), 0.0), O.horizontal_distance((5, 6), (7, 8), 0.0), O.vertical_distance((10, 11), (12, 15), 0.0),
    O.horizontal_distance((2, 3), (13, 0), 0.0), O.fixed(7, 0.0), O.fixed(6, 0.0),
    O.distance((0, 1), (2, 3), 0.0), O.distance((5, 6), (10, 11), 0.0), O.point_line_distance((0, 1), (5, 6), (12, 13), 0.0),
    O._mk(O.ARC_LENGTH, [0, 1, 5, 6, 10, 11], 0.0), O._mk(O.LINES_AT_ANGLE, [0, 1, 2, 3, 5, 6, 7, 8], 0.0, tag=O.ANGLE_OTHER_RAD),
    O._mk(O.POINTS_AT_ANGLE, [10, 11, 12, 13, 14, 15], 0.0, tag=O.ANGLE_OTHER_DEG)])
N12 = len(RECORDS12)
_CACHE = {}


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


def dists_of(E, tuples):
    return [E.McDist(*t) for t in tuples]


def system16(E):
    if "s16" not in _CACHE:
        _CACHE["s16"] = E.System(O.stack([O.fixed(v, float(X16[v])) for v in range(N16)]), N16)
    return _CACHE["s16"]


def ranges(E):
    if "nom" not in _CACHE:
        _CACHE["nom"] = system16(E).measure(X16[None, :], RECORDS12)[0]
    nom = _CACHE["nom"]
    return (nom - 0.03, nom + 0.04), (nom - 0.05, nom + 0.08, 16)


def run16(E, samples, chunk=0, **kw):
    key = ("run", samples, chunk, tuple(sorted(kw)))
    if key not in _CACHE:
        limits, hist = ranges(E)
        _CACHE[key] = system16(E).tolerance_mc(X16, POS16, dists_of(E, DISTS16), RECORDS12, samples, seed=SEED, limits=limits, hist=hist,
                                               chunk=chunk, keep=True, **kw)
    return _CACHE[key]


def result_bytes(res):
    return [res.stats.tobytes(), res.totals.tobytes(), res.hist.tobytes(), res.params.tobytes(), res.m.tobytes(), res.flags.tobytes(), res.ok.tobytes()]


def assert_draws(got, want, central):
    assert got.shape == want.shape
    assert got[central].tobytes() == want[central].tobytes()
    sigma = np.array([d[1] if d[0] == R.NORMAL else 0.0 for d in DISTS16])
    assert np.all(np.abs(got - want) <= 1e-13 * sigma + 2.0 ** -52 * np.abs(want))


def test_600_samples_are_the_host_samplers_and_the_references(E):
    res = run16(E, 600)  # two blocks and a part; 75 runs of the walk for every dimension
    want, central = Q.sample(SEED, DISTS16, X16, 0, 600)
    flagged_normal = [j for j, d in enumerate(DISTS16) if d[3] and d[0] == R.NORMAL]
    assert all(0.7 * 600 <= central[:, j].sum() < 600 for j in flagged_normal)  # (both branches of the inverse are drawn)
    assert_draws(res.params, want, central)
    assert_draws(res.params, E.mc_sample(SEED, dists_of(E, DISTS16), X16, 0, 600), central)
    assert res.ok.all() and res.n_ok == 600  # (a Fixed system takes every value)
    limits, hist = ranges(E)
    stats, totals, counts = R.statistics(res.m, res.flags, res.ok, res.nominal, limits, hist)
    for f in R.STATS_DTYPE.names:
        assert res.stats[f].tobytes() == stats[f].tobytes(), f
    assert res.totals.tobytes() == totals.tobytes() and res.hist.tobytes() == counts.tobytes()
    # the option of the run flags every UNIFORM and NORMAL dimension of the call, and the default none
    every = system16(E).tolerance_mc(X16, POS16, dists_of(E, DISTS16), RECORDS12, 300, seed=SEED, keep=True, sampling="sequence")
    want_every = E.mc_sample(SEED, [E.McDist(k, a, b, k in (R.UNIFORM, R.NORMAL)) for k, a, b, _ in DISTS16], X16, 0, 300)
    assert_draws(every.params, want_every, Q.sample(SEED, [(k, a, b, 1) for k, a, b, _ in DISTS16], X16, 0, 300)[1])
    assert every.params[:, 3].tobytes() != res.params[:300, 3].tobytes() and every.params[:, 0].tobytes() == res.params[:300, 0].tobytes()


def test_cutting_the_run_changes_no_byte_nor_does_another_stream(E):
    import torch

    whole = result_bytes(run16(E, 1000, chunk=0))
    assert result_bytes(run16(E, 1000, chunk=256)) == whole  # (rounds of 256: 32 runs of the walk each; the last one has 232 samples)
    s = system16(E)
    limits, hist = ranges(E)
    x0 = torch.from_numpy(X16).cuda()
    out = lambda n: torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")  # noqa: E731
    stats, totals, counts = out(N12 * 88), out(24), out(N12 * 18 * 8)
    kp, km, kf, ko = out(1000 * N16 * 8), out(1000 * N12 * 8), out(1000 * N12), out(1000)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s.tolerance_mc_device(x0.data_ptr(), POS16, dists_of(E, DISTS16), RECORDS12, 1000, stats.data_ptr(), totals.data_ptr(), counts.data_ptr(),
                              seed=SEED, limits=limits, hist=hist, chunk=256, keep_params_ptr=kp.data_ptr(), keep_m_ptr=km.data_ptr(),
                              keep_flags_ptr=kf.data_ptr(), keep_ok_ptr=ko.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert [t.cpu().numpy().tobytes() for t in (stats, totals, counts, kp, km, kf, ko)] == whole


def test_a_round_larger_than_the_grid(E):
    # The sampler's grid is capped at 16 workgroups a compute unit -- 1 048 576 work items on 256 units -- and a work item is 8 samples
    # of one dimension: one round of 150 016 samples x 64 dimensions is 1 200 128 of them, so some threads take a second trip.
    n, samples = 64, 150016
    x0 = np.arange(n) * 0.25
    s = E.System(O.stack([O.fixed(v, float(x0[v])) for v in range(n)]), n)
    dists = [E.McDist.uniform(-0.5, 0.5, sequence=True)] * n
    records = O.stack([O.horizontal_distance((0, 1), (62, 63), 0.0)])
    one = s.tolerance_mc(x0, list(range(n)), dists, records, samples, seed=SEED, chunk=samples, keep=True)
    assert one.params.tobytes() == E.mc_sample(SEED, dists, x0, 0, samples).tobytes()
    cut = s.tolerance_mc(x0, list(range(n)), dists, records, samples, seed=SEED, keep=True)  # (rounds of 65 536: inside the grid)
    assert result_bytes_no_hist(cut) == result_bytes_no_hist(one) and one.n_ok == samples


def result_bytes_no_hist(res):
    return [res.stats.tobytes(), res.totals.tobytes(), res.params.tobytes(), res.m.tobytes(), res.flags.tobytes(), res.ok.tobytes()]


def test_contributors_of_flagged_samples(E):
    res = run16(E, 600, contributors=True)
    assert result_bytes(res) == result_bytes(run16(E, 600))
    moments, n_complete = E.mc_moments(res.params, res.m, res.flags, res.ok, X16, res.nominal)
    assert res.moments.tobytes() == moments.tobytes() and res.n_complete == n_complete and n_complete >= 500
    host, c = E.mc_contributors(res.moments, res.n_complete, N16, N12), res.contributors
    for name in ("cov", "beta", "contrib", "r2"):
        assert getattr(c, name).tobytes() == getattr(host, name).tobytes(), name
    assert c.dropped == host.dropped == sum(1 << j for j, d in enumerate(DISTS16) if d[0] == R.FIXED)


def test_quantiles_of_flagged_samples(E):
    probs = [0.0, 0.01, 0.5, 0.99865, 1.0]
    res = run16(E, 600, quantiles=probs)
    assert result_bytes(res) == result_bytes(run16(E, 600))
    assert res.quantiles.tobytes() == E.mc_quantiles(res.m, res.flags, res.ok, probs, 0.0).tobytes()


def test_effects_of_flagged_samples(E):
    res = run16(E, 600, effects=E.EffectsConfig(8))
    assert result_bytes(res) == result_bytes(run16(E, 600))
    e = res.effects
    sums, counts = E.mc_effects(res.params, res.m, res.flags, res.ok, res.nominal, e.edges)
    assert e.sums.tobytes() == sums.tobytes() and e.counts.tobytes() == counts.tobytes()
    host = E.mc_effect_indices(e.sums, e.counts, res.nominal)
    for name in ("cond_mean", "cond_var", "eta2", "first", "bins_used"):
        assert getattr(e, name).tobytes() == getattr(host, name).tobytes(), name
    # equiprobable bins of a flagged dimension are filled evenly.  Dimension 0 is UNIFORM, its 8 bins are the intervals of width 1/8
    # of u, and a shift keeps the net: samples 0 .. 511 put 64 in each, 512 .. 575 another 8, and the last 24 fall one to an
    # interval of width 1/32, at most four to a bin -- 72 .. 76 (a plain run's counts scatter by sqrt(600 * 7 / 64) = 8)
    counts = e.counts[0, :, 0].astype(np.int64)
    assert counts.sum() == 600 and counts.min() >= 72 and counts.max() <= 76, counts


def test_the_sobol_indices_refuse_flagged_dimensions(E):
    import sobol_ref
    from ezpz_amd._lib import CMcConfig, CSobolConfig
    from ezpz_amd.api import mc_dists

    s, K, M = system16(E), 4, 3
    flagged = [E.McDist.uniform(-0.1, 0.1), E.McDist.normal(0.1, 0.0, sequence=True), E.McDist.fixed(), E.McDist.uniform(-0.1, 0.1)]
    plain = [E.McDist.uniform(-0.1, 0.1), E.McDist.normal(0.1), E.McDist(R.FIXED, 0.0, 0.0, True), E.McDist.uniform(-0.1, 0.1)]
    with pytest.raises(E.NonLinearSystemError) as err:
        s.tolerance_sobol(X16, POS16[:K], flagged, RECORDS12[:M], 300, seed=SEED)
    assert err.value.code == ERR_INVALID_ARGUMENT
    pos = np.array(POS16[:K], np.uint32)
    outs = {"stats": np.full(M * 88, 0xA5, np.uint8), "totals": np.full(24, 0xA5, np.uint8), "sums": np.full(M * sobol_ref.width(K), 7.0),
            "n_complete": np.full(M, 7, np.uint64), "var": np.full(M, 7.0), "first": np.full(M * K, 7.0), "total": np.full(M * K, 7.0),
            "first_var": np.full(M * K, 7.0), "total_var": np.full(M * K, 7.0)}
    before = {name: a.copy() for name, a in outs.items()}
    cfg, recs = E.Config()._c(), np.ascontiguousarray(RECORDS12[:M])

    def call(dists):
        d, mc, sc = mc_dists(dists), CMcConfig(SEED, 0, 0), CSobolConfig(SEED + 1, 0)
        return E.lib().ezpz_system_tolerance_sobol(s._h, X16.ctypes.data, pos.ctypes.data, K, d.ctypes.data, None, recs.ctypes.data, M, 300,
                                                   C.byref(mc), C.byref(cfg), C.byref(sc), *(a.ctypes.data for a in outs.values()), None, None, None)

    assert call(flagged) == ERR_INVALID_ARGUMENT
    assert all(a.tobytes() == before[name].tobytes() for name, a in outs.items())
    assert call(plain) == 0 and outs["n_complete"].tolist() == [300] * M  # (the flag on a FIXED dimension is ignored)


def test_the_branches_start_from_flagged_draws(E):
    f = branch_ref.blocks(3)
    system = E.System(f.records, f.n_vars)
    dists = [E.McDist(k, a, b, True) for k, a, b in f.spread(3.0)]
    samples, seed = 512, 11
    got = system.solve_branches(f.x0, dists, samples, seed=seed, keep=True)
    starts = E.mc_sample(seed, dists, f.x0, 0, samples)
    assert starts.tobytes() != E.mc_sample(seed, [E.McDist(*t) for t in f.spread(3.0)], f.x0, 0, samples).tobytes()
    starts[0] = f.x0
    x, st = system.solve_batch(starts)[:2]
    want = branch_ref.cluster_batch(x[None], branch_ref.ok_of(st["converged"], st["n_unsatisfied"])[None], origin=np.asarray(f.x0)[None], status=st[None])
    have = [np.ascontiguousarray(a).tobytes() for a in (got.info, got.branches, got.x, got.labels)]
    for what, g, w in zip(("info", "branches", "x_branch", "labels"), have, branch_ref.result_bytes(*want)):
        assert g == w, what
    assert got.info["n_branches"][0] == 8 and got.info["n_ok"][0] >= 0.9 * samples
