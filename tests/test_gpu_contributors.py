"""GPU tests (-m gpu) of the tolerance contributors (ezpz_mc_moments, ezpz_system_tolerance_mc_contrib and their _device forms;
csrc/mc_moments.hip, csrc/tolerance_mc.hip): the moments are the sums tests/contrib_ref.py states, bit for bit; cutting the
reduction into rounds or moving it to another stream changes no byte; the run with contributors is the plain run byte for byte,
its moments are the reduction alone on its kept samples and its closing kernel is the host's closing step; and the answers mean
what they say on the device's own samples.  Every case is small: the shapes are the edges of a block of 256 samples and of a
round, not a workload.

Bars.  Everything but the meaning: bytes.  beta and cov against numpy.linalg.lstsq (with an intercept) and numpy.cov over the kept
complete samples: 1e-9 of the largest magnitude of the array compared -- the bar of tests/test_contributors_cpu.py, there derived
(independent draws, a condition number of the input block below 10 -- asserted here too --, normal equations that lose ~1e-13).
Records that are differences of two driven coordinates: beta = +-1 and r2 = 1 within 1e-4.  That one is a SANITY bar, not a derived
one: the solve stops at a residual of 1e-8 while the dimensions vary by 0.1, so about 1e-7 is expected."""
import numpy as np
import pytest

import contrib_ref as R
import mc_ref
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
SEED = 0xC0FFEE1234
_CACHE = {}


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


# ---- the moments alone: synthetic samples with every cause of an incomplete one ---------------------------------------------------
def samples_of(k, m, samples, all_incomplete=False):
    """(params, m, flags, ok, nominal_p, nominal_m): references that answer to the inputs, and incomplete samples sprinkled in by
    each cause -- ok = 0, flag bit 0, NaN m, +inf m (flag bits other than 0 do not count)."""
    key = ("samples", k, m, samples, all_incomplete)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * k + 10 * m + samples)
        nominal_p, nominal_m = rng.uniform(-5.0, 5.0, k), rng.uniform(-5.0, 5.0, m)
        p = nominal_p + rng.normal(size=(samples, k)) * rng.uniform(0.01, 0.3, k)
        A = rng.normal(size=(m, k))
        y = nominal_m + (p - nominal_p) @ A.T + 0.05 * rng.normal(size=(samples, m))
        flags = (rng.integers(0, 2, (samples, m)) * 2).astype(np.uint8)  # (bit 1: not the guard's)
        ok = np.ones(samples, np.uint8)
        for b in range(samples):
            cause, i = b % (4 if all_incomplete else 11), b % m  # (causes 4 .. 10: a complete sample)
            if cause == 0:
                ok[b] = 0
            elif cause == 1:
                flags[b, i] |= 1
            elif cause == 2:
                y[b, i] = np.nan
            elif cause == 3:
                y[b, i] = np.inf
        _CACHE[key] = (p, y, flags, ok, nominal_p, nominal_m)
    return _CACHE[key]


def reference_moments(k, m, samples, all_incomplete=False):
    key = ("ref", k, m, samples, all_incomplete)
    if key not in _CACHE:
        _CACHE[key] = R.moments(*samples_of(k, m, samples, all_incomplete))
    return _CACHE[key]


SHAPES = [(k, m, s) for (k, m) in ((0, 1), (2, 1)) for s in (1, 255, 256, 257, 1000)] + [(32, 32, 257)]


@pytest.mark.parametrize("k,m,samples", SHAPES)
def test_the_moments_are_the_stated_sums(E, k, m, samples):
    a = samples_of(k, m, samples)
    want, n_complete = reference_moments(k, m, samples)
    got, got_n = E.mc_moments(*a)
    assert got_n == n_complete and got.tobytes() == want.tobytes(), (got, want)
    if samples >= 255:
        assert 0 < n_complete < samples  # (the causes are there, and do not take everything)
    # flags == NULL: every bit clear; ok == NULL: every one set
    p, y, flags, ok, nominal_p, nominal_m = a
    if samples == 257:
        want2, n2 = R.moments(p, y, None, None, nominal_p, nominal_m)
        got2, got_n2 = E.mc_moments(p, y, None, None, nominal_p, nominal_m)
        assert got_n2 == n2 > n_complete and got2.tobytes() == want2.tobytes()


def test_every_sample_incomplete(E):
    a = samples_of(2, 1, 300, all_incomplete=True)
    want, n_complete = reference_moments(2, 1, 300, all_incomplete=True)
    got, got_n = E.mc_moments(*a)
    assert n_complete == 0 and got_n == 0 and got.tobytes() == want.tobytes() == np.zeros(R.entries(3)).tobytes()
    c = E.mc_contributors(got, got_n, 2, 1)
    assert c.dropped == R.UINT64_MAX and np.isnan(c.cov).all() and np.isnan(c.r2).all()


def test_rounds_and_streams_change_no_byte(E):
    import torch

    p, y, flags, ok, nominal_p, nominal_m = a = samples_of(2, 1, 1000)
    want, n_complete = reference_moments(2, 1, 1000)
    for chunk in (256, 512, 300, 0):  # (300 rounds up to 512)
        got, got_n = E.mc_moments(*a, chunk=chunk)
        assert got_n == n_complete and got.tobytes() == want.tobytes(), chunk
    dev = [torch.from_numpy(v).cuda() for v in a]
    moments = torch.full((R.entries(3),), 7.0, dtype=torch.float64, device="cuda")
    info = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for chunk in (256, 0):
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_mc_moments_device(*(t.data_ptr() for t in dev), 1000, 2, 1, chunk, moments.data_ptr(), info.data_ptr(), stream.cuda_stream)
        assert rc == 0
        stream.synchronize()
        assert moments.cpu().numpy().tobytes() == want.tobytes() and info.cpu().tolist() == [1000, n_complete], chunk
    # an argument error of the device form: nothing enqueued, no output touched
    moments.fill_(7.0)
    rc = E.lib().ezpz_mc_moments_device(*(t.data_ptr() for t in dev), 1000, 60, 5, 0, moments.data_ptr(), info.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == ERR_INVALID_ARGUMENT and bool((moments == 7.0).all())


# ---- the run: a 16-variable system, all Fixed, every parameter driven; a dozen records of linear and curved kinds -----------------
N16 = 16
_rng = np.random.default_rng(7)
X16 = _rng.uniform(0.5, 3.0, N16) * _rng.choice([-1.0, 1.0], N16) + np.arange(N16) * 0.37  # the nominal values, and the nominal solution
POS16 = list(range(N16))
# (kind, a, b) per dimension: mixed kinds; the FIXED dimensions are 4, 9, 14, the CORNER ones 3, 8, 13
DISTS16 = [[(mc_ref.UNIFORM, -0.2, 0.2), (mc_ref.NORMAL, 0.1, 0.0), (mc_ref.NORMAL, 0.15, 1.5), (mc_ref.CORNER, -0.1, 0.1),
            (mc_ref.FIXED, 0.0, 0.0)][j % 5] for j in range(N16)]
FIXED_DIMS = [j for j in range(N16) if DISTS16[j][0] == mc_ref.FIXED]
# records 0 .. 3: differences of two driven coordinates (record, the variable with +-1, the other one)
DIFFERENCES = [(O.vertical_distance((0, 1), (2, 6), 0.0), 1, 6), (O.horizontal_distance((5, 6), (7, 8), 0.0), 5, 7),
               (O.vertical_distance((10, 11), (12, 15), 0.0), 11, 15), (O.horizontal_distance((2, 3), (13, 0), 0.0), 2, 13)]
RECORDS12 = O.stack([d[0] for d in DIFFERENCES] + [
    O.fixed(7, 0.0), O.fixed(4, 0.0),  # (the second reads a FIXED dimension: a constant reference dimension)
    O.distance((0, 1), (2, 3), 0.0), O.distance((5, 6), (10, 11), 0.0), O.point_line_distance((0, 1), (5, 6), (12, 13), 0.0),
    O._mk(O.ARC_LENGTH, [0, 1, 5, 6, 10, 11], 0.0), O._mk(O.LINES_AT_ANGLE, [0, 1, 2, 3, 5, 6, 7, 8], 0.0, tag=O.ANGLE_OTHER_RAD),
    O._mk(O.POINTS_AT_ANGLE, [10, 11, 12, 13, 14, 15], 0.0, tag=O.ANGLE_OTHER_DEG)])
N12 = len(RECORDS12)


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


def run16(E, chunk, contributors):
    key = ("run", chunk, contributors)
    if key not in _CACHE:
        limits, hist = ranges(E)
        _CACHE[key] = system16(E).tolerance_mc(X16, POS16, dists_of(E, DISTS16), RECORDS12, 1000, seed=SEED, limits=limits, hist=hist,
                                               chunk=chunk, keep=True, contributors=contributors)
    return _CACHE[key]


def plain_bytes(res):
    return [res.stats.tobytes(), res.totals.tobytes(), res.hist.tobytes(), res.params.tobytes(), res.m.tobytes(), res.flags.tobytes(),
            res.ok.tobytes()]


def contrib_bytes(c):
    return [c.cov.tobytes(), c.beta.tobytes(), c.contrib.tobytes(), c.r2.tobytes(), np.uint64(c.dropped).tobytes()]


def complete_of(res):
    return (res.ok != 0) & ~((res.flags & 1) != 0).any(axis=1) & np.isfinite(res.m).all(axis=1)


@pytest.mark.parametrize("chunk", [0, 256])
def test_the_run_with_contributors(E, chunk):
    res, plain = run16(E, chunk, True), run16(E, chunk, False)
    assert plain_bytes(res) == plain_bytes(plain) and not hasattr(plain, "moments")
    moments, n_complete = E.mc_moments(res.params, res.m, res.flags, res.ok, X16, res.nominal)
    assert res.moments.tobytes() == moments.tobytes() and res.n_complete == n_complete
    assert n_complete == int(complete_of(res).sum()) and 900 <= n_complete <= 1000
    host = E.mc_contributors(res.moments, res.n_complete, N16, N12)
    assert contrib_bytes(res.contributors) == contrib_bytes(host)
    assert res.dropped == sum(1 << j for j in FIXED_DIMS) and res.contributors.dropped_mask.nonzero()[0].tolist() == FIXED_DIMS
    assert not res.cov[FIXED_DIMS].any() and not res.beta[:, FIXED_DIMS].any()
    assert np.isnan(res.r2[5]) and np.isnan(res.contrib[5]).all() and np.isfinite(np.delete(res.r2, 5)).all()  # (record 5 is constant)
    varying = np.diag(res.cov) > 0.0
    assert np.all(np.abs(np.diag(res.corr)[varying] - 1.0) <= 1e-15) and np.isnan(np.diag(res.corr)[~varying]).all()
    if chunk == 256:  # cutting the run changes nothing
        whole = run16(E, 0, True)
        assert res.moments.tobytes() == whole.moments.tobytes() and contrib_bytes(res.contributors) == contrib_bytes(whole.contributors)


def test_the_device_form_on_another_stream_equals_the_host_form(E):
    import torch

    s, res = system16(E), run16(E, 256, True)
    limits, hist = ranges(E)
    K = N16 + N12
    x0 = torch.from_numpy(X16).cuda()
    out = lambda n: torch.full((max(n, 1),), 0x5A, dtype=torch.uint8, device="cuda")  # noqa: E731
    stats, totals, counts = out(N12 * 88), out(24), out(N12 * 18 * 8)
    kp, km, kf, ko = out(1000 * N16 * 8), out(1000 * N12 * 8), out(1000 * N12), out(1000)
    moments, info, cov, beta, contrib, r2, dropped = (out(8 * n) for n in (R.entries(K), 2, K * K, N12 * N16, N12 * N16, N12, 1))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s.tolerance_mc_device(x0.data_ptr(), POS16, dists_of(E, DISTS16), RECORDS12, 1000, stats.data_ptr(), totals.data_ptr(), counts.data_ptr(),
                              seed=SEED, limits=limits, hist=hist, chunk=256, keep_params_ptr=kp.data_ptr(), keep_m_ptr=km.data_ptr(),
                              keep_flags_ptr=kf.data_ptr(), keep_ok_ptr=ko.data_ptr(), stream=stream.cuda_stream, moments_ptr=moments.data_ptr(),
                              info_ptr=info.data_ptr(), cov_ptr=cov.data_ptr(), beta_ptr=beta.data_ptr(), contrib_ptr=contrib.data_ptr(),
                              r2_ptr=r2.data_ptr(), dropped_ptr=dropped.data_ptr())
    stream.synchronize()
    raw = lambda t: t.cpu().numpy().tobytes()  # noqa: E731
    assert [raw(t) for t in (stats, totals, counts, kp, km, kf, ko)] == plain_bytes(res)
    assert raw(moments) == res.moments.tobytes() and raw(info) == np.array([1000, res.n_complete], np.uint64).tobytes()
    assert [raw(t) for t in (cov, beta, contrib, r2, dropped)] == contrib_bytes(res.contributors)


def close(got, want, bar):
    return np.max(np.abs(got - want)) <= bar * np.max(np.abs(want))


def test_meaning_on_the_devices_own_samples(E):
    res = run16(E, 0, True)
    done = complete_of(res)
    live = [j for j in range(N16) if j not in FIXED_DIMS]
    p, y = res.params[done][:, live], np.delete(res.m[done], 5, axis=1)
    cov = np.cov(np.concatenate([p, y], axis=1).T)
    assert np.linalg.cond(cov[: len(live), : len(live)]) < 10.0
    X = np.concatenate([p, np.ones((len(p), 1))], axis=1)
    coef, *_ = np.linalg.lstsq(X, y, rcond=None)
    keep = live + [N16 + i for i in range(N12) if i != 5]
    assert close(res.cov[np.ix_(keep, keep)], cov, 1e-9)
    assert close(np.delete(res.beta, 5, axis=0)[:, live], coef[:-1].T, 1e-9)
    # SANITY bar (see the module's text): a difference of two driven coordinates answers to them with +-1 and to nothing else
    for i, (_, a, b) in enumerate(DIFFERENCES):
        want = np.zeros(N16)
        want[a], want[b] = res.beta[i, a] / abs(res.beta[i, a]), res.beta[i, b] / abs(res.beta[i, b])
        assert want[a] == -want[b]
        print("difference record", i, "max |beta - (+-1)|", np.max(np.abs(res.beta[i] - want)), "|r2 - 1|", abs(res.r2[i] - 1.0))
        assert np.max(np.abs(res.beta[i] - want)) <= 1e-4 and abs(res.r2[i] - 1.0) <= 1e-4
    # the curved records are seen as curved, the contributions are shares
    assert np.all(np.delete(res.r2, 5) <= 1.0 + 1e-9) and np.all(np.delete(res.contrib, 5, axis=0) >= 0.0)


# ---- variants that do not assemble: a triangle whose third side can outgrow the other two --------------------------------------
A, B, Cc = (0, 1), (2, 3), (4, 5)
TRIANGLE = O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(3, 0.0), O.distance(A, B, 1.0), O.distance(B, Cc, 1.0), O.distance(Cc, A, 1.9)])
TRI_POS, TRI_NOMINAL = [3, 4, 5], np.array([1.0, 1.0, 1.9])
TRI_DISTS = [(mc_ref.UNIFORM, -0.05, 0.05), (mc_ref.UNIFORM, -0.05, 0.05), (mc_ref.UNIFORM, -0.3, 0.3)]
TRI_MEASURE = O.stack([O.vertical_distance(Cc, A, 0.0), O.distance(B, Cc, 0.0)])


def test_variants_that_do_not_assemble_are_left_out(E):
    rc, x0, _, conv, nun = O.solve_batch(TRIANGLE, np.array([[0.0, 0.0, 1.0, 0.0, 0.9, 0.4]]))
    assert rc == 0 and conv[0] and nun[0] == 0
    s = E.System(TRIANGLE, 6)
    res = s.tolerance_mc(x0[0], TRI_POS, dists_of(E, TRI_DISTS), TRI_MEASURE, 600, seed=SEED, keep=True, contributors=True)
    plain = s.tolerance_mc(x0[0], TRI_POS, dists_of(E, TRI_DISTS), TRI_MEASURE, 600, seed=SEED, keep=True)
    assert plain_bytes_no_hist(res) == plain_bytes_no_hist(plain)
    assert 300 <= res.n_ok <= 500 and not (res.flags & 1).any() and res.n_complete == res.n_ok == int(np.count_nonzero(res.ok))
    want, n_complete = R.moments(res.params, res.m, res.flags, res.ok, TRI_NOMINAL, res.nominal)
    assert n_complete == res.n_complete and res.moments.tobytes() == want.tobytes()  # (the leaves of the failed samples are +0.0)
    assert res.dropped == 0 and np.isfinite(res.beta).all()


def plain_bytes_no_hist(res):
    return [res.stats.tobytes(), res.totals.tobytes(), res.params.tobytes(), res.m.tobytes(), res.flags.tobytes(), res.ok.tobytes()]


# ---- argument errors of the run: the return code, no output touched ---------------------------------------------------------------
def test_argument_errors_of_the_run(E):
    s = system16(E)
    with pytest.raises(E.NonLinearSystemError) as e:
        s.tolerance_mc(X16, POS16, dists_of(E, DISTS16), RECORDS12, 300, contributors=True, pivot_rel=-1.0)
    assert e.value.code == ERR_INVALID_ARGUMENT
    with pytest.raises(E.NonLinearSystemError):
        s.tolerance_mc(X16, POS16, dists_of(E, DISTS16), RECORDS12, 300, contributors=True, pivot_rel=float("nan"))
    # K = 0 and K > 64 (the plain run takes both)
    assert s.tolerance_mc(X16, [], [], RECORDS12[:0], 10).n_ok == 10
    with pytest.raises(E.NonLinearSystemError):
        s.tolerance_mc(X16, [], [], RECORDS12[:0], 10, contributors=True)
    many = O.stack([O.fixed(v % N16, 0.0) for v in range(49)])
    assert s.tolerance_mc(X16, POS16, dists_of(E, DISTS16), many, 10).n_ok == 10
    with pytest.raises(E.NonLinearSystemError):
        s.tolerance_mc(X16, POS16, dists_of(E, DISTS16), many, 10, contributors=True)
    assert s.tolerance_mc(X16, POS16, dists_of(E, DISTS16), many[:48], 10, contributors=True).n_complete == 10  # (K = 64)
    # a NULL output with samples > 0, by the raw entry; samples == 0 with the same arguments is EZPZ_OK and writes nothing
    import ctypes as C

    from ezpz_amd._lib import CMcConfig

    d, recs, pos = E.api.mc_dists(dists_of(E, DISTS16)), RECORDS12, np.arange(N16, dtype=np.uint32)
    K = N16 + N12
    outs = {"moments": np.full(R.entries(K), 7.0), "info": np.full(2, 7, np.uint64), "cov": np.full(K * K, 7.0), "beta": np.full(N12 * N16, 7.0),
            "contrib": np.full(N12 * N16, 7.0), "r2": np.full(N12, 7.0), "dropped": np.full(1, 7, np.uint64)}
    stats, totals = np.full(N12 * 88, 0xA5, np.uint8), np.full(24, 0xA5, np.uint8)
    mc, cfg = CMcConfig(1, 0, 0), E.Config()._c()

    def call(samples, missing):
        return E.lib().ezpz_system_tolerance_mc_contrib(s._h, X16.ctypes.data, pos.ctypes.data, N16, d.ctypes.data, None, recs.ctypes.data, N12, None,
                                                        None, None, None, samples, C.byref(mc), C.byref(cfg), stats.ctypes.data, totals.ctypes.data,
                                                        None, None, None, None, None, None,
                                                        *(None if name == missing else a.ctypes.data for name, a in outs.items()))

    for missing in outs:
        assert call(300, missing) == ERR_INVALID_ARGUMENT, missing
        assert call(0, missing) == 0, missing
    assert all(np.all(a == 7) for a in outs.values()) and np.all(stats == 0xA5) and np.all(totals == 0xA5)
    assert call(300, None) == 0 and outs["info"].tolist()[0] == 300
