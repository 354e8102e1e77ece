"""GPU tests (-m gpu) of the Monte-Carlo main effects (ezpz_mc_effects_device, ezpz_system_tolerance_mc_effects and its _device form;
csrc/mc_effects.hip, csrc/tolerance_mc.hip): the device's cells are the sums and counts tests/effects_ref.py states, bit for bit,
and the host form's; cutting the reduction into rounds or moving it to another stream changes no byte; the run with effects is the
plain run byte for byte, its cells are the reduction alone on its kept samples and its closing kernel is the host's closing step;
and the answers mean what they say on the device's own samples.  Every case is small: the shapes are the edges of a block of 256
samples, of a round and of the cells' limits, not a workload.

Bars.  Everything but the meaning: bytes.  Records that are differences of two driven coordinates: `first` within 1e-4 of the host
reference on ezpz_mc_sample's draws (UNIFORM dimensions: the same bits on both sides).  That one is a SANITY bar, as in
tests/test_gpu_contributors.py: the solve stops at a residual of 1e-8 while the dimensions vary by 0.1, so about 1e-7 is expected.
Against tolerance_sobol: |difference| <= 4 first_se + 0.05, a SANITY bar too -- the 0.05 covers the bins' bias, which nobody has
measured on these records.

The curved case (chosen BEFORE any run).  A point at nominal (1, 0), its x = 1 + u and y = v each a driven dimension, u uniform on
+-0.01 and v on +-0.35: its distance from the origin is ~ 1 + u + v^2 / 2, Var(v^2 / 2) = 0.35^4 / 45 = 3.3e-4 against Var(u) =
3.3e-5, so y causes some 0.9 of the variance -- through curvature alone: the regression's coefficient for y is 0 by symmetry and
its contrib is the squared sample correlation, about 1 / samples = 6e-5.  Sixteen bins: the issue's simulation puts the bins' bias on
such a curve at 0.06 of 0.84 with eight bins and 0.016 with sixteen, and the bar against pick-freeze allows 0.05."""
import ctypes as C

import numpy as np
import pytest

import effects_cases as cases
import effects_ref as R
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


def dists_of(E, tuples):
    return [E.McDist(*t) for t in tuples]


# ---- the reduction alone ---------------------------------------------------------------------------------------------------------------
def device_effects(E, a, chunk, stream=None, shape=None):
    """(rc, sums, counts) of ezpz_mc_effects_device on the case `a`, its outputs poisoned first."""
    import torch

    p, y, flags, ok, nominal_m, edges = a
    k, m, B = shape or (p.shape[1], y.shape[1], edges.shape[1] + 1)
    dev = [None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (p, y, flags, ok, nominal_m, edges)]
    cells = p.shape[1] * (edges.shape[1] + 1) * y.shape[1]
    sums = torch.full((2 * cells,), 7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((cells,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    if stream is None:
        rc = E.lib().ezpz_mc_effects_device(*(ptr(t) for t in dev), len(p), k, m, B, chunk, sums.data_ptr(), counts.data_ptr(), None)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_mc_effects_device(*(ptr(t) for t in dev), len(p), k, m, B, chunk, sums.data_ptr(), counts.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    return rc, sums.cpu().numpy(), counts.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("k,m,B,samples", cases.SHAPES)
def test_the_device_cells_are_the_stated_cells(E, k, m, B, samples):
    import torch

    a = p, y, flags, ok, nominal_m, edges = cases.case(k, m, B, samples)
    want, want_n = cases.reference(k, m, B, samples)
    host, host_n = E.mc_effects(*a)
    assert host.tobytes() == want.tobytes() and host_n.tobytes() == want_n.tobytes()
    rc, got, got_n = device_effects(E, a, 0)
    assert rc == 0 and got_n.tobytes() == want_n.tobytes() and got.tobytes() == want.tobytes()
    rc, got, got_n = device_effects(E, a, 256, torch.cuda.Stream())
    assert rc == 0 and got_n.tobytes() == want_n.tobytes() and got.tobytes() == want.tobytes()
    assert np.all(got_n.reshape(k, B, m).sum(axis=1) == R.valid(y, flags, ok).sum(axis=0)[None, :])
    if samples == 257:  # flags == NULL: every bit clear; ok == NULL: every one set
        want2, n2 = R.effects(p, y, None, None, nominal_m, edges)
        rc, got2, got_n2 = device_effects(E, (p, y, None, None, nominal_m, edges), 0)
        assert rc == 0 and got_n2.tobytes() == n2.tobytes() and got2.tobytes() == want2.tobytes()


def test_rounds_and_streams_change_no_byte(E):
    import torch

    a = cases.case(2, 1, 4, 1000)
    want, want_n = cases.reference(2, 1, 4, 1000)
    stream = torch.cuda.Stream()
    for chunk in (256, 512, 300, 0):  # (300 rounds up to 512)
        for st in (None, stream):
            rc, got, got_n = device_effects(E, a, chunk, st)
            assert rc == 0 and got_n.tobytes() == want_n.tobytes() and got.tobytes() == want.tobytes(), (chunk, st)
    # argument errors of the device form: nothing enqueued, the poisoned outputs untouched
    for shape in ((0, 1, 4), (2, 0, 4), (33, 1, 4), (2, 33, 4), (2, 1, 1), (2, 1, 65), (32, 32, 5)):
        rc, got, got_n = device_effects(E, a, 0, stream, shape=shape)
        assert rc == ERR_INVALID_ARGUMENT and np.all(got == 7.0) and np.all(got_n == 7), shape
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in a]
    sums = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((8,), 7, dtype=torch.int64, device="cuda")
    for missing in range(8):
        if missing in (2, 3):  # (flags and ok may be NULL)
            continue
        ptrs = [t.data_ptr() for t in dev] + [sums.data_ptr(), counts.data_ptr()]
        ptrs[missing] = None
        assert E.lib().ezpz_mc_effects_device(*ptrs[:6], 1000, 2, 1, 4, 0, *ptrs[6:], None) == ERR_INVALID_ARGUMENT, missing
        assert E.lib().ezpz_mc_effects_device(*ptrs[:6], 0, 2, 1, 4, 0, *ptrs[6:], None) == 0, missing
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all()) and bool((counts == 7).all())


# ---- the run: the 16-variable all-Fixed system of tests/test_gpu_contributors.py, rebuilt here ----------------------------------------
N16 = 16
_rng = np.random.default_rng(7)
X16 = _rng.uniform(0.5, 3.0, N16) * _rng.choice([-1.0, 1.0], N16) + np.arange(N16) * 0.37  # the nominal values, and the nominal solution
POS16 = list(range(N16))
# (kind, a, b) per dimension: mixed kinds; the FIXED dimensions are 4, 9, 14, the CORNER ones 3, 8, 13
DISTS16 = [[(mc_ref.UNIFORM, -0.2, 0.2), (mc_ref.NORMAL, 0.1, 0.0), (mc_ref.NORMAL, 0.15, 1.5), (mc_ref.CORNER, -0.1, 0.1),
            (mc_ref.FIXED, 0.0, 0.0)][j % 5] for j in range(N16)]
FIXED_DIMS = [j for j in range(N16) if DISTS16[j][0] == mc_ref.FIXED]
CORNER_DIMS = [j for j in range(N16) if DISTS16[j][0] == mc_ref.CORNER]
LIVE_DIMS = [j for j in range(N16) if j not in FIXED_DIMS and j not in CORNER_DIMS]
# records 0 .. 3: differences of two driven coordinates (record, the two variables)
DIFFERENCES = [(O.vertical_distance((0, 1), (2, 6), 0.0), 1, 6), (O.horizontal_distance((5, 6), (7, 8), 0.0), 5, 7),
               (O.vertical_distance((10, 11), (12, 15), 0.0), 11, 15), (O.horizontal_distance((2, 3), (13, 0), 0.0), 2, 13)]
RECORDS12 = O.stack([d[0] for d in DIFFERENCES] + [
    O.fixed(7, 0.0), O.fixed(4, 0.0),  # (the second reads a FIXED dimension: a constant reference dimension)
    O.distance((0, 1), (2, 3), 0.0), O.distance((5, 6), (10, 11), 0.0), O.point_line_distance((0, 1), (5, 6), (12, 13), 0.0),
    O._mk(O.ARC_LENGTH, [0, 1, 5, 6, 10, 11], 0.0), O._mk(O.LINES_AT_ANGLE, [0, 1, 2, 3, 5, 6, 7, 8], 0.0, tag=O.ANGLE_OTHER_RAD),
    O._mk(O.POINTS_AT_ANGLE, [10, 11, 12, 13, 14, 15], 0.0, tag=O.ANGLE_OTHER_DEG)])
N12 = len(RECORDS12)
BINS16 = 8  # 16 x 8 x 12 = 1536 cells


def system16(E):
    if "s16" not in _CACHE:
        _CACHE["s16"] = E.System(O.stack([O.fixed(v, float(X16[v])) for v in range(N16)]), N16)
    return _CACHE["s16"]


def ranges(E):
    if "nom" not in _CACHE:
        _CACHE["nom"] = system16(E).measure(X16[None, :], RECORDS12)[0]
    nom = _CACHE["nom"]
    return (nom - 0.03, nom + 0.04), (nom - 0.05, nom + 0.08, 16)


def run16(E, chunk, effects):
    key = ("run", chunk, effects)
    if key not in _CACHE:
        limits, hist = ranges(E)
        _CACHE[key] = system16(E).tolerance_mc(X16, POS16, dists_of(E, DISTS16), RECORDS12, 1000, seed=SEED, limits=limits, hist=hist, chunk=chunk,
                                               keep=True, effects=E.EffectsConfig(BINS16) if effects else None)
    return _CACHE[key]


def plain_bytes(res):
    return [res.stats.tobytes(), res.totals.tobytes(), res.hist.tobytes(), res.params.tobytes(), res.m.tobytes(), res.flags.tobytes(),
            res.ok.tobytes()]


def effect_bytes(e):
    return [e.sums.tobytes(), e.counts.tobytes(), e.cond_mean.tobytes(), e.cond_var.tobytes(), e.eta2.tobytes(), e.first.tobytes(), e.bins_used.tobytes()]


@pytest.mark.parametrize("chunk", [0, 256])
def test_the_run_with_effects(E, chunk):
    res, plain = run16(E, chunk, True), run16(E, chunk, False)
    assert plain_bytes(res) == plain_bytes(plain) and not hasattr(plain, "effects")
    e = res.effects
    assert e.edges.tobytes() == E.mc_effect_edges(dists_of(E, DISTS16), X16, BINS16).tobytes()
    sums, counts = E.mc_effects(res.params, res.m, res.flags, res.ok, res.nominal, e.edges)
    assert e.sums.tobytes() == sums.tobytes() and e.counts.tobytes() == counts.tobytes()
    assert np.all(e.counts.sum(axis=1) == res.n_valid[None, :]) and np.all(res.n_valid >= 900)
    host = E.mc_effect_indices(e.sums, e.counts, res.nominal)
    assert effect_bytes(e)[2:] == effect_bytes(host)[2:]
    zero = np.zeros(N12).tobytes()
    for j in FIXED_DIMS:  # one bin: nothing to tell apart
        assert e.bins_used[:, j].tolist() == [1] * N12 and e.first[:, j].tobytes() == zero and e.eta2[:, j].tobytes() == zero
    for j in CORNER_DIMS:
        assert e.bins_used[:, j].tolist() == [2] * N12 and not e.counts[j, 2:].any()
    for j in LIVE_DIMS:
        assert e.bins_used[:, j].tolist() == [BINS16] * N12
    moving = [j for j in range(N16) if j not in FIXED_DIMS]
    assert np.isnan(e.first[5, moving]).all() and np.isnan(e.eta2[5, moving]).all()  # (record 5 is constant)
    assert np.isfinite(np.delete(e.first, 5, axis=0)).all() and np.isfinite(e.cond_mean[LIVE_DIMS]).all()
    # a driven coordinate read back (record 4 reads variable 7): all of its variance lies between its own bins but the bins' share
    assert e.first[4, 7] > 0.9 and np.all(np.abs(np.delete(e.first[4], 7)) < 0.1)
    if chunk == 256:  # cutting the run changes nothing
        assert effect_bytes(e) == effect_bytes(run16(E, 0, True).effects)


def test_the_device_form_on_another_stream_equals_the_host_form(E):
    import torch

    s, res = system16(E), run16(E, 256, True)
    limits, hist = ranges(E)
    cells = N16 * BINS16 * N12
    x0 = torch.from_numpy(X16).cuda()
    out = lambda n: torch.full((max(n, 1),), 0x5A, dtype=torch.uint8, device="cuda")  # noqa: E731
    stats, totals, counts = out(N12 * 88), out(24), out(N12 * 18 * 8)
    kp, km, kf, ko = out(1000 * N16 * 8), out(1000 * N12 * 8), out(1000 * N12), out(1000)
    sums, cnt, cond_mean, cond_var, eta2, first = (out(8 * n) for n in (2 * cells, cells, cells, cells, N12 * N16, N12 * N16))
    used = out(4 * N12 * N16)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        edges = s.tolerance_mc_device(x0.data_ptr(), POS16, dists_of(E, DISTS16), RECORDS12, 1000, stats.data_ptr(), totals.data_ptr(),
                                      counts.data_ptr(), seed=SEED, limits=limits, hist=hist, chunk=256, keep_params_ptr=kp.data_ptr(),
                                      keep_m_ptr=km.data_ptr(), keep_flags_ptr=kf.data_ptr(), keep_ok_ptr=ko.data_ptr(), stream=stream.cuda_stream,
                                      effects=E.EffectsConfig(BINS16), effect_sums_ptr=sums.data_ptr(), effect_counts_ptr=cnt.data_ptr(),
                                      cond_mean_ptr=cond_mean.data_ptr(), cond_var_ptr=cond_var.data_ptr(), eta2_ptr=eta2.data_ptr(),
                                      first_ptr=first.data_ptr(), bins_used_ptr=used.data_ptr())
    stream.synchronize()
    raw = lambda t: t.cpu().numpy().tobytes()  # noqa: E731
    assert [raw(t) for t in (stats, totals, counts, kp, km, kf, ko)] == plain_bytes(res)
    assert [raw(t) for t in (sums, cnt, cond_mean, cond_var, eta2, first, used)] == effect_bytes(res.effects)
    assert edges.tobytes() == res.effects.edges.tobytes()
    # the caller's own edges, other than the last run's, on the host form: the reduction alone agrees again
    own = res.effects.edges.copy()
    own[0] = X16[0] + np.linspace(-0.1, 0.1, BINS16 - 1)
    again = s.tolerance_mc(X16, POS16, dists_of(E, DISTS16), RECORDS12, 1000, seed=SEED, chunk=256, keep=True, effects=E.EffectsConfig(BINS16, own))
    sums2, counts2 = E.mc_effects(again.params, again.m, again.flags, again.ok, again.nominal, own)
    assert again.effects.sums.tobytes() == sums2.tobytes() and again.effects.counts.tobytes() == counts2.tobytes()
    assert again.effects.counts[0].tobytes() != res.effects.counts[0].tobytes() and again.effects.counts[1:].tobytes() == res.effects.counts[1:].tobytes()


# ---- variants that do not assemble: the triangle of tests/test_gpu_contributors.py -------------------------------------------------
A, B, Cc = (0, 1), (2, 3), (4, 5)
TRIANGLE = O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(3, 0.0), O.distance(A, B, 1.0), O.distance(B, Cc, 1.0), O.distance(Cc, A, 1.9)])
TRI_POS, TRI_NOMINAL = [3, 4, 5], np.array([1.0, 1.0, 1.9])
TRI_DISTS = [(mc_ref.UNIFORM, -0.05, 0.05), (mc_ref.UNIFORM, -0.05, 0.05), (mc_ref.UNIFORM, -0.3, 0.3)]
TRI_MEASURE = O.stack([O.vertical_distance(Cc, A, 0.0), O.distance(B, Cc, 0.0)])


def test_variants_that_do_not_assemble_are_left_out(E):
    rc, x0, _, conv, nun = O.solve_batch(TRIANGLE, np.array([[0.0, 0.0, 1.0, 0.0, 0.9, 0.4]]))
    assert rc == 0 and conv[0] and nun[0] == 0
    s = E.System(TRIANGLE, 6)
    res = s.tolerance_mc(x0[0], TRI_POS, dists_of(E, TRI_DISTS), TRI_MEASURE, 600, seed=SEED, keep=True, effects=E.EffectsConfig(6))
    plain = s.tolerance_mc(x0[0], TRI_POS, dists_of(E, TRI_DISTS), TRI_MEASURE, 600, seed=SEED, keep=True)
    for name in ("stats", "totals", "params", "m", "flags", "ok"):
        assert getattr(res, name).tobytes() == getattr(plain, name).tobytes(), name
    assert 300 <= res.n_ok <= 500 and not (res.flags & 1).any()
    e = res.effects
    assert np.all(e.counts.sum(axis=1) == res.n_valid[None, :]) and res.n_valid.tolist() == [res.n_ok] * 2
    want, want_n = R.effects(res.params, res.m, res.flags, res.ok, res.nominal, e.edges)
    assert e.counts.tobytes() == want_n.tobytes() and e.sums.tobytes() == want.tobytes()  # (the leaves of the failed samples are +0.0)
    # the long side's upper bins are where the triangle stops closing: fewer samples count there, none in the last
    assert e.counts[2, 0, 0] > e.counts[2, 5, 0] and np.isfinite(e.first).all()


# ---- meaning, on the device's own samples -------------------------------------------------------------------------------------------
UNIFORM16 = [(mc_ref.UNIFORM, -0.1 - 0.01 * j, 0.1 + 0.005 * j) for j in range(N16)]


def test_difference_records_agree_with_the_host_reference(E):
    records = O.stack([d[0] for d in DIFFERENCES])
    res = system16(E).tolerance_mc(X16, POS16, dists_of(E, UNIFORM16), records, 1000, seed=SEED, keep=True, effects=E.EffectsConfig(8))
    p = E.mc_sample(SEED, dists_of(E, UNIFORM16), X16, 0, 1000)
    assert p.tobytes() == res.params.tobytes() and res.n_ok == 1000  # (UNIFORM draws: the same bits on both sides)
    y = np.stack([p[:, a] - p[:, b] for _, a, b in DIFFERENCES], axis=1)
    nominal_m = np.array([X16[a] - X16[b] for _, a, b in DIFFERENCES])
    sums, counts = R.effects(p, y, None, None, nominal_m, res.effects.edges)
    _, _, eta2, first, used = R.indices(sums, counts, nominal_m)
    assert res.effects.counts.tobytes() == counts.tobytes() and res.effects.bins_used.tobytes() == used.tobytes()
    print("difference records: max |first - reference|", np.max(np.abs(res.effects.first - first)), "max |eta2 - reference|",
          np.max(np.abs(res.effects.eta2 - eta2)))
    assert np.max(np.abs(res.effects.first - first)) <= 1e-4 and np.max(np.abs(res.effects.eta2 - eta2)) <= 1e-4
    for i, (_, a, b) in enumerate(DIFFERENCES):  # the two coordinates share the variance by their widths; nobody else has any
        wa, wb = (UNIFORM16[a][2] - UNIFORM16[a][1]) ** 2, (UNIFORM16[b][2] - UNIFORM16[b][1]) ** 2
        others = np.delete(res.effects.first[i], [a, b])
        print("record", i, "first", res.effects.first[i, [a, b]], "shares", wa / (wa + wb), wb / (wa + wb), "others' largest", np.max(np.abs(others)))
        assert res.effects.first[i, a] + res.effects.first[i, b] > 0.9 and np.all(np.abs(others) < 0.1)


# variables: the point (0, 1), a second x (2), the origin (3, 4); every one Fixed; driven: the point's x and y and the second x
HU, HV, HQ = 0.01, 0.35, 0.2
POINT = O.stack([O.fixed(0, 1.0), O.fixed(1, 0.0), O.fixed(2, 0.5), O.fixed(3, 0.0), O.fixed(4, 0.0)])
POINT_X0 = np.array([1.0, 0.0, 0.5, 0.0, 0.0])
POINT_DISTS = [(mc_ref.UNIFORM, -HU, HU), (mc_ref.UNIFORM, -HV, HV), (mc_ref.UNIFORM, -HQ, HQ)]
POINT_RECORDS = O.stack([O.horizontal_distance((0, 1), (2, 1), 0.0), O.distance((3, 4), (0, 1), 0.0)])
MEAN_SAMPLES = 16384


def test_the_curve_the_regression_does_not_see(E):
    s = E.System(POINT, 5)
    run = lambda **kw: s.tolerance_mc(POINT_X0, [0, 1, 2], dists_of(E, POINT_DISTS), POINT_RECORDS, MEAN_SAMPLES, seed=SEED, **kw)  # noqa: E731
    res, lin = run(effects=E.EffectsConfig(16)), run(contributors=True)
    assert res.stats.tobytes() == lin.stats.tobytes() and res.n_ok == MEAN_SAMPLES
    e = res.effects
    print("y in the distance: contrib", lin.contrib[1, 1], "first", e.first[1, 1], "eta2", e.eta2[1, 1])
    assert lin.contrib[1, 1] < 1e-3 and e.first[1, 1] > 0.5
    centres, means, n = e.curve(1, 1)
    print("the curve: centres", centres, "means", means, "counts", n)
    assert len(centres) == 16 and n.sum() == MEAN_SAMPLES and np.all(np.abs(n - MEAN_SAMPLES / 16) <= 6.0 * np.sqrt(MEAN_SAMPLES * 15 / 256))
    assert min(means[0], means[15]) > max(means[7], means[8]) and np.all(np.diff(means[:8]) < 0.0) and np.all(np.diff(means[8:]) > 0.0)
    # (the bin's own width w = 0.044 moves the mean by ~ w^2 / 24 = 8e-5, x's +-0.01 over a thousand samples by 2e-4)
    assert np.all(np.abs(means - np.sqrt(1.0 + centres ** 2)) <= 2e-3)
    # against the pick-freeze estimate of the same seed: SANITY bar (see the module's text)
    sob = s.tolerance_sobol(POINT_X0, [0, 1, 2], dists_of(E, POINT_DISTS), POINT_RECORDS, MEAN_SAMPLES, seed=SEED)
    for i in range(2):
        print("record", i, "first by the bins", e.first[i], "by pick-freeze", sob.first[i], "first_se", sob.first_se[i])
    assert np.all(np.abs(e.first - sob.first) <= 4.0 * sob.first_se + 0.05)


# ---- argument errors of the run: the return code, no output touched ---------------------------------------------------------------
def test_argument_errors_of_the_run(E):
    from ezpz_amd._lib import CMcConfig, CMcEffectConfig

    s = system16(E)
    dists = dists_of(E, DISTS16)
    for bad in (1, 65, 22):  # (16 x 22 x 12 > 4096 cells)
        with pytest.raises(E.NonLinearSystemError) as e:
            s.tolerance_mc(X16, POS16, dists, RECORDS12, 300, effects=E.EffectsConfig(bad))
        assert e.value.code == ERR_INVALID_ARGUMENT
    assert s.tolerance_mc(X16, POS16, dists, RECORDS12, 300, effects=E.EffectsConfig(21)).effects.counts.shape == (N16, 21, N12)
    with pytest.raises(E.NonLinearSystemError):  # k == 0 (the plain run takes it)
        s.tolerance_mc(X16, [], [], RECORDS12, 10, effects=E.EffectsConfig(4))
    with pytest.raises(E.NonLinearSystemError):  # m == 0
        s.tolerance_mc(X16, POS16, dists, RECORDS12[:0], 10, effects=E.EffectsConfig(4))
    with pytest.raises(ValueError):
        s.tolerance_mc(X16, POS16, dists, RECORDS12, 10, effects=E.EffectsConfig(4), contributors=True)
    with pytest.raises(ValueError):
        s.tolerance_mc(X16, POS16, dists, RECORDS12, 10, effects=E.EffectsConfig(4), quantiles=[0.5])
    good = E.mc_effect_edges(dists, X16, 4)
    for what, j, row in (("NaN", 0, [0.0, np.nan, 1.0]), ("decreasing", 5, [1.0, 0.5, 2.0])):
        edges = good.copy()
        edges[j] = row
        with pytest.raises(E.NonLinearSystemError) as e:
            s.tolerance_mc(X16, POS16, dists, RECORDS12, 10, effects=E.EffectsConfig(4, edges))
        assert e.value.code == ERR_INVALID_ARGUMENT, what
    # a NULL output with samples > 0, by the raw entry; samples == 0 with the same arguments is EZPZ_OK and writes nothing; an error of
    # the plain run comes back from this entry too
    d, pos = E.api.mc_dists(dists), np.arange(N16, dtype=np.uint32)
    cells = N16 * 4 * N12
    outs = {"sums": np.full(2 * cells, 7.0), "counts": np.full(cells, 7, np.uint64), "cond_mean": np.full(cells, 7.0), "cond_var": np.full(cells, 7.0),
            "eta2": np.full(N12 * N16, 7.0), "first": np.full(N12 * N16, 7.0), "bins_used": np.full(N12 * N16, 7, np.uint32)}
    stats, totals = np.full(N12 * 88, 0xA5, np.uint8), np.full(24, 0xA5, np.uint8)
    mc, cfg, ec = CMcConfig(1, 0, 0), E.Config()._c(), CMcEffectConfig(4, 0)

    def call(samples, missing, mc_=mc, edges_=good):
        return E.lib().ezpz_system_tolerance_mc_effects(s._h, X16.ctypes.data, pos.ctypes.data, N16, d.ctypes.data, None, RECORDS12.ctypes.data, N12, None,
                                                        None, None, None, samples, C.byref(mc_), C.byref(cfg), stats.ctypes.data, totals.ctypes.data,
                                                        None, None, None, None, None, C.byref(ec), None if edges_ is None else edges_.ctypes.data,
                                                        *(None if name == missing else a.ctypes.data for name, a in outs.items()))

    for missing in outs:
        assert call(300, missing) == ERR_INVALID_ARGUMENT, missing
        assert call(0, missing) == 0, missing
    assert call(300, None, edges_=None) == ERR_INVALID_ARGUMENT and call(0, None, edges_=None) == 0
    assert call(300, None, mc_=CMcConfig(1, 0, 65)) == ERR_INVALID_ARGUMENT  # (hist_bins > 64: the plain run's)
    assert all(np.all(a == 7) for a in outs.values()) and np.all(stats == 0xA5) and np.all(totals == 0xA5)
    assert call(300, None) == 0 and not np.any(outs["counts"] == 7) and int(outs["counts"].reshape(N16, 4, N12).sum(axis=1)[0, 0]) == 300
