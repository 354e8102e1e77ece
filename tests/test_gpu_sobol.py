"""GPU tests (-m gpu) of the Sobol tolerance indices (ezpz_mc_sobol_sums_device, ezpz_system_tolerance_sobol and its _device form;
csrc/mc_sobol.hip, csrc/tolerance_mc.hip): the device's sums are the sums tests/sobol_ref.py states, bit for bit, and the host
form's; cutting the reduction into rounds or moving it to another stream changes no byte; the run's matrix A is the plain
Monte-Carlo run byte for byte, its rows are the chain sampler -> params entry -> measure entry, its sums are the reduction alone on
its kept rows and its closing kernel is the host's closing step; and the indices mean what they say on the device's own samples.
Every case is small: the shapes are the edges of a block of 256 samples and of a round, not a workload.

Bars.  Everything but the meaning: bytes.  The meaning: six standard errors, the convention of tests/test_tolerance_mc_cpu.py,
the standard error computed here from the kept rows with numpy.

The curved case.  A point at nominal (1, 0), its x = 1 + u and y = v each a driven dimension, u uniform on +-0.25 and v on +-0.35
(chosen BEFORE any run, from this estimate): its distance from the origin sqrt((1 + u)^2 + v^2) ~ 1 + u + v^2 / 2, so y acts
through curvature alone: Var(v^2 / 2) = 0.35^4 / 45 = 3.3e-4 against Var(u) = 0.25^2 / 3 = 2.1e-2, a first-order index near 0.016,
while the regression's coefficient for y is 0 by symmetry.  With 16384 samples the standard error of that index is about
std(dB) std(t) / V / 128 = 0.145 * 0.026 / 0.021 / 128 = 1.4e-3: the index stands some eleven standard errors above 0, so
`first > contrib + 6 se` has five to spare.  The exact indices come from a midpoint rule on a 2000 x 2000 grid (error ~1e-7)."""
import ctypes as C

import numpy as np
import pytest

import mc_ref
import sobol_ref as R
from oracle import oracle as O
from test_sobol_cpu import SUM_SHAPES, TRI_DISTS, TRI_NOMINAL, TRI_POS, TRI_SAMPLES, TRI_SEED, TRI_START, rows_of, triangle

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


# ---- the reduction alone ------------------------------------------------------------------------------------------------------------
def device_sums(E, f, flags, ok, nominal_m, mask, chunk=0, stream=None, k=None, m=None, prefill=None):
    """ezpz_mc_sobol_sums_device on copies of the arrays: (rc, sums, n_complete)."""
    import torch

    samples, rows, n_meas = f.shape
    k, m = rows - 2 if k is None else k, n_meas if m is None else m
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (f, flags, ok, nominal_m)]
    sums = torch.full((max(m, 1) * R.width(min(k, 40)),), 7.0, dtype=torch.float64, device="cuda")
    n = torch.full((max(m, 1),), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    args = [0 if t is None else t.data_ptr() for t in dev] + [mask, samples, k, m, chunk, sums.data_ptr(), n.data_ptr()]
    if stream is None:
        rc = E.lib().ezpz_mc_sobol_sums_device(*args, None)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_mc_sobol_sums_device(*args, stream.cuda_stream)
        stream.synchronize()
    return rc, sums.cpu().numpy().reshape(max(m, 1), -1), n.cpu().numpy().astype(np.uint64)


def reference_sums(k, m, samples, mask):
    key = ("ref", k, m, samples, mask)
    if key not in _CACHE:
        _CACHE[key] = R.sums(*rows_of(k, m, samples, mask), mask)
    return _CACHE[key]


WIDE_MASK = 0b1000_0000_0001_0000_0000_0000_0100_0010  # FIXED dimensions 1, 6, 20 and 31 of 32


# (U = m (k + 1) units pick the length of the kernel's sub-trees: 16, 32 and 64 units are the 2, 4 and 8 eights the other shapes miss)
@pytest.mark.parametrize("k,m,samples,mask", SUM_SHAPES + [(1, 1, 257, 0), (8, 8, 257, 0b100), (32, 32, 257, WIDE_MASK),
                                                           (3, 4, 257, 0), (7, 4, 257, 0), (7, 8, 257, 0)])
def test_the_device_sums_are_the_stated_sums(E, k, m, samples, mask):
    a = rows_of(k, m, samples, mask)
    want, want_n = reference_sums(k, m, samples, mask)
    rc, got, got_n = device_sums(E, *a, mask)
    assert rc == 0 and got_n.tolist() == want_n.tolist() and got.tobytes() == want.tobytes(), (got, want)
    host, host_n = E.mc_sobol_sums(*a, mask)
    assert host.tobytes() == got.tobytes() and host_n.tolist() == got_n.tolist()
    if samples == 257:  # flags == NULL: every bit clear; ok == NULL: every one set
        f, _, _, nominal_m = a
        host2, host_n2 = E.mc_sobol_sums(f, None, None, nominal_m, mask)
        rc, got2, got_n2 = device_sums(E, f, None, None, nominal_m, mask)
        assert rc == 0 and got2.tobytes() == host2.tobytes() and got_n2.tolist() == host_n2.tolist() and np.all(host_n2 >= want_n)


def test_rounds_and_streams_change_no_byte(E):
    import torch

    k, m, samples, mask = 3, 2, 1000, 0b010
    a = rows_of(k, m, samples, mask)
    want, want_n = reference_sums(k, m, samples, mask)
    for chunk in (256, 512, 300, 0):  # (300 rounds up to 512)
        rc, got, got_n = device_sums(E, *a, mask, chunk=chunk)
        assert rc == 0 and got_n.tolist() == want_n.tolist() and got.tobytes() == want.tobytes(), chunk
    stream = torch.cuda.Stream()
    for chunk in (256, 0):  # (the outputs are pre-filled with 7)
        rc, got, got_n = device_sums(E, *a, mask, chunk=chunk, stream=stream)
        assert rc == 0 and got_n.tolist() == want_n.tolist() and got.tobytes() == want.tobytes(), chunk


def test_argument_errors_of_the_device_reduction(E):
    a = rows_of(2, 2, 10)
    for bad in (dict(k=33), dict(m=0), dict(m=33)):
        rc, sums, n = device_sums(E, *a, 0, **bad)
        assert rc == ERR_INVALID_ARGUMENT and np.all(sums == 7.0) and np.all(n == 7), bad
    rc, sums, n = device_sums(E, *a, 0b100)
    assert rc == ERR_INVALID_ARGUMENT and np.all(sums == 7.0) and np.all(n == 7)
    f, flags, ok, nominal_m = a
    rc, sums, n = device_sums(E, f, flags, ok, None, 0)
    assert rc == ERR_INVALID_ARGUMENT and np.all(sums == 7.0) and np.all(n == 7)
    assert E.lib().ezpz_mc_sobol_sums_device(None, None, None, None, 0, 10, 2, 2, 0, None, None, None) == ERR_INVALID_ARGUMENT
    assert E.lib().ezpz_mc_sobol_sums_device(None, None, None, None, 0, 0, 2, 2, 0, None, None, None) == 0  # samples == 0


# ---- the run: the 16-variable system of tests/test_gpu_contributors.py, all Fixed, cut to three sampled dimensions and a FIXED one ---
N16 = 16
_rng = np.random.default_rng(7)
X16 = _rng.uniform(0.5, 3.0, N16) * _rng.choice([-1.0, 1.0], N16) + np.arange(N16) * 0.37  # the nominal values, and the nominal solution
POS4 = [1, 6, 4, 11]
DISTS4 = [(mc_ref.UNIFORM, -0.2, 0.2), (mc_ref.NORMAL, 0.1, 0.0), (mc_ref.FIXED, 0.0, 0.0), (mc_ref.NORMAL, 0.15, 1.5)]
NOMINAL4 = X16[POS4]
FIXED_J, MASK4 = 2, 0b0100
# a difference of two driven coordinates, two curved records, one that reads the FIXED dimension alone (constant), a driven coordinate
RECORDS5 = O.stack([O.vertical_distance((0, 1), (2, 6), 0.0), O.distance((0, 1), (2, 3), 0.0), O.fixed(4, 0.0),
                    O.point_line_distance((0, 1), (5, 6), (10, 11), 0.0), O.fixed(11, 0.0)])
K4, M5, RUN_SAMPLES = 4, 5, 1000
SEED_B = SEED ^ R.SEED_B


def dists_of(E, tuples):
    return [E.McDist(*t) for t in tuples]


def system16(E):
    if "s16" not in _CACHE:
        _CACHE["s16"] = E.System(O.stack([O.fixed(v, float(X16[v])) for v in range(N16)]), N16)
    return _CACHE["s16"]


def run4(E, chunk):
    key = ("run", chunk)
    if key not in _CACHE:
        _CACHE[key] = system16(E).tolerance_sobol(X16, POS4, dists_of(E, DISTS4), RECORDS5, RUN_SAMPLES, seed=SEED, chunk=chunk, keep=True)
    return _CACHE[key]


def plain(E, seed):
    key = ("plain", seed)
    if key not in _CACHE:
        _CACHE[key] = system16(E).tolerance_mc(X16, POS4, dists_of(E, DISTS4), RECORDS5, RUN_SAMPLES, seed=seed, keep=True)
    return _CACHE[key]


def index_bytes(r):
    return [r.sums.tobytes(), r.n_complete.tobytes(), r.var.tobytes(), r.first.tobytes(), r.total.tobytes(), r.first_var.tobytes(),
            r.total_var.tobytes()]


@pytest.mark.parametrize("chunk", [256, 0])
def test_the_run(E, chunk):
    s, res, pa, pb = system16(E), run4(E, chunk), plain(E, SEED), plain(E, SEED_B)
    assert res.seed_b == SEED_B and res.f.shape == (RUN_SAMPLES, K4 + 2, M5)
    # matrix A is the plain run with the same seed, matrix B the plain run with seed_b
    assert res.stats.tobytes() == pa.stats.tobytes() and res.totals.tobytes() == pa.totals.tobytes() and res.n_ok == RUN_SAMPLES
    for row, p in ((0, pa), (1, pb)):
        assert res.f[:, row].tobytes() == p.m.tobytes() and res.flags[:, row].tobytes() == p.flags.tobytes(), row
        assert res.ok[:, row].tobytes() == p.ok.tobytes(), row
    # the sampler: UNIFORM draws are the host's bits (NORMAL ones may differ in the last bits: the kept device draws are the matrices)
    host_a = E.mc_sample(SEED, dists_of(E, DISTS4), NOMINAL4, 0, RUN_SAMPLES)
    assert pa.params[:, [0, 2]].tobytes() == host_a[:, [0, 2]].tobytes() and np.max(np.abs(pa.params - host_a)) < 1e-12
    # row 2 + j is the chain: A with column j from B, the params entry, the measure entry
    for j in range(K4):
        if j == FIXED_J:
            assert res.f[:, 2 + j].tobytes() == res.f[:, 0].tobytes() and res.flags[:, 2 + j].tobytes() == res.flags[:, 0].tobytes()
            assert res.ok[:, 2 + j].tobytes() == res.ok[:, 0].tobytes()
            continue
        ab = pa.params.copy()
        ab[:, j] = pb.params[:, j]
        x, st, _ = s.solve_batch_params(np.tile(X16, (RUN_SAMPLES, 1)), POS4, ab)
        m, flags = s.measure(x, RECORDS5, want_flags=True)
        assert res.f[:, 2 + j].tobytes() == m.tobytes() and res.flags[:, 2 + j].tobytes() == flags.tobytes(), j
        assert res.ok[:, 2 + j].tolist() == ((st["converged"] != 0) & (st["n_unsatisfied"] == 0)).astype(np.uint8).tolist(), j
    # the sums are the reduction alone on the kept rows, on the device and on the host, and the restatement's
    rc, dev_sums, dev_n = device_sums(E, res.f, res.flags, res.ok, res.nominal, MASK4)
    host_sums, host_n = E.mc_sobol_sums(res.f, res.flags, res.ok, res.nominal, MASK4)
    if "run_ref" not in _CACHE:
        _CACHE["run_ref"] = R.sums(res.f, res.flags, res.ok, res.nominal, MASK4)
    ref_sums, ref_n = _CACHE["run_ref"]
    assert rc == 0 and res.sums.tobytes() == dev_sums.tobytes() == host_sums.tobytes() == ref_sums.tobytes()
    assert res.n_complete.tolist() == dev_n.tolist() == host_n.tolist() == ref_n.tolist() == [RUN_SAMPLES] * M5
    # the closing kernel is the host's closing step, and the restatement's
    host = E.mc_sobol_indices(res.sums, res.n_complete)
    assert index_bytes(res) == index_bytes(host)
    for name, want in zip(("var", "first", "total", "first_var", "total_var"), R.indices(res.sums, res.n_complete)):
        assert getattr(res, name).tobytes() == want.tobytes(), name
    # what the numbers say: a FIXED dimension has +0.0 everywhere, the constant record NaN, the driven coordinate one index of 1
    assert res.first[[0, 1, 3, 4], FIXED_J].tobytes() == res.total[[0, 1, 3, 4], FIXED_J].tobytes() == np.zeros(4).tobytes()
    assert res.var[2] == 0.0 and np.isnan(res.first[2]).all() and np.isnan(res.total[2]).all()
    assert np.all(np.abs(res.total[4] - [0.0, 0.0, 0.0, 1.0]) <= 6.0 * res.total_se[4] + 1e-12)
    if chunk == 0:  # cutting the run changes nothing
        assert index_bytes(res) == index_bytes(run4(E, 256)) and res.f.tobytes() == run4(E, 256).f.tobytes()


def test_the_device_form_on_another_stream_equals_the_host_form(E):
    import torch

    s, res = system16(E), run4(E, 256)
    x0 = torch.from_numpy(X16).cuda()
    out = lambda n: torch.full((max(n, 1),), 0x5A, dtype=torch.uint8, device="cuda")  # noqa: E731
    stats, totals = out(M5 * 88), out(24)
    sums, n, var = out(8 * M5 * R.width(K4)), out(8 * M5), out(8 * M5)
    first, total, first_var, total_var = (out(8 * M5 * K4) for _ in range(4))
    kf, kflags, kok = out(8 * RUN_SAMPLES * (K4 + 2) * M5), out(RUN_SAMPLES * (K4 + 2) * M5), out(RUN_SAMPLES * (K4 + 2))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s.tolerance_sobol_device(x0.data_ptr(), POS4, dists_of(E, DISTS4), RECORDS5, RUN_SAMPLES, stats.data_ptr(), totals.data_ptr(), sums.data_ptr(),
                                 n.data_ptr(), var.data_ptr(), first.data_ptr(), total.data_ptr(), first_var.data_ptr(), total_var.data_ptr(),
                                 seed=SEED, chunk=256, keep_f_ptr=kf.data_ptr(), keep_flags_ptr=kflags.data_ptr(), keep_ok_ptr=kok.data_ptr(),
                                 stream=stream.cuda_stream)
    stream.synchronize()
    raw = lambda t: t.cpu().numpy().tobytes()  # noqa: E731
    assert [raw(t) for t in (stats, totals)] == [res.stats.tobytes(), res.totals.tobytes()]
    assert [raw(t) for t in (sums, n, var, first, total, first_var, total_var)] == index_bytes(res)
    assert [raw(t) for t in (kf, kflags, kok)] == [res.f.tobytes(), res.flags.tobytes(), res.ok.tobytes()]


# ---- meaning, on the device's own samples -------------------------------------------------------------------------------------------
# variables: the point (0, 1), a second x (2), the origin (3, 4); every one Fixed; driven: the point's x and y and the second x
HU, HV, HQ = 0.25, 0.35, 0.2
POINT = O.stack([O.fixed(0, 1.0), O.fixed(1, 0.0), O.fixed(2, 0.5), O.fixed(3, 0.0), O.fixed(4, 0.0)])
POINT_X0 = np.array([1.0, 0.0, 0.5, 0.0, 0.0])
POINT_DISTS = [(mc_ref.UNIFORM, -HU, HU), (mc_ref.UNIFORM, -HV, HV), (mc_ref.UNIFORM, -HQ, HQ)]
POINT_RECORDS = O.stack([O.horizontal_distance((0, 1), (2, 1), 0.0), O.distance((3, 4), (0, 1), 0.0)])
MEAN_SAMPLES = 16384


def quadrature():
    """(first [2], total [2]) of sqrt((1 + u)^2 + v^2) for u, v uniform: the midpoint rule on a dense grid."""
    n = 2000
    u = (np.arange(n) + 0.5) / n * 2 * HU - HU
    v = (np.arange(n) + 0.5) / n * 2 * HV - HV
    f = np.sqrt((1.0 + u[:, None]) ** 2 + v[None, :] ** 2)
    V = f.var()
    first = np.array([f.mean(axis=1).var(), f.mean(axis=0).var()]) / V
    total = np.array([f.var(axis=0).mean(), f.var(axis=1).mean()]) / V
    return first, total


def test_meaning_on_the_devices_own_samples(E):
    s = E.System(POINT, 5)
    res = s.tolerance_sobol(POINT_X0, [0, 1, 2], dists_of(E, POINT_DISTS), POINT_RECORDS, MEAN_SAMPLES, seed=SEED, keep=True)
    assert res.n_complete.tolist() == [MEAN_SAMPLES] * 2 and res.n_ok == MEAN_SAMPLES
    d = res.f - res.nominal
    dA, dB = d[:, 0], d[:, 1]
    var = np.concatenate([dA, dB]).var(axis=0, ddof=1)
    assert np.max(np.abs(res.var / var - 1.0)) <= 1e-9
    se_first, se_total = np.zeros((2, 3)), np.zeros((2, 3))
    for j in range(3):
        t = d[:, 2 + j] - dA
        se_first[:, j] = (dB * t).std(axis=0, ddof=1) / np.sqrt(MEAN_SAMPLES) / var
        se_total[:, j] = (t * t / 2.0).std(axis=0, ddof=1) / np.sqrt(MEAN_SAMPLES) / var
    # (a) the difference of two driven coordinates: linear, first = total = w_j^2 s_j^2 / sum, s_j^2 = h_j^2 / 3 the variances
    w2 = np.array([HU * HU, 0.0, HQ * HQ]) / 3.0
    want_a = w2 / w2.sum()
    # (b) the distance from the origin
    first_b, total_b = quadrature()
    want_first, want_total = np.array([want_a, [*first_b, 0.0]]), np.array([want_a, [*total_b, 0.0]])
    for i in range(2):
        print("record", i, "first", res.first[i], "want", want_first[i], "se", se_first[i])
        print("record", i, "total", res.total[i], "want", want_total[i], "se", se_total[i])
    assert np.all(np.abs(res.first - want_first) <= 6.0 * se_first + 1e-12)
    assert np.all(np.abs(res.total - want_total) <= 6.0 * se_total + 1e-12)
    # the case the indices exist for: y moves the distance through curvature alone -- the regression does not see it
    mc = s.tolerance_mc(POINT_X0, [0, 1, 2], dists_of(E, POINT_DISTS), POINT_RECORDS, MEAN_SAMPLES, seed=SEED, contributors=True)
    print("y in the distance: first", res.first[1, 1], "contrib", mc.contrib[1, 1], "six standard errors", 6.0 * se_first[1, 1])
    assert res.first[1, 1] > mc.contrib[1, 1] + 6.0 * se_first[1, 1]
    assert mc.stats.tobytes() == res.stats.tobytes()


# ---- variants that do not assemble: the triangle of tests/test_gpu_contributors.py -------------------------------------------------
TRI_MEASURE = O.stack([O.vertical_distance((4, 5), (0, 1), 0.0), O.distance((2, 3), (4, 5), 0.0)])


def test_variants_that_do_not_assemble_are_left_out(E):
    rc, x0, _, conv, nun = O.solve_batch(triangle(TRI_NOMINAL), TRI_START)
    assert rc == 0 and conv[0] and nun[0] == 0
    s = E.System(triangle(TRI_NOMINAL), 6)
    res = s.tolerance_sobol(x0[0], TRI_POS, dists_of(E, TRI_DISTS), TRI_MEASURE, TRI_SAMPLES, seed=TRI_SEED, keep=True)
    complete = (res.ok != 0).all(axis=1)[:, None] & ~((res.flags & 1) != 0).any(axis=1) & np.isfinite(res.f).all(axis=1)
    count = complete.sum(axis=0)
    print("complete pick-freeze samples of the triangle:", count.tolist(), "of", TRI_SAMPLES, "; ok per row", (res.ok != 0).sum(axis=0).tolist())
    assert res.n_complete.tolist() == count.tolist() and np.all(0 < count) and np.all(count < TRI_SAMPLES)
    assert np.all(0.10 * TRI_SAMPLES <= count) and np.all(count <= 0.90 * TRI_SAMPLES)
    plain_run = s.tolerance_mc(x0[0], TRI_POS, dists_of(E, TRI_DISTS), TRI_MEASURE, TRI_SAMPLES, seed=TRI_SEED, keep=True)
    assert res.stats.tobytes() == plain_run.stats.tobytes() and res.totals.tobytes() == plain_run.totals.tobytes()
    assert res.ok[:, 0].tobytes() == plain_run.ok.tobytes() and res.n_ok < TRI_SAMPLES
    want, want_n = R.sums(res.f, res.flags, res.ok, res.nominal, 0)
    assert res.sums.tobytes() == want.tobytes() and res.n_complete.tolist() == want_n.tolist()  # (the failed samples' leaves are +0.0)
    assert np.isfinite(res.first).all() and np.isfinite(res.total).all()


# ---- argument errors of the run: the return code, no output touched -----------------------------------------------------------------
def test_argument_errors_of_the_run(E):
    from ezpz_amd._lib import CMcConfig, CSobolConfig

    s = system16(E)
    d4 = dists_of(E, DISTS4)
    for bad in (dict(seed_b=SEED), dict(dists=d4[:3] + [E.McDist.corner(-0.1, 0.1)]), dict(records=RECORDS5[:0]),
                dict(records=O.stack([O.fixed(v % N16, 0.0) for v in range(33)])),
                dict(dists=d4[:3] + [E.McDist(mc_ref.UNIFORM, 0.2, -0.2)])):
        kw = dict(positions=POS4, dists=d4, records=RECORDS5, seed_b=None)
        kw.update(bad)
        with pytest.raises(E.NonLinearSystemError) as e:
            s.tolerance_sobol(X16, kw["positions"], kw["dists"], kw["records"], 300, seed=SEED, seed_b=kw["seed_b"])
        assert e.value.code == ERR_INVALID_ARGUMENT, bad
    # more than 32 driving dimensions
    big = E.System(O.stack([O.fixed(v, float(v)) for v in range(33)]), 33)
    wide = [E.McDist(mc_ref.UNIFORM, -0.1, 0.1)] * 33
    with pytest.raises(E.NonLinearSystemError) as e:
        big.tolerance_sobol(np.arange(33.0), list(range(33)), wide, O.stack([O.fixed(0, 0.0)]), 10)
    assert e.value.code == ERR_INVALID_ARGUMENT
    assert big.tolerance_sobol(np.arange(33.0), list(range(32)), wide[:32], O.stack([O.fixed(0, 0.0)]), 10).n_complete.tolist() == [10]
    assert s.tolerance_sobol(X16, [], [], RECORDS5, 10).n_complete.tolist() == [10] * M5  # (k = 0 is legal)
    # by the raw entry: a NULL output or x0 with samples > 0, a histogram; samples == 0 with the same arguments is EZPZ_OK, nothing written
    d, pos = E.api.mc_dists(d4), np.array(POS4, np.uint32)
    outs = {"stats": np.full(M5 * 88, 0xA5, np.uint8), "totals": np.full(24, 0xA5, np.uint8), "sums": np.full(M5 * R.width(K4), 7.0),
            "n_complete": np.full(M5, 7, np.uint64), "var": np.full(M5, 7.0), "first": np.full(M5 * K4, 7.0), "total": np.full(M5 * K4, 7.0),
            "first_var": np.full(M5 * K4, 7.0), "total_var": np.full(M5 * K4, 7.0)}
    before = {name: a.copy() for name, a in outs.items()}
    cfg = E.Config()._c()

    def call(samples, missing=None, hist_bins=0, seed_b=SEED_B, x0=X16):
        mc, sc = CMcConfig(SEED, 0, hist_bins), CSobolConfig(seed_b, 0)
        return E.lib().ezpz_system_tolerance_sobol(s._h, None if x0 is None else x0.ctypes.data, pos.ctypes.data, K4, d.ctypes.data, None,
                                                   RECORDS5.ctypes.data, M5, samples, C.byref(mc), C.byref(cfg), C.byref(sc),
                                                   *(None if name == missing else a.ctypes.data for name, a in outs.items()), None, None, None)

    for missing in outs:
        assert call(300, missing) == ERR_INVALID_ARGUMENT, missing
        assert call(0, missing) == 0, missing
    assert call(300, hist_bins=8) == ERR_INVALID_ARGUMENT and call(300, seed_b=SEED) == ERR_INVALID_ARGUMENT and call(0, seed_b=SEED) == ERR_INVALID_ARGUMENT
    assert call(300, x0=None) == ERR_INVALID_ARGUMENT
    assert all(a.tobytes() == before[name].tobytes() for name, a in outs.items())
    assert call(300) == 0 and outs["n_complete"].tolist() == [300] * M5  # (sobol == NULL is the default seed_b: not the run's)
