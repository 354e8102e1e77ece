"""GPU tests (-m gpu) of the Monte-Carlo quantiles (ezpz_mc_quantiles_device, ezpz_system_tolerance_mc_quantiles and its _device
form; csrc/mc_quantiles.hip, csrc/tolerance_mc.hip): the device's radix select gives the records tests/quantile_ref.py states and
the host form's, byte for byte; another stream changes no byte; the run is the plain Monte-Carlo run byte for byte and its quantiles
are the selection alone on its kept rows; and the quantiles say what mean and std cannot.  Every case is small: the shapes are the
edges of a turn of the count kernel, of a digit and of the key, not a workload.

Bars.  Everything but the curved case: bytes.

The curved case.  A point at (1, 0), its x FIXED and its y = v uniform on +-0.35 (chosen BEFORE any run): its distance from the origin
is m = sqrt(1 + v^2) >= 1, increasing in |v|, and |v| is uniform on [0, 0.35], so the exact quantile is sqrt(1 + (0.35 p)^2).  The
mean is about 1 + 0.35^2 / 6 = 1.0204 and the standard deviation about 0.35^2 / 2 * sqrt(4 / 45) = 0.0183: mean - 3 std = 0.9655 lies
below 1, a distance no variant can have, while the 0.135 % quantile is 1 + 1e-7.  The band: tests/test_quantiles_cpu.py's reasoning,
z = 6 (at p = 0.00135 and n = 16384: n p = 22, so the lower rank is clamped to 0 and the band holds unless no draw at all falls
below the quantile, probability e^-22)."""
import ctypes as C

import numpy as np
import pytest

import mc_ref
import quantile_ref as R
from ezpz_amd._lib import CMcQuantileConfig
from oracle import oracle as O
from test_quantiles_cpu import SAMPLES, SHAPES, probs_of, reference, rows_of_q
from test_sobol_cpu import TRI_DISTS, TRI_NOMINAL, TRI_POS, TRI_SAMPLES, TRI_SEED, TRI_START, triangle

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


# ---- the selection alone -------------------------------------------------------------------------------------------------------------
def device_quantiles(E, m, flags, ok, probs, z, stream=None, n_meas=None, n_q=None, samples=None, m_null=False, probs_null=False,
                     out_null=False):
    """ezpz_mc_quantiles_device on copies of the arrays, the output prefilled with 7: (rc, records or the raw bytes on an error)."""
    import torch

    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (m, flags, ok)]
    probs = np.ascontiguousarray(probs, dtype=np.float64)
    n_meas, n_q, samples = m.shape[1] if n_meas is None else n_meas, len(probs) if n_q is None else n_q, len(m) if samples is None else samples
    out = torch.full((64 * 17 * 80,), 7, dtype=torch.uint8, device="cuda")
    qc = CMcQuantileConfig(z, 0)
    torch.cuda.synchronize()
    args = [0 if t is None else t.data_ptr() for t in dev] + [samples, n_meas, None if probs_null else probs.ctypes.data, n_q, C.byref(qc),
                                                              None if out_null else out.data_ptr()]
    if m_null:
        args[0] = None
    if stream is None:
        rc = E.lib().ezpz_mc_quantiles_device(*args, None)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_mc_quantiles_device(*args, stream.cuda_stream)
        stream.synchronize()
    raw = out.cpu().numpy()
    if rc != 0 or out_null:
        return rc, raw
    used = min(n_meas, 64) * min(n_q, 16) * 80
    assert np.all(raw[used:] == 7)
    return rc, raw[:used].view(R.DTYPE).reshape(n_meas, n_q)


@pytest.mark.parametrize("n_meas,n_q", SHAPES)
@pytest.mark.parametrize("samples", SAMPLES + (1025, 2500))  # (a turn of the count kernel is 1024 samples)
def test_the_device_selection_is_the_stated_rule(E, samples, n_meas, n_q):
    m, flags, ok = rows_of_q(n_meas, samples, samples % 2)
    probs = probs_of(n_q)
    for z in (0.0, 3.0):
        want = reference(n_meas, n_q, samples, z)
        rc, got = device_quantiles(E, m, flags, ok, probs, z)
        assert rc == 0 and got.tobytes() == want.tobytes(), (z, got, want)
        assert E.mc_quantiles(m, flags, ok, probs, z).tobytes() == got.tobytes()
    if samples in (257, 2500):  # flags == NULL: every bit clear; ok == NULL: every one set
        want = reference(n_meas, n_q, samples, 3.0, bare=True)
        rc, got = device_quantiles(E, m, None, None, probs, 3.0)
        assert rc == 0 and got.tobytes() == want.tobytes() == E.mc_quantiles(m, None, None, probs, 3.0).tobytes()
        rc, got = device_quantiles(E, m, flags, None, probs, 3.0)
        assert rc == 0 and got.tobytes() == E.mc_quantiles(m, flags, None, probs, 3.0).tobytes()


def test_another_stream_changes_no_byte(E):
    import torch

    stream = torch.cuda.Stream()
    for n_meas, n_q, samples in ((3, 5, 1000), (64, 16, 257), (1, 1, 2500)):
        m, flags, ok = rows_of_q(n_meas, samples, samples % 2)
        want = reference(n_meas, n_q, samples, 3.0)
        for _ in range(2):  # (the second call finds the workspace as the first left it)
            rc, got = device_quantiles(E, m, flags, ok, probs_of(n_q), 3.0, stream=stream)
            assert rc == 0 and got.tobytes() == want.tobytes(), (n_meas, n_q, samples)


def test_argument_errors_of_the_device_selection_leave_the_prefill(E):
    m, flags, ok = rows_of_q(3, 10, 0)
    probs = [0.1, 0.5, 0.9]
    nan, inf = float("nan"), float("inf")
    cases = [dict(n_meas=0), dict(n_meas=65), dict(n_q=17, probs=[0.5] * 17), dict(samples=1 << 32), dict(probs=[0.1, -1e-300, 0.9]),
             dict(probs=[0.1, 1.0000000000000002, 0.9]), dict(probs=[nan, 0.5, 0.9]), dict(probs=[0.1, 0.5, inf]), dict(z=-1.0), dict(z=nan),
             dict(z=inf), dict(probs_null=True), dict(m_null=True), dict(out_null=True)]
    for case in cases:
        a = dict(probs=probs, z=0.0)
        a.update(case)
        rc, raw = device_quantiles(E, m, flags, ok, a.pop("probs"), a.pop("z"), **a)
        assert rc == ERR_INVALID_ARGUMENT and np.all(raw == 7), case
    rc, raw = device_quantiles(E, m, flags, ok, probs, 0.0, samples=0)  # samples == 0, n_q == 0: EZPZ_OK, nothing written
    assert rc == 0 and np.all(raw.view(np.uint8) == 7)
    rc, raw = device_quantiles(E, m, flags, ok, probs, 0.0, n_q=0, out_null=True)
    assert rc == 0 and np.all(raw == 7)


# ---- the run: the 16-variable all-Fixed system of tests/test_gpu_sobol.py (its constants restated) ------------------------------------
N16 = 16
_rng = np.random.default_rng(7)
X16 = _rng.uniform(0.5, 3.0, N16) * _rng.choice([-1.0, 1.0], N16) + np.arange(N16) * 0.37  # the nominal values, and the nominal solution
POS4 = [1, 6, 4, 11]
DISTS4 = [(mc_ref.UNIFORM, -0.2, 0.2), (mc_ref.NORMAL, 0.1, 0.0), (mc_ref.FIXED, 0.0, 0.0), (mc_ref.NORMAL, 0.15, 1.5)]
RECORDS5 = O.stack([O.vertical_distance((0, 1), (2, 6), 0.0), O.distance((0, 1), (2, 3), 0.0), O.fixed(4, 0.0),
                    O.point_line_distance((0, 1), (5, 6), (10, 11), 0.0), O.fixed(11, 0.0)])
M5, RUN_SAMPLES = 5, 1000
RUN_PROBS, RUN_Z = [0.00135, 0.5, 0.99865, 0.0, 1.0, 0.25], 3.0
RUN_LIMITS, RUN_HIST = (-10.0, 10.0), (-8.0, 8.0, 16)


def dists_of(E, tuples):
    return [E.McDist(*t) for t in tuples]


def system16(E):
    if "s16" not in _CACHE:
        _CACHE["s16"] = E.System(O.stack([O.fixed(v, float(X16[v])) for v in range(N16)]), N16)
    return _CACHE["s16"]


def run_q(E, chunk):
    key = ("run", chunk)
    if key not in _CACHE:
        _CACHE[key] = system16(E).tolerance_mc(X16, POS4, dists_of(E, DISTS4), RECORDS5, RUN_SAMPLES, seed=SEED, chunk=chunk, keep=True,
                                               limits=RUN_LIMITS, hist=RUN_HIST, quantiles=RUN_PROBS, quantile_z=RUN_Z)
    return _CACHE[key]


def plain(E):
    if "plain" not in _CACHE:
        _CACHE["plain"] = system16(E).tolerance_mc(X16, POS4, dists_of(E, DISTS4), RECORDS5, RUN_SAMPLES, seed=SEED, keep=True,
                                                   limits=RUN_LIMITS, hist=RUN_HIST)
    return _CACHE["plain"]


def run_bytes(r):
    return [r.stats.tobytes(), r.totals.tobytes(), r.hist.tobytes(), r.params.tobytes(), r.m.tobytes(), r.flags.tobytes(), r.ok.tobytes()]


@pytest.mark.parametrize("chunk", [256, 0])
def test_the_run(E, chunk):
    res, p = run_q(E, chunk), plain(E)
    # it is that run: stats, totals, hist and the kept arrays are tolerance_mc's bytes for the seed
    assert run_bytes(res) == run_bytes(p) and res.n_ok == RUN_SAMPLES and not hasattr(p, "quantiles")
    # the quantiles are the selection alone on the run's kept rows: the device form, the host form, the restatement
    rc, dev = device_quantiles(E, res.m, res.flags, res.ok, RUN_PROBS, RUN_Z)
    host = E.mc_quantiles(res.m, res.flags, res.ok, RUN_PROBS, RUN_Z)
    if "run_ref" not in _CACHE:
        _CACHE["run_ref"] = R.quantiles(res.m, res.flags, res.ok, RUN_PROBS, RUN_Z)
    assert rc == 0 and res.quantiles.shape == (M5, len(RUN_PROBS))
    assert res.quantiles.tobytes() == dev.tobytes() == host.tobytes() == _CACHE["run_ref"].tobytes()
    for name in ("value", "lo", "hi", "band_lo", "band_hi"):
        assert getattr(res, "q_" + name).tobytes() == res.quantiles[name].tobytes()
    # what the numbers say: the constant record is its value everywhere; the extremes are min and max
    assert np.all(res.quantiles["n_valid"] == res.n_valid[:, None]) and np.all(res.q_value[2] == res.min[2]) and res.min[2] == res.max[2]
    assert res.q_value[:, 3].tobytes() == res.min.tobytes() and res.q_value[:, 4].tobytes() == res.max.tobytes()
    if chunk == 0:  # both chunks give the same bytes
        assert res.quantiles.tobytes() == run_q(E, 256).quantiles.tobytes() and run_bytes(res) == run_bytes(run_q(E, 256))


def test_the_device_form_on_another_stream_equals_the_host_form(E):
    import torch

    s, res = system16(E), run_q(E, 256)
    x0 = torch.from_numpy(X16).cuda()
    out = lambda n: torch.full((max(n, 1),), 0x5A, dtype=torch.uint8, device="cuda")  # noqa: E731
    raw = lambda t: t.cpu().numpy().tobytes()  # noqa: E731
    stream = torch.cuda.Stream()
    for kept in (True, False):  # the rows in the caller's keep buffers, then in the plan's workspace
        stats, totals, hist, quant = out(M5 * 88), out(24), out(M5 * 18 * 8), out(M5 * len(RUN_PROBS) * 80)
        kp, km, kflags, kok = out(8 * RUN_SAMPLES * 4), out(8 * RUN_SAMPLES * M5), out(RUN_SAMPLES * M5), out(RUN_SAMPLES)
        keep = dict(keep_params_ptr=kp.data_ptr(), keep_m_ptr=km.data_ptr(), keep_flags_ptr=kflags.data_ptr(), keep_ok_ptr=kok.data_ptr()) if kept else {}
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s.tolerance_mc_device(x0.data_ptr(), POS4, dists_of(E, DISTS4), RECORDS5, RUN_SAMPLES, stats.data_ptr(), totals.data_ptr(), hist.data_ptr(),
                                  seed=SEED, chunk=256, limits=RUN_LIMITS, hist=RUN_HIST, stream=stream.cuda_stream, quantiles=RUN_PROBS,
                                  quantile_z=RUN_Z, quantiles_ptr=quant.data_ptr(), **keep)
        stream.synchronize()
        assert [raw(t) for t in (stats, totals, hist)] == [res.stats.tobytes(), res.totals.tobytes(), res.hist.tobytes()], kept
        assert raw(quant) == res.quantiles.tobytes(), kept
        if kept:
            assert [raw(t) for t in (kp, km, kflags, kok)] == [res.params.tobytes(), res.m.tobytes(), res.flags.tobytes(), res.ok.tobytes()]
    # the run's argument errors touch nothing
    quant = out(M5 * 80)
    for bad in (dict(quantiles=[1.5]), dict(quantiles=[0.5], quantile_z=-1.0), dict(quantiles=[0.5] * 17)):
        with pytest.raises(E.NonLinearSystemError):
            s.tolerance_mc_device(x0.data_ptr(), POS4, dists_of(E, DISTS4), RECORDS5, RUN_SAMPLES, stats.data_ptr(), totals.data_ptr(), 0, seed=SEED,
                                  quantiles_ptr=quant.data_ptr(), **bad)
    with pytest.raises(E.NonLinearSystemError):
        s.tolerance_mc_device(x0.data_ptr(), POS4, dists_of(E, DISTS4), RECORDS5, RUN_SAMPLES, stats.data_ptr(), totals.data_ptr(), 0, seed=SEED,
                              quantiles=[0.5], quantiles_ptr=0)
    torch.cuda.synchronize()
    assert np.all(quant.cpu().numpy() == 0x5A) and raw(stats) == res.stats.tobytes()
    with pytest.raises(ValueError):
        s.tolerance_mc(X16, POS4, dists_of(E, DISTS4), RECORDS5, 10, contributors=True, quantiles=[0.5])


# ---- variants that do not assemble: the triangle of tests/test_sobol_cpu.py -----------------------------------------------------------
TRI_MEASURE = O.stack([O.vertical_distance((4, 5), (0, 1), 0.0), O.distance((2, 3), (4, 5), 0.0)])


def test_variants_that_do_not_assemble_are_left_out(E):
    rc, x0, _, conv, nun = O.solve_batch(triangle(TRI_NOMINAL), TRI_START)
    assert rc == 0 and conv[0] and nun[0] == 0
    s = E.System(triangle(TRI_NOMINAL), 6)
    probs = [0.0, 0.1, 0.5, 0.9, 1.0]
    res = s.tolerance_mc(x0[0], TRI_POS, dists_of(E, TRI_DISTS), TRI_MEASURE, TRI_SAMPLES, seed=TRI_SEED, keep=True, quantiles=probs, quantile_z=2.0)
    print("ok samples of the triangle:", res.n_ok, "of", TRI_SAMPLES, "; n_valid", res.n_valid.tolist())
    assert 0 < res.n_ok < TRI_SAMPLES and np.all(res.quantiles["n_valid"] == res.stats["n_valid"][:, None])
    good = res.ok != 0
    assert res.quantiles.tobytes() == R.quantiles(res.m[good], res.flags[good], None, probs, 2.0).tobytes()  # of the ok samples only
    assert res.quantiles.tobytes() == R.quantiles(res.m, res.flags, res.ok, probs, 2.0).tobytes()
    assert res.q_value[:, 0].tobytes() == res.min.tobytes() and res.q_value[:, 4].tobytes() == res.max.tobytes()


# ---- the curved case --------------------------------------------------------------------------------------------------------------
HV, CURVED_SAMPLES = 0.35, 16384
POINT = O.stack([O.fixed(0, 1.0), O.fixed(1, 0.0), O.fixed(2, 0.0), O.fixed(3, 0.0)])  # the point (0, 1) and the origin (2, 3)
POINT_X0 = np.array([1.0, 0.0, 0.0, 0.0])
CURVED_PROBS = [0.00135, 0.5, 0.99865]


def test_the_curved_case(E):
    s = E.System(POINT, 4)
    res = s.tolerance_mc(POINT_X0, [0, 1], dists_of(E, [(mc_ref.FIXED, 0.0, 0.0), (mc_ref.UNIFORM, -HV, HV)]),
                         O.stack([O.distance((2, 3), (0, 1), 0.0)]), CURVED_SAMPLES, seed=SEED, quantiles=CURVED_PROBS, quantile_z=6.0)
    assert res.n_ok == CURVED_SAMPLES and np.all(res.quantiles["n_valid"] == CURVED_SAMPLES)
    mean, std = float(res.mean[0]), float(res.std[0])
    print("mean", mean, "std", std, "mean - 3 std", mean - 3 * std, "q(0.00135)", res.q_value[0, 0])
    assert mean - 3 * std < 1.0 <= res.q_value[0, 0]
    for q, p in enumerate(CURVED_PROBS):
        exact = np.sqrt(1.0 + (HV * p) ** 2)
        print("p", p, "exact", exact, "band", res.q_band_lo[0, q], res.q_band_hi[0, q], "value", res.q_value[0, q])
        assert res.q_band_lo[0, q] <= exact <= res.q_band_hi[0, q], p
