"""GPU tests (-m gpu) of the Monte-Carlo tolerance analysis (ezpz_system_tolerance_mc and its _device form; csrc/tolerance_mc.hip):
the run is the chain of the entries it is made of -- the host sampler, solve_batch_params, measure -- the statistics are the sums
tests/mc_ref.py states, bit for bit, on the device's own samples, and cutting the run into rounds changes no byte.  Variants that
do not assemble are held to the oracle's verdicts.  Every case is small: the shapes are the boundaries of a block of 256 samples
and of a round, not the workload's.

Bars.  keep_params against ezpz_mc_sample: bitwise for FIXED, UNIFORM and CORNER, 1e-13 * sigma + 2^-52 * |p| for NORMAL (the bar
of tests/test_tolerance_mc_cpu.py, there derived).  Everything else: bytes."""
import ctypes as C

import numpy as np
import pytest

import mc_ref as R
import measure_ref as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
# csrc/call_trace.hpp: the symbolic phase of a system's first request (analysis and its tables; no launch) -- every other stamp is
# a stage of a call that launches
COLD_STAMPS = {20, 21, 22, 23}
KINDS13 = M.SUBTRACTING + M.CURVED
N16 = 16
SEED = 0xC0FFEE1234


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


def _trace(E, call):
    """(what call() returned, the stamps of csrc/call_trace.hpp it left: ids only)."""
    trace = np.zeros(256, dtype=np.uint64)
    E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
    try:
        out = call()
    finally:
        k = E.lib().ezpz_debug_call_trace(None, 0)
    return out, [int(v) for v in trace[:k:2]]


# ---- the 16-variable system: all Fixed, every parameter driven; the 46-record list of every measurable kind and tag -----------
def _record(rng, kind, tag, n_vars=N16):
    return O._mk(kind, list(rng.permutation(n_vars)[: O.KIND_NUM_IDS[kind]]), 0.0, tag=tag)


def _all46():
    rng = np.random.default_rng(46)
    pairs = [(k, t) for k in KINDS13 for t in range(4) if k not in M.ANGLES or t in (O.ANGLE_OTHER_DEG, O.ANGLE_OTHER_RAD)]
    assert len(pairs) == 46
    return O.stack([_record(rng, k, t) for k, t in pairs])


ALL46 = _all46()
_rng = np.random.default_rng(7)
X16 = _rng.uniform(0.5, 3.0, N16) * _rng.choice([-1.0, 1.0], N16) + np.arange(N16) * 0.37  # the nominal values, and the nominal solution
POS16 = list(range(N16))
# (kind, a, b) per dimension: mixed kinds
DISTS16 = [[(R.UNIFORM, -0.2, 0.2), (R.NORMAL, 0.1, 0.0), (R.NORMAL, 0.15, 1.5), (R.CORNER, -0.1, 0.1), (R.FIXED, 0.0, 0.0)][j % 5]
           for j in range(N16)]
_CACHE = {}


def dists_of(E, tuples):
    return [E.McDist(*t) for t in tuples]


def system16(E):
    if "s16" not in _CACHE:
        _CACHE["s16"] = E.System(O.stack([O.fixed(v, float(X16[v])) for v in range(N16)]), N16)
    return _CACHE["s16"]


def nominal46(E):
    """m(record, X16) by the measure entry: what the statistics' `nominal` has to be, and what the ranges below are built around."""
    if "nom" not in _CACHE:
        _CACHE["nom"] = system16(E).measure(X16[None, :], ALL46)[0]
    return _CACHE["nom"]


def ranges(E):
    """limits that cut through the samples, and 16 bins that leave values under and over."""
    nom = nominal46(E)
    return (nom - 0.03, nom + 0.04), (nom - 0.05, nom + 0.08, 16)


def run16(E, samples, chunk=0):
    key = ("run", samples, chunk)
    if key not in _CACHE:
        limits, hist = ranges(E)
        _CACHE[key] = system16(E).tolerance_mc(X16, POS16, dists_of(E, DISTS16), ALL46, samples, seed=SEED, limits=limits, hist=hist,
                                               chunk=chunk, keep=True)
    return _CACHE[key]


def assert_draws(got, want, dists):
    kinds = np.array([d[0] for d in dists])
    exact = kinds != R.NORMAL
    assert got[:, exact].tobytes() == want[:, exact].tobytes()
    sigma = np.array([d[1] if d[0] == R.NORMAL else 0.0 for d in dists])
    assert np.all(np.abs(got - want) <= 1e-13 * sigma + 2.0 ** -52 * np.abs(want))


def result_bytes(res, keep=True):
    out = [res.stats.tobytes(), res.totals.tobytes(), res.hist.tobytes() if res.hist is not None else b""]
    return out + ([res.params.tobytes(), res.m.tobytes(), res.flags.tobytes(), res.ok.tobytes()] if keep else [])


def assert_statistics_are_the_reference(res, limits, hist):
    stats, totals, counts = R.statistics(res.m, res.flags, res.ok, res.nominal, limits, hist)
    for f in R.STATS_DTYPE.names:
        assert res.stats[f].tobytes() == stats[f].tobytes(), (f, res.stats[f], stats[f])
    assert res.totals.tobytes() == totals.tobytes(), (res.totals, totals)
    if hist is not None:
        assert res.hist.tobytes() == counts.tobytes()


def test_the_run_is_the_chain(E):
    s, res = system16(E), run16(E, 600)
    assert_draws(res.params, E.mc_sample(SEED, dists_of(E, DISTS16), X16, 0, 600), DISTS16)
    x, st, _ = s.solve_batch_params(np.tile(X16, (600, 1)), POS16, res.params)
    assert np.array_equal((st["converged"] != 0) & (st["n_unsatisfied"] == 0), res.ok != 0)
    assert res.ok.all() and res.n_ok == 600  # (a Fixed system takes every value)
    m, flags = s.measure(x, ALL46, want_flags=True)
    assert m.tobytes() == res.m.tobytes() and flags.tobytes() == res.flags.tobytes()
    assert res.nominal.tobytes() == nominal46(E).tobytes()


@pytest.mark.parametrize("samples", [1, 255, 256, 257, 1000])
def test_the_statistics_are_the_stated_sums(E, samples):
    res = run16(E, samples)
    limits, hist = ranges(E)
    assert res.samples == samples and res.m.shape == (samples, 46)
    assert_statistics_are_the_reference(res, limits, hist)
    assert np.array_equal(res.std, np.sqrt(res.var), equal_nan=True)
    if samples == 1000:  # the inputs reach what they are meant to: values under, inside and over the bins, limits that cut
        assert res.hist[:, 0].sum() > 0 and res.hist[:, -1].sum() > 0 and res.hist[:, 1:-1].sum() > 0
        assert np.any((res.n_in > 0) & (res.n_in < res.n_valid)) and 0 <= res.n_all_in < samples
        assert np.all(res.hist.sum(axis=1) == res.n_valid)


def test_cutting_the_run_changes_nothing(E):
    want = result_bytes(run16(E, 1000, chunk=0))
    for chunk in (256, 512, 300):  # (300 rounds up to 512)
        assert result_bytes(run16(E, 1000, chunk=chunk)) == want, chunk


def test_device_form_on_another_stream_equals_the_host_form(E):
    import torch

    s, res = system16(E), run16(E, 1000)
    limits, hist = ranges(E)
    x0 = torch.from_numpy(X16).cuda()
    out = lambda n: torch.full((max(n, 1),), 0x5A, dtype=torch.uint8, device="cuda")  # noqa: E731
    stats, totals, counts = out(46 * 88), out(24), out(46 * 18 * 8)
    kp, km, kf, ko = out(1000 * N16 * 8), out(1000 * 46 * 8), out(1000 * 46), out(1000)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s.tolerance_mc_device(x0.data_ptr(), POS16, dists_of(E, DISTS16), ALL46, 1000, stats.data_ptr(), totals.data_ptr(), counts.data_ptr(),
                              seed=SEED, limits=limits, hist=hist, chunk=256, keep_params_ptr=kp.data_ptr(), keep_m_ptr=km.data_ptr(),
                              keep_flags_ptr=kf.data_ptr(), keep_ok_ptr=ko.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    got = [t.cpu().numpy().tobytes() for t in (stats, totals, counts, kp, km, kf, ko)]
    assert got == result_bytes(res)


# ---- the kinds of run share a system's plan: what one leaves in it changes no byte of the next ------------------------------------
RECS6 = ALL46[:6]
SMOOTH16 = [(R.UNIFORM, -0.2, 0.2) if d[0] == R.CORNER else d for d in DISTS16]  # (the Sobol run takes no CORNER dimension)
CORNERS16 = [(R.CORNER, -0.1, 0.1)] * 3 + [(R.FIXED, 0.0, 0.0)] * (N16 - 3)


def _contrib_on_a_second_stream(E, s):
    import torch

    K = N16 + 6
    x0 = torch.from_numpy(X16).cuda()
    sizes = (6 * 88, 24, (K + K * (K + 1) // 2) * 8, 16, K * K * 8, 6 * N16 * 8, 6 * N16 * 8, 6 * 8, 8)  # stats .. dropped
    out = [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in sizes]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s.tolerance_mc_device(x0.data_ptr(), POS16, dists_of(E, DISTS16), RECS6, 257, out[0].data_ptr(), out[1].data_ptr(), seed=SEED, chunk=256,
                              stream=stream.cuda_stream, **{name: t.data_ptr() for name, t in zip(
                                  ("moments_ptr", "info_ptr", "cov_ptr", "beta_ptr", "contrib_ptr", "r2_ptr", "dropped_ptr"), out[2:])})
    stream.synchronize()
    return [t.cpu().numpy().tobytes() for t in out]


def _kind_calls(E):
    """name -> call(system) -> every output of the call as bytes."""
    def run(samples=257, dists=DISTS16, keep=False, also=(), **kind):
        def call(s):
            res = s.tolerance_mc(X16, POS16, dists_of(E, dists), RECS6, samples, seed=SEED, chunk=256, keep=keep, **kind)
            return result_bytes(res, keep) + [np.ascontiguousarray(get(res)).tobytes() for get in also]
        return call

    def part(owner, *names):
        return [lambda res, n=n: getattr(getattr(res, owner) if owner else res, n) for n in names]

    def sobol(s):
        res = s.tolerance_sobol(X16, POS16, dists_of(E, SMOOTH16), RECS6, 257, seed=SEED, chunk=256, keep=True)
        return [np.ascontiguousarray(a).tobytes() for a in (res.stats, res.totals, res.sums, res.n_complete, res.var, res.first, res.total,
                                                            res.first_var, res.total_var, res.f, res.flags, res.ok)]

    quantiles = dict(quantiles=[0.0, 0.1, 0.5, 1.0], quantile_z=2.0, also=part("", "quantiles"))
    return {"plain": run(keep=True),
            "contributors": lambda s: _contrib_on_a_second_stream(E, s),
            "quantiles": run(**quantiles),
            "effects": run(effects=E.EffectsConfig(8), also=part("effects", "sums", "counts", "edges", "cond_mean", "cond_var", "eta2", "first",
                                                                  "bins_used")),
            "factorial": run(samples=8, dists=CORNERS16, factorial=True, also=part("factorial", "info", "main", "pair", "ss_order", "ss_total",
                                                                                   "first", "total")),
            "sobol": sobol,
            "quantiles of 600": run(samples=600, **quantiles)}


def test_the_kinds_share_a_plan(E):
    """Two rounds a run, the second of one sample.  Every kind after every other on ONE system -- the six in order, then in reverse
    order, then the quantiles on rows that have to grow after the factorial run has used them -- gives, output for output and byte
    for byte, what the same call gives on a system that has run nothing else."""
    calls = _kind_calls(E)
    fixed16 = O.stack([O.fixed(v, float(X16[v])) for v in range(N16)])
    want = {name: call(E.System(fixed16, N16)) for name, call in calls.items()}
    shared = E.System(fixed16, N16)
    six = list(calls)[:6]
    for name in six + six[::-1] + ["quantiles of 600"]:
        assert calls[name](shared) == want[name], name


# ---- variants that do not assemble: a triangle whose third side can outgrow the other two --------------------------------------
A, B, Cc = (0, 1), (2, 3), (4, 5)
TRIANGLE = O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(3, 0.0), O.distance(A, B, 1.0), O.distance(B, Cc, 1.0), O.distance(Cc, A, 1.9)])
TRI_POS, TRI_NOMINAL = [3, 4, 5], np.array([1.0, 1.0, 1.9])
TRI_DISTS = [(R.UNIFORM, -0.05, 0.05), (R.UNIFORM, -0.05, 0.05), (R.UNIFORM, -0.3, 0.3)]
TRI_MEASURE = O.stack([O.vertical_distance(Cc, A, 0.0), O.distance(B, Cc, 0.0)])


def triangle(E):
    if "tri" not in _CACHE:
        rc, x0, _, conv, nun = O.solve_batch(TRIANGLE, np.array([[0.0, 0.0, 1.0, 0.0, 0.9, 0.4]]))
        assert rc == 0 and conv[0] and nun[0] == 0
        _CACHE["tri"] = (E.System(TRIANGLE, 6), x0[0])
    return _CACHE["tri"]


def test_variants_that_do_not_assemble_are_counted_not_averaged(E):
    s, x0 = triangle(E)
    p = E.mc_sample(SEED, dists_of(E, TRI_DISTS), TRI_NOMINAL, 0, 600)
    verdict = np.zeros(600, bool)
    recs = TRIANGLE.copy()
    for b in range(600):
        recs["param"][TRI_POS] = p[b]
        rc, _, _, conv, nun = O.solve_batch(recs, x0[None, :])
        assert rc == 0
        verdict[b] = bool(conv[0]) and nun[0] == 0
    assert (~verdict).sum() >= 100 and verdict.sum() >= 300
    res = s.tolerance_mc(x0, TRI_POS, dists_of(E, TRI_DISTS), TRI_MEASURE, 600, seed=SEED, keep=True)  # (nominal: the system's own)
    assert res.params.tobytes() == p.tobytes()
    clear = np.abs(p[:, 2] - p[:, 0] - p[:, 1]) > 1e-3
    assert clear.sum() >= 500 and np.array_equal(res.ok[clear] != 0, verdict[clear])
    n_ok = int(np.count_nonzero(res.ok))
    assert res.n_ok == n_ok and res.n_valid.tolist() == [n_ok, n_ok] and res.n_in.tolist() == [n_ok, n_ok] and res.n_all_in == n_ok
    assert res.ok[int(res.argmax[1])] and res.ok[int(res.argmin[1])]
    assert_statistics_are_the_reference(res, None, None)  # (the leaves of the failed samples are +0.0)


def test_a_degenerate_measurement_is_left_out_per_record(E):
    # a line from (1, 1) to (1 + deviation, 1): deviation 0 puts its second point on top of its first
    values = np.array([0.3, 0.7, 1.0, 1.0, 1.0, 1.0])
    s = E.System(O.stack([O.fixed(v, float(values[v])) for v in range(6)]), 6)
    dists = dists_of(E, [(R.FIXED, 0.0, 0.0)] * 4 + [(R.CORNER, 0.0, 1.0), (R.FIXED, 0.0, 0.0)])
    records = O.stack([O.point_line_distance((0, 1), (2, 3), (4, 5), 0.0), O.distance((0, 1), (2, 3), 0.0)])
    res = s.tolerance_mc(values, list(range(6)), dists, records, 8, keep=True)
    assert res.n_ok == 8 and res.params[:, 4].tolist() == [1.0, 2.0] * 4
    assert (res.flags[:, 0] & 1).tolist() == [1, 0] * 4 and not res.flags[:, 1].any()
    assert res.n_valid.tolist() == [4, 8] and res.n_all_in == 4
    assert res.nominal[0] == 0.0 and res.argmin.tolist() == [1, 0]  # (the nominal point is degenerate itself: 0 where the guard fires)
    assert_statistics_are_the_reference(res, None, None)


def test_no_valid_sample_and_one(E):
    s, x0 = triangle(E)
    # a third side of 3 against two of 1: no variant assembles
    res = s.tolerance_mc(x0, TRI_POS, dists_of(E, [(R.FIXED, 0.0, 0.0)] * 3), TRI_MEASURE, 300, nominal=[1.0, 1.0, 3.0], hist=(0.0, 1.0, 4))
    assert res.samples == 300 and res.n_ok == 0 and res.n_all_in == 0
    assert res.n_valid.tolist() == [0, 0] and res.n_in.tolist() == [0, 0] and not res.hist.any()
    assert np.isnan(res.mean).all() and np.isnan(res.var).all() and np.isnan(res.std).all()
    assert np.all(res.min == np.inf) and np.all(res.max == -np.inf)
    assert res.argmin.tolist() == [R.UINT64_MAX] * 2 and res.argmax.tolist() == [R.UINT64_MAX] * 2
    assert res.sum_d.tolist() == [0.0, 0.0] and res.sum_d2.tolist() == [0.0, 0.0]
    # one sample.  Each record reads one Fixed variable of magnitude >= 0.5 moved by at most 0.2: m / 2 <= nominal <= 2 m, so
    # d = m - nominal is exact (Sterbenz) and mean = nominal + d is m itself
    read = [v for v in range(N16) if abs(X16[v]) >= 0.5][:4]
    assert len(read) == 4
    records = O.stack([O.fixed(v, 0.0) for v in read])
    one = system16(E).tolerance_mc(X16, POS16, dists_of(E, [(R.UNIFORM, -0.2, 0.2)] * N16), records, 1, seed=3, keep=True)
    assert one.n_valid.tolist() == [1] * 4 and np.isnan(one.var).all()
    assert one.mean.tobytes() == one.min.tobytes() == one.max.tobytes() == one.m[0].tobytes()
    assert one.argmin.tolist() == [0] * 4 and one.argmax.tolist() == [0] * 4 and np.all(one.m[0] != X16[read])


# ---- argument errors: the return code, no output touched, nothing launched ------------------------------------------------------
N22 = 22


def _error_case(E, what):
    """The arguments of a legal host call on a 22-variable Fixed system (21 CORNER dimensions need 21 driven constraints), with
    one thing wrong."""
    if "s22" not in _CACHE:
        cons = [O.fixed(v, 1.0 + v) for v in range(N22)] + [O.vertical((0, 1), (2, 3))]  # (the last one has no parameter)
        _CACHE["s22"] = E.System(O.stack(cons), N22)
    a = dict(sys=_CACHE["s22"], x0=1.0 + np.arange(N22), positions=np.arange(4, dtype=np.uint32), dist=[(R.UNIFORM, -0.1, 0.1)] * 4,
             nominal=np.ones(4), records=O.stack([O.fixed(0, 0.0), O.distance((0, 1), (2, 3), 0.0)]), lim_lo=np.zeros(2), lim_hi=np.ones(2),
             hist_lo=np.zeros(2), hist_hi=np.ones(2), samples=300, bins=8, stats=True, totals=True, n_param=None, n_meas=None)
    bad = {
        "position >= n_cs": dict(positions=np.array([0, 1, 2, N22 + 1], np.uint32)),
        "position listed twice": dict(positions=np.array([0, 1, 2, 1], np.uint32)),
        "position without a parameter": dict(positions=np.array([0, 1, 2, N22], np.uint32)),
        "positions NULL": dict(positions=None, n_param=4),
        "record not measurable": dict(records=O.stack([O.fixed(0, 0.0), O.vertical((0, 1), (2, 3))])),
        "record id >= n_vars": dict(records=O.stack([O.fixed(0, 0.0), O.distance((0, 1), (2, N22), 0.0)])),
        "records NULL": dict(records=None, n_meas=2),
        "dist NULL": dict(dist=None, n_param=4),
        "unknown kind": dict(dist=[(R.UNIFORM, -0.1, 0.1)] * 3 + [(7, 0.0, 0.0)]),
        "non-finite a": dict(dist=[(R.UNIFORM, -np.inf, 0.1)] * 4),
        "non-finite nominal": dict(nominal=np.array([1.0, np.nan, 1.0, 1.0])),
        "uniform a > b": dict(dist=[(R.UNIFORM, 0.2, 0.1)] * 4),
        "sigma < 0": dict(dist=[(R.NORMAL, -0.1, 0.0)] * 4),
        "truncation in (0, 1)": dict(dist=[(R.NORMAL, 0.1, 0.5)] * 4),
        "21 corners": dict(positions=np.arange(21, dtype=np.uint32), dist=[(R.CORNER, 0.0, 0.1)] * 21, nominal=np.ones(21)),
        "hist_bins > 64": dict(bins=65),
        "bins without ranges": dict(hist_lo=None, hist_hi=None),
        "bins with one range": dict(hist_hi=None),
        "hist_hi <= hist_lo": dict(hist_hi=np.array([1.0, 0.0])),
        "one limit array": dict(lim_hi=None),
        "lim_lo > lim_hi": dict(lim_lo=np.array([0.0, 2.0])),
        "stats NULL": dict(stats=False),
        "totals NULL": dict(totals=False),
    }
    a.update(bad[what])
    return a


ERROR_CASES = ["position >= n_cs", "position listed twice", "position without a parameter", "positions NULL", "record not measurable",
               "record id >= n_vars", "records NULL", "dist NULL", "unknown kind", "non-finite a", "non-finite nominal", "uniform a > b",
               "sigma < 0", "truncation in (0, 1)", "21 corners", "hist_bins > 64", "bins without ranges", "bins with one range",
               "hist_hi <= hist_lo", "one limit array", "lim_lo > lim_hi", "stats NULL", "totals NULL"]


def _raw_host_call(E, a, outputs):
    from ezpz_amd._lib import CMcConfig

    ptr = lambda v: v.ctypes.data if v is not None else None  # noqa: E731
    d = E.api.mc_dists(dists_of(E, a["dist"])) if a["dist"] is not None else None
    n_param = a["n_param"] if a["n_param"] is not None else len(a["positions"])
    n_meas = a["n_meas"] if a["n_meas"] is not None else len(a["records"])
    mc, cfg = CMcConfig(1, 0, a["bins"]), E.Config()._c()
    stats, totals, hist, kp, km, kf, ko = outputs
    return E.lib().ezpz_system_tolerance_mc(a["sys"]._h, ptr(a["x0"]), ptr(a["positions"]), n_param, ptr(d), ptr(a["nominal"]), ptr(a["records"]),
                                            n_meas, ptr(a["lim_lo"]), ptr(a["lim_hi"]), ptr(a["hist_lo"]), ptr(a["hist_hi"]), a["samples"],
                                            C.byref(mc), C.byref(cfg), ptr(stats) if a["stats"] else None, ptr(totals) if a["totals"] else None,
                                            ptr(hist), ptr(kp), ptr(km), ptr(kf), ptr(ko))


def _outputs():
    return [np.full(n, 0xA5, np.uint8) for n in (2 * 88, 24, 2 * 66 * 8, 300 * 21 * 8, 300 * 2 * 8, 300 * 2, 300)]


@pytest.mark.parametrize("what", ERROR_CASES)
def test_argument_errors(E, what):
    outputs = _outputs()
    rc, stamps = _trace(E, lambda: _raw_host_call(E, _error_case(E, what), outputs))
    assert rc == ERR_INVALID_ARGUMENT and not set(stamps) - COLD_STAMPS, (what, rc, stamps)
    assert all(np.all(o == 0xA5) for o in outputs), what


def test_the_legal_call_of_the_error_cases_and_the_empty_ones(E):
    # the same arguments with nothing wrong run (so each case above fails for its one reason), and leave their stamps
    a = _error_case(E, "stats NULL")
    a["stats"] = True
    outputs = _outputs()
    rc, stamps = _trace(E, lambda: _raw_host_call(E, a, outputs))
    assert rc == 0 and 61 in stamps and 51 in stamps, (rc, stamps)
    totals = outputs[1].view(R.TOTALS_DTYPE)
    assert totals["samples"][0] == 300 and totals["n_ok"][0] <= 300
    # samples == 0: EZPZ_OK, nothing written, nothing launched -- but still an error where the request is wrong
    outputs = _outputs()
    a["samples"] = 0
    rc, stamps = _trace(E, lambda: _raw_host_call(E, a, outputs))
    assert rc == 0 and not set(stamps) - COLD_STAMPS and all(np.all(o == 0xA5) for o in outputs)
    a["bins"] = 65
    assert _raw_host_call(E, a, outputs) == ERR_INVALID_ARGUMENT
    # n_param == 0: every sample is the same solve
    s = system16(E)
    res = s.tolerance_mc(X16, [], [], ALL46[:3], 300, keep=True)
    assert res.n_ok == 300 and res.params.shape == (300, 0) and np.all(res.m == res.m[0]) and res.min.tobytes() == res.max.tobytes()


def test_device_form_argument_error_touches_nothing(E):
    import torch

    s = system16(E)
    stats, totals = (torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (46 * 88, 24))
    x0 = torch.from_numpy(X16).cuda()
    torch.cuda.synchronize()

    def call():
        with pytest.raises(E.NonLinearSystemError):
            s.tolerance_mc_device(x0.data_ptr(), POS16, dists_of(E, DISTS16), ALL46, 300, stats.data_ptr(), totals.data_ptr(),
                                  limits=(np.ones(46), np.zeros(46)))

    _, stamps = _trace(E, call)
    torch.cuda.synchronize()
    assert not set(stamps) - COLD_STAMPS and bool((stats == 0x5A).all()) and bool((totals == 0x5A).all())
