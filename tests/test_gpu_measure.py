"""GPU tests (-m gpu) of the reference dimensions (ezpz_system_measure, _measure_response, _measure_vjp and their _device forms;
csrc/measure.hip.hpp) against the host function ezpz_constraint_measure (itself held to the oracle by tests/test_measure_cpu.py)
and the sequential loops of tests/measure_ref.py.  Every case is small: the shapes are the boundaries -- past one wavefront, past
a workgroup, past the LDS table, both placements -- not the workload's.

Bars.  Against the host function: bitwise for the kinds that call no libm function; 1e-11 * max(1, |m|) and 1e-10 * max(1,
|grad|inf) for the others (the project's residual and Jacobian parity bars).  D and grad_x: 1e-10 * the sum of the |terms| of each
sum.  worst: bitwise against the sequential loop on the device's own D; rss: within 2 ulp of it.  Meaning: see the two tests."""
import ctypes as C

import numpy as np
import pytest

import measure_ref as M
import sensitivity_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
UPLOADED, LAUNCHED, ROW, DIRECT = 50, 51, 52, 53
KINDS13 = M.SUBTRACTING + M.CURVED
N16 = 16


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


@pytest.fixture(autouse=True)
def _route(monkeypatch):
    monkeypatch.delenv("EZPZ_MEASURE_ROUTE", raising=False)


def _trace(E, call):
    """(what call() returned, the stamps of csrc/call_trace.hpp it left: ids only)."""
    trace = np.zeros(64, dtype=np.uint64)
    E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
    try:
        out = call()
    finally:
        k = E.lib().ezpz_debug_call_trace(None, 0)
    return out, [int(v) for v in trace[:k:2]]


# ---- the 16-variable system, its lists and values, and the host function's answers (computed once) -----------------------------
def _record(rng, kind, tag, n_vars=N16):
    return O._mk(kind, list(rng.permutation(n_vars)[: O.KIND_NUM_IDS[kind]]), 0.0, tag=tag)


def _lists():
    rng = np.random.default_rng(46)
    pairs = [(k, t) for k in KINDS13 for t in range(4) if k not in M.ANGLES or t in (O.ANGLE_OTHER_DEG, O.ANGLE_OTHER_RAD)]
    assert len(pairs) == 46
    all46 = O.stack([_record(rng, k, t) for k, t in pairs])
    list300 = O.stack([_record(rng, *pairs[int(rng.integers(0, 46))]) for _ in range(300)])
    return all46, list300


ALL46, LIST300 = _lists()
BOTH = np.concatenate([ALL46, LIST300])
BATCHES = (1, 63, 64, 65, 130, 1025)


def _values(batch, seed=7):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 3.0, (batch, N16)) * rng.choice([-1.0, 1.0], (batch, N16)) + np.arange(N16) * 0.37


X = _values(max(BATCHES))
_HOST = {}


def host_answers(E, recs, x):
    """(m [batch, k], grad [batch, k, 8], flags [batch, k]) by ezpz_constraint_measure, one call per (system, record)."""
    fn = E.lib().ezpz_constraint_measure
    x = np.ascontiguousarray(x)
    m, grad, flags = np.zeros((len(x), len(recs))), np.zeros((len(x), len(recs), 8)), np.zeros((len(x), len(recs)), np.uint8)
    one, fl = C.c_double(0.0), C.c_int(0)
    rec_ptrs = [recs[i:i + 1].ctypes.data for i in range(len(recs))]
    for b in range(len(x)):
        xp = x[b].ctypes.data
        for i, rp in enumerate(rec_ptrs):
            assert fn(rp, xp, C.byref(one), grad[b, i].ctypes.data, C.byref(fl)) > 0
            m[b, i], flags[b, i] = one.value, fl.value
    return m, grad, flags


def host16(E):
    if "x16" not in _HOST:
        _HOST["x16"] = host_answers(E, BOTH, X)
    return _HOST["x16"]


def system16(E):
    if "s16" not in _HOST:
        _HOST["s16"] = E.System(O.stack([O.fixed(v, 0.0) for v in range(N16)]), N16)
    return _HOST["s16"]


def assert_equals_host(recs, got, want, what):
    (m, grad, flags), (hm, hg, hf) = got, want
    assert np.array_equal(flags, hf), what
    exact = np.isin(recs["kind"], M.NO_LIBM)
    assert m[:, exact].tobytes() == hm[:, exact].tobytes() and grad[:, exact].tobytes() == hg[:, exact].tobytes(), what
    assert np.all(np.abs(m - hm) <= 1e-11 * np.maximum(1.0, np.abs(hm))), what
    assert np.all(np.abs(grad - hg) <= 1e-10 * np.maximum(1.0, np.abs(hg).max(axis=2, keepdims=True))), what
    assert not np.any(np.signbit(grad[:, :, 6:][:, recs["kind"] != O.LINES_AT_ANGLE])), what  # slots past n_ids are +0.0


@pytest.mark.parametrize("route,stamp", [("row", ROW), ("direct", DIRECT)])
@pytest.mark.parametrize("batch", BATCHES)
def test_against_the_host_function(E, monkeypatch, route, stamp, batch):
    monkeypatch.setenv("EZPZ_MEASURE_ROUTE", route)
    s = system16(E)
    hm, hg, hf = host16(E)
    for recs, cols in ((ALL46, slice(0, 46)), (LIST300, slice(46, 346))):
        got, stamps = _trace(E, lambda: s.measure(X[:batch], recs, want_grad=True, want_flags=True))
        assert stamp in stamps and LAUNCHED in stamps, stamps
        assert_equals_host(recs, got, (hm[:batch, cols], hg[:batch, cols], hf[:batch, cols]), (route, batch, len(recs)))
        # only what was asked for: the same values
        assert s.measure(X[:batch], recs).tobytes() == got[0].tobytes()


@pytest.mark.parametrize("n_vars,stamp", [(2000, ROW), (9000, DIRECT)])
def test_long_rows_take_their_placement(E, monkeypatch, n_vars, stamp):
    """2000 variables can be staged in LDS, 9000 are above what ROW holds whatever the threshold: gathered from global memory even
    when ROW is asked for.  The placement the policy chooses by itself gives the same bits."""
    rng = np.random.default_rng(n_vars)
    s = E.System(O.stack([O.fixed(v, 0.0) for v in range(n_vars)]), n_vars)
    recs = O.stack([_record(rng, *[(k, t) for k in KINDS13 for t in (2, 3)][i % 26], n_vars=n_vars) for i in range(52)]
                   + [O._mk(O.DISTANCE, [n_vars - 4, n_vars - 3, n_vars - 2, n_vars - 1]), O._mk(O.FIXED, [n_vars - 1])])
    x = rng.uniform(0.5, 3.0, (3, n_vars)) * rng.choice([-1.0, 1.0], (3, n_vars)) + (np.arange(n_vars) % 8) * 0.37
    got, stamps = _trace(E, lambda: s.measure(x, recs, want_grad=True, want_flags=True))
    assert (ROW in stamps) != (DIRECT in stamps), stamps
    assert_equals_host(recs, got, host_answers(E, recs, x), n_vars)
    monkeypatch.setenv("EZPZ_MEASURE_ROUTE", "row")
    forced, stamps = _trace(E, lambda: s.measure(x, recs, want_grad=True, want_flags=True))
    assert stamp in stamps and all(a.tobytes() == b.tobytes() for a, b in zip(got, forced))
    monkeypatch.setenv("EZPZ_MEASURE_ROUTE", "direct")
    forced, stamps = _trace(E, lambda: s.measure(x, recs, want_grad=True, want_flags=True))
    assert DIRECT in stamps and all(a.tobytes() == b.tobytes() for a, b in zip(got, forced))


_FIXED_SYSTEMS = {}


def _fixed_system(E, n_vars):
    if n_vars not in _FIXED_SYSTEMS:
        _FIXED_SYSTEMS[n_vars] = E.System(O.stack([O.fixed(v, 0.0) for v in range(n_vars)]), n_vars)
    return _FIXED_SYSTEMS[n_vars]


def _against_host(E, n_vars, count, batch):
    """`count` records of all 46 kind x tag pairs in turn over `n_vars` variables at `batch` systems, held to the host function;
    returns the call's stamps."""
    rng = np.random.default_rng(1000 * n_vars + count)
    pairs = [(int(k), int(t)) for k, t in zip(ALL46["kind"], ALL46["tag"])]
    recs = O.stack([_record(rng, *pairs[i % 46], n_vars=n_vars) for i in range(count)])
    x = rng.uniform(0.5, 3.0, (batch, n_vars)) * rng.choice([-1.0, 1.0], (batch, n_vars)) + (np.arange(n_vars) % 8) * 0.37
    s = _fixed_system(E, n_vars)
    got, stamps = _trace(E, lambda: s.measure(x, recs, want_grad=True, want_flags=True))
    assert_equals_host(recs, got, host_answers(E, recs, x), (n_vars, count, batch))
    return stamps


@pytest.mark.parametrize("n_vars,count,batch", [(16, 600, 65), (7000, 300, 3)])
def test_row_with_the_table_left_in_global_memory(E, monkeypatch, n_vars, count, batch):
    """ROW keeps the record table in LDS up to 16 KiB (455 records) and while rows and table fit 64 KiB together: 600 records
    (21 600 bytes) are past the first limit, 300 records beside a row of 7000 variables (56 KB + 10.8 KB) past the second.  The
    lanes then read the table from global memory."""
    monkeypatch.setenv("EZPZ_MEASURE_ROUTE", "row")
    assert ROW in _against_host(E, n_vars, count, batch)


@pytest.mark.parametrize("n_vars", [15, 17])
def test_row_with_an_odd_number_of_variables(E, monkeypatch, n_vars):
    """Every other piece of rows then starts at an odd index: one double alone, the 16-byte loads shifted by one, and (where the
    piece's length is odd too) one double alone at its end.  65 systems: several systems per workgroup, pieces of both parities and a
    short last one."""
    monkeypatch.setenv("EZPZ_MEASURE_ROUTE", "row")
    assert ROW in _against_host(E, n_vars, 92, 65)
    assert ROW in _against_host(E, n_vars, 300, 1)


def test_the_policy_places_by_itself(E):
    """No EZPZ_MEASURE_ROUTE: 1024 variables lie inside the ROW window of csrc/policy.hpp (512 .. 1536), 16 and 2000 outside."""
    for n_vars, stamp, other in ((1024, ROW, DIRECT), (16, DIRECT, ROW), (2000, DIRECT, ROW)):
        stamps = _against_host(E, n_vars, 60, 5)
        assert stamp in stamps and other not in stamps, (n_vars, stamps)


def test_misaligned_device_pointers(E, monkeypatch):
    """x_dev or grad_out_dev at 8 modulo 16 bytes: ROW's 16-byte loads need an aligned x, so such a call takes DIRECT even when ROW is
    asked for, and the gradient's eight doubles leave as single stores -- the bits of the aligned call either way."""
    import torch

    monkeypatch.setenv("EZPZ_MEASURE_ROUTE", "row")
    s = system16(E)
    batch = 65
    want = s.measure(X[:batch], ALL46, want_grad=True, want_flags=True)
    xbuf = torch.zeros(batch * N16 + 1, dtype=torch.float64, device="cuda")
    gbuf = torch.full((batch * 46 * 8 + 1,), 9.0, dtype=torch.float64, device="cuda")
    flat = torch.tensor(X[:batch].reshape(-1), device="cuda")
    for x_off, g_off, stamp in ((1, 0, DIRECT), (0, 1, ROW), (1, 1, DIRECT)):
        xd, gd = xbuf[x_off:x_off + batch * N16], gbuf[g_off:g_off + batch * 46 * 8]
        xd.copy_(flat)
        gd.fill_(9.0)
        assert xd.data_ptr() % 16 == 8 * x_off and gd.data_ptr() % 16 == 8 * g_off
        m = torch.zeros((batch, 46), dtype=torch.float64, device="cuda")
        fl = torch.zeros((batch, 46), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _, stamps = _trace(E, lambda: s.measure_device(xd.data_ptr(), ALL46, batch, m.data_ptr(), fl.data_ptr(), gd.data_ptr()))
        torch.cuda.synchronize()
        assert stamp in stamps, (x_off, g_off, stamps)
        for got, w in zip((m, gd, fl), want):
            assert got.cpu().numpy().tobytes() == w.tobytes(), (x_off, g_off)


@pytest.mark.parametrize("route", ["row", "direct"])
def test_independence_and_determinism(E, monkeypatch, route):
    monkeypatch.setenv("EZPZ_MEASURE_ROUTE", route)
    s = system16(E)
    x = X[:130]
    whole = s.measure(x, ALL46, want_grad=True, want_flags=True)
    again = s.measure(x, ALL46, want_grad=True, want_flags=True)
    back = s.measure(x, ALL46[::-1].copy(), want_grad=True, want_flags=True)
    for a, b, c in zip(whole, again, back):
        assert a.tobytes() == b.tobytes() and a.tobytes() == np.ascontiguousarray(c[:, ::-1]).tobytes()
    for i in range(len(ALL46)):
        alone = s.measure(x[:3], ALL46[i:i + 1], want_grad=True, want_flags=True)
        for a, b in zip(whole, alone):
            assert np.ascontiguousarray(a[:3, i:i + 1]).tobytes() == b.tobytes(), i
    # one system alone, first, last and in the middle of a batch of 130
    one = s.measure(x[77:78], LIST300, want_grad=True, want_flags=True)
    for place in (0, 64, 129):
        moved = x.copy()
        moved[place] = x[77]
        got = s.measure(moved, LIST300, want_grad=True, want_flags=True)
        for a, b in zip(one, got):
            assert a[0].tobytes() == b[place].tobytes(), place


@pytest.mark.parametrize("route", ["row", "direct"])
def test_a_guarded_system_inside_a_batch(E, monkeypatch, route):
    monkeypatch.setenv("EZPZ_MEASURE_ROUTE", route)
    s = system16(E)
    guarded = [i for i in range(46) if int(ALL46["kind"][i]) in M.CURVED + (O.POINT_LINE_DISTANCE, O.VERTICAL_POINT_LINE_DISTANCE,
                                                                          O.HORIZONTAL_POINT_LINE_DISTANCE)]
    x = X[:65].copy()
    clean = s.measure(x, ALL46, want_grad=True, want_flags=True)
    x[31] = 1.25  # every point of the system on one spot: every guard there is fires
    m, grad, flags = s.measure(x, ALL46, want_grad=True, want_flags=True)
    assert np.all(flags[31, guarded] == 1) and np.all(m[31, guarded] == 0.0) and np.all(grad[31, guarded] == 0.0)
    dist = [i for i in range(46) if int(ALL46["kind"][i]) in (O.DISTANCE, O.ARC_RADIUS)]
    assert np.all(flags[31, dist] == 2) and np.all(m[31, dist] == 0.0) and np.all(grad[31, dist] == 0.0)
    assert np.array_equal(flags[31], host_answers(E, ALL46, x[31:32])[2][0])
    keep = np.arange(65) != 31
    for a, b in zip(clean, (m, grad, flags)):
        assert a[keep].tobytes() == b[keep].tobytes()


# ---- meaning ------------------------------------------------------------------------------------------------------------------
def sketch(E):
    if "sketch" not in _HOST:
        s = R.system("sketch150")
        _HOST["sketch"] = (E.System(s["recs"], s["n_vars"]), s)
    return _HOST["sketch"]


def reference_dimensions():
    """Three reference dimensions on sketch150: a distance and an angle that no constraint fixes, and a point-line distance."""
    P = lambda i: (2 * i, 2 * i + 1)
    return O.stack([O.distance(P(10), P(100), 0.0), O.arc_angle(P(50), P(20), P(120), ("deg", 0.0)), O.point_line_distance(P(75), P(30), P(140), 0.0)])


def test_meaning_a_solved_sketch_measures_its_own_dimensions(E):
    """sketch150 solved at residual tolerance 1e-13, measured with its own parametrised constraints as records: their residual is
    m - param, so |m - param| <= final_residual_inf / weight + 1e-11 * max(1, |param|)."""
    sysobj, s = sketch(E)
    recs = s["recs"]
    assert all(int(k) in M.SUBTRACTING for k in recs["kind"])
    x, st, _ = sysobj.solve_batch(s["start"], E.Config(max_iterations=60, residual_tolerance=1e-13))
    m, flags = sysobj.measure(x, recs, want_flags=True)
    assert m.shape == (len(x), len(recs)) and not flags.any()
    bar = st["final_residual_inf"][:, None] / recs["weight"][None, :] + 1e-11 * np.maximum(1.0, np.abs(recs["param"]))[None, :]
    err = np.abs(m - recs["param"][None, :])
    print("own dimensions: largest |m - param|", err.max(), "final residuals", st["final_residual_inf"].tolist())
    R.log(f"measure, sketch150's own dimensions: largest |m - param| {err.max():.3e} | smallest bar granted {bar.min():.3e}")
    assert np.all(err <= bar)
    # any leading shape is kept: [steps, batch, n_vars] as a sweep returns it
    m3, g3 = sysobj.measure(np.stack([x, x[::-1]]), recs[:7], want_grad=True)
    assert m3.shape == (2, len(x), 7) and g3.shape == (2, len(x), 7, 8) and m3[0].tobytes() == np.ascontiguousarray(m[:, :7]).tobytes()
    assert m3[1].tobytes() == np.ascontiguousarray(m[::-1, :7]).tobytes()


def test_meaning_of_the_response_finite_differences_of_two_solves(E):
    """D[:, :, j] against (m(x(p + delta e_j)) - m(x(p))) / delta from two solve_batch_params calls, delta = 1e-6; granted: 4 x the
    distance between the ORACLE's same finite difference and response_ref on the numpy S (the rule of
    tests/test_gpu_sensitivity.py: test_meaning_finite_differences_of_two_solves -- largest entry over the measurements, relative
    to max(1, the largest reference entry))."""
    sysobj, s = sketch(E)
    recs, pos, n = s["recs"], s["pos"], s["n_vars"]
    dims = reference_dimensions()
    delta = 1e-6
    cfg = E.Config(max_iterations=60, residual_tolerance=1e-13)
    ocfg = O.Config(max_iterations=60, residual_tolerance=1e-13)
    p0 = recs["param"][pos].copy()
    picks = [0, len(pos) // 3, len(pos) // 2, len(pos) - 1]
    rows = np.stack([p0] + [p0 + delta * (np.arange(len(pos)) == j) for j in picks])
    x0 = np.repeat(s["start"][0][None, :], len(rows), axis=0)
    x, st, _ = sysobj.solve_batch_params(x0, pos, rows, cfg)
    xo = np.stack([O.solve_batch(R.substituted(recs, pos, r), x0[:1], ocfg, linsolve=O.LINSOLVE_SPARSE)[1][0] for r in rows])
    S, status = sysobj.param_sensitivity(x[:1], pos, rows[:1], lam=s["lam"])
    assert not status.any()
    D = sysobj.measure_response(x[:1], dims, S)[0]
    m_dev = sysobj.measure(x, dims)
    Sref, _ = R.reference(recs, n, xo[0], pos, rows[0], s["lam"])
    Dref, _ = M.response_ref(dims, host_answers(E, dims, xo[:1])[1][0], Sref)
    m_orc = np.asarray([[M.measure_ref(d, xo[k])[0] for d in dims] for k in range(len(rows))])
    for k, j in enumerate(picks):
        fd_dev, fd_orc = (m_dev[k + 1] - m_dev[0]) / delta, (m_orc[k + 1] - m_orc[0]) / delta
        scale = max(1.0, np.abs(Dref[:, j]).max())
        granted = 4.0 * np.abs(fd_orc - Dref[:, j]).max() / scale
        err = np.abs(fd_dev - D[:, j]).max() / scale
        print("meaning of the response", j, "oracle's finite difference to the numpy D", granted / 4.0, "device", err)
        R.log(f"measure response, sketch150 parameter {j}: oracle's finite difference to response_ref on the numpy S {granted / 4.0:.3e}; "
              f"device's to its D {err:.3e} (granted {granted:.3e})")
        assert err <= granted, (j, err, granted)


# ---- response and stack-up ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_param", [1, 5, 70])
@pytest.mark.parametrize("n_meas", [1, 300])
@pytest.mark.parametrize("batch", [1, 65])
def test_response_and_stackup(E, n_param, n_meas, batch):
    s = system16(E)
    recs = LIST300[:n_meas]
    rng = np.random.default_rng(1000 * n_param + n_meas + batch)
    x = X[:batch]
    S = rng.uniform(-2.0, 2.0, (batch, n_param, N16))
    tol = rng.uniform(0.0, 0.1, n_param)
    D, worst, rss = s.measure_response(x, recs, S, tol=tol)
    assert D.shape == (batch, n_meas, n_param) and worst.shape == rss.shape == (batch, n_meas)
    assert s.measure_response(x, recs, S).tobytes() == D.tobytes()
    _, hg, _ = host16(E)
    for b in sorted({0, batch // 2, batch - 1}):
        Dref, mag = M.response_ref(recs, hg[b, 46:46 + n_meas], S[b])
        assert np.all(np.abs(D[b] - Dref) <= 1e-10 * mag), (b, np.abs(D[b] - Dref).max())
        wref, qref = M.worst_ref(D[b], tol)
        assert worst[b].tobytes() == wref.tobytes(), b
        assert np.all(np.abs(rss[b] - qref) <= 2.0 * np.spacing(qref)), b
    if batch > 1:
        # a system whose sensitivities failed (S_b all NaN): NaN there, the neighbours keep their bits
        bad = S.copy()
        bad[3] = np.nan
        D2, worst2, rss2 = s.measure_response(x, recs, bad, tol=tol)
        assert np.isnan(D2[3]).all() and np.isnan(worst2[3]).all() and np.isnan(rss2[3]).all()
        keep = np.arange(batch) != 3
        assert D2[keep].tobytes() == D[keep].tobytes() and worst2[keep].tobytes() == worst[keep].tobytes() and rss2[keep].tobytes() == rss[keep].tobytes()
        # ... and a system alone gives the bits it has in the batch
        one = s.measure_response(x[7:8], recs, S[7:8], tol=tol)
        assert all(a[0].tobytes() == b[7].tobytes() for a, b in zip(one, (D, worst, rss)))


def test_response_on_the_devices_own_sensitivities(E):
    """D against response_ref on the S that param_sensitivity computed on the device (sketch150, every driven dimension: S has
    entries from 1e-9 to 1) and the host function's gradients, at 1e-10 * the sum of the |terms|; the stack-up on that D."""
    sysobj, s = sketch(E)
    recs = np.concatenate([reference_dimensions(), s["recs"][s["pos"][:40]]])
    x = s["x"]
    S, status = sysobj.param_sensitivity(x, s["pos"], s["params"], lam=s["lam"])
    assert not status.any()
    tol = np.random.default_rng(12).uniform(0.0, 0.05, len(s["pos"]))
    D, worst, rss = sysobj.measure_response(x, recs, S, tol=tol)
    grads = host_answers(E, recs, x)[1]
    for b in range(len(x)):
        Dref, mag = M.response_ref(recs, grads[b], S[b])
        assert np.all(np.abs(D[b] - Dref) <= 1e-10 * mag), (b, np.abs(D[b] - Dref).max())
        wref, qref = M.worst_ref(D[b], tol)
        assert worst[b].tobytes() == wref.tobytes() and np.all(np.abs(rss[b] - qref) <= 2.0 * np.spacing(qref)), b


# ---- vjp ----------------------------------------------------------------------------------------------------------------------
def test_vjp(E):
    s = system16(E)
    rng = np.random.default_rng(9)
    _, hg, _ = host16(E)
    for recs, cols, batch in ((ALL46, slice(0, 46), 65), (LIST300, slice(46, 346), 3)):
        gm = rng.uniform(-1.0, 1.0, (batch, len(recs)))
        gx = s.measure_vjp(X[:batch], recs, gm)
        assert gx.shape == (batch, N16) and s.measure_vjp(X[:batch], recs, gm).tobytes() == gx.tobytes()
        for b in sorted({0, batch // 2, batch - 1}):
            want, mag = M.vjp_ref(recs, hg[b, cols], gm[b], N16)
            assert np.all(np.abs(gx[b] - want) <= 1e-10 * mag), (b, np.abs(gx[b] - want).max())
        assert s.measure_vjp(X[1:2], recs, gm[1:2])[0].tobytes() == gx[1].tobytes()
    # one variable named by 300 records (and four that none names: +0.0, sign bit clear, whatever grad_m is)
    hub = O.stack([O._mk(O.DISTANCE, [0, 1, 2 + 2 * (i % 5), 3 + 2 * (i % 5)]) for i in range(300)])
    gm = -rng.uniform(0.5, 1.0, (2, 300))
    gx = s.measure_vjp(X[:2], hub, gm)
    want, mag = M.vjp_ref(hub, host_answers(E, hub, X[:1])[1][0], gm[0], N16)
    assert np.all(np.abs(gx[0] - want) <= 1e-10 * mag) and mag[0] > 10.0
    assert np.all(gx[:, 12:] == 0.0) and not np.any(np.signbit(gx[:, 12:]))
    assert s.measure_vjp(X[:2], hub, gm).tobytes() == gx.tobytes()


# ---- torch --------------------------------------------------------------------------------------------------------------------
def test_torch_measure_and_its_backward(E):
    import torch

    from ezpz_amd import torch_ops

    s = system16(E)
    x = torch.tensor(X[:65], device="cuda", requires_grad=True)
    m, flags = torch_ops.measure(s, x, ALL46, return_flags=True)
    hm, hf = s.measure(X[:65], ALL46, want_flags=True)
    assert m.detach().cpu().numpy().tobytes() == hm.tobytes() and flags.cpu().numpy().tobytes() == hf.tobytes()
    gm = np.random.default_rng(3).uniform(-1.0, 1.0, hm.shape)
    m.backward(torch.tensor(gm, device="cuda"))
    assert x.grad.cpu().numpy().tobytes() == s.measure_vjp(X[:65], ALL46, gm).tobytes()


def test_torch_measure_of_solve_params_fills_params_grad(E):
    """params.grad[b, j] = sum_i D[b, i, j] with D from measure_response on the device's S at the forward's answer, at 1e-10 * the sum
    of the |terms|."""
    import torch

    from ezpz_amd import torch_ops

    sysobj, s = sketch(E)
    dims = reference_dimensions()
    x0, p = torch.tensor(s["start"], device="cuda"), torch.tensor(s["params"], device="cuda", requires_grad=True)
    xs = torch_ops.solve_params(sysobj, x0, s["pos"], p, lam=s["lam"])
    torch_ops.measure(sysobj, xs, dims).sum().backward()
    got = p.grad.cpu().numpy()
    xf = xs.detach().cpu().numpy()
    S, status = sysobj.param_sensitivity(xf, s["pos"], s["params"], lam=s["lam"])
    assert not status.any()
    D = sysobj.measure_response(xf, dims, S)
    grads = sysobj.measure(xf, dims, want_grad=True)[1]
    for b in range(len(xf)):
        mag = M.response_ref(dims, grads[b], S[b])[1].sum(axis=0)
        err = np.abs(got[b] - D[b].sum(axis=0))
        print("measure(solve_params) backward", b, "largest error / bar", (err[mag > 0] / (1e-10 * mag[mag > 0])).max())
        assert np.all(err <= 1e-10 * mag), (b, err.max())


# ---- entries ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(E):
    s = system16(E)
    L = E.lib()
    recs = ALL46[:5].copy()
    x = np.ascontiguousarray(X[:2])
    S = np.ones((2, 3, N16))
    tol = np.full(3, 0.1)
    gm = np.ones((2, 5))
    outs = dict(m=np.full((2, 5), 77.0), fl=np.full((2, 5), 77, np.uint8), g=np.full((2, 5, 8), 77.0), D=np.full((2, 5, 3), 77.0),
                w=np.full((2, 5), 77.0), q=np.full((2, 5), 77.0), gx=np.full((2, N16), 77.0))
    p = lambda a: a.ctypes.data if a is not None else None
    untouched = lambda: all(np.all(a == 77) for a in outs.values())

    def measure(recs_=recs, n=5, x_=x, batch=2, m_=outs["m"]):
        return L.ezpz_system_measure(s._h, p(recs_), n, p(x_), batch, p(m_), p(outs["fl"]), p(outs["g"]))

    def response(recs_=recs, n=5, x_=x, S_=S, n_param=3, batch=2, tol_=tol, D_=outs["D"], w_=outs["w"], q_=outs["q"]):
        return L.ezpz_system_measure_response(s._h, p(recs_), n, p(x_), p(S_), n_param, batch, p(tol_), p(D_), p(w_), p(q_))

    def vjp(recs_=recs, n=5, x_=x, gm_=gm, batch=2, gx_=outs["gx"]):
        return L.ezpz_system_measure_vjp(s._h, p(recs_), n, p(x_), p(gm_), batch, p(gx_))

    parallel = recs.copy()
    parallel[2] = O._mk(O.LINES_AT_ANGLE, list(range(8)), 0.0, tag=O.ANGLE_PARALLEL)
    unmeasurable = recs.copy()
    unmeasurable[4] = O._mk(O.MIDPOINT, list(range(6)))
    far = recs.copy()
    far["ids"][1][0] = N16
    for bad in (parallel, unmeasurable, far, None):
        assert measure(recs_=bad) == response(recs_=bad) == vjp(recs_=bad) == ERR_INVALID_ARGUMENT and untouched()
    assert measure(x_=None) == measure(m_=None) == ERR_INVALID_ARGUMENT and untouched()
    assert response(x_=None) == response(S_=None) == response(D_=None) == ERR_INVALID_ARGUMENT and untouched()
    assert response(tol_=None) == response(w_=None) == response(q_=None) == ERR_INVALID_ARGUMENT and untouched()
    for t in (-0.1, float("nan"), float("inf")):
        assert response(tol_=np.asarray([0.1, t, 0.1])) == ERR_INVALID_ARGUMENT and untouched()
    assert vjp(x_=None) == vjp(gm_=None) == vjp(gx_=None) == ERR_INVALID_ARGUMENT and untouched()
    # nothing to do: EZPZ_OK, nothing written
    assert measure(batch=0) == measure(n=0) == measure(n=0, recs_=None) == 0 and untouched()
    assert response(batch=0) == response(n=0) == response(n_param=0) == 0 and vjp(batch=0) == vjp(n=0) == 0 and untouched()
    # the device entries check the same before they enqueue anything (null pointers stand for device memory here: never read)
    assert L.ezpz_system_measure_device(s._h, p(recs), 5, None, 2, None, None, None, None) == ERR_INVALID_ARGUMENT
    assert L.ezpz_system_measure_device(s._h, p(far), 5, None, 0, None, None, None, None) == ERR_INVALID_ARGUMENT
    assert L.ezpz_system_measure_response_device(s._h, p(recs), 5, None, None, 3, 2, None, None, None, None, None) == ERR_INVALID_ARGUMENT
    assert L.ezpz_system_measure_vjp_device(s._h, p(recs), 5, None, None, 2, None, None) == ERR_INVALID_ARGUMENT
    assert L.ezpz_system_measure_device(s._h, p(recs), 5, None, 0, None, None, None, None) == 0
    assert measure() == response() == vjp() == 0 and not untouched()


def test_device_forms_on_side_streams(E):
    """The _device forms on a stream of the caller's give the host forms' bits; a long call on one stream with a short one with
    another list right behind it on a second stream gives the bits of the calls made alone; a repeated list uploads nothing."""
    import torch

    s = system16(E)
    xl, xs_ = np.ascontiguousarray(X), np.ascontiguousarray(X[:5])
    short = ALL46[::-1].copy()
    want_long = s.measure(xl, LIST300, want_grad=True, want_flags=True)
    want_short = s.measure(xs_, short, want_grad=True, want_flags=True)
    rng = np.random.default_rng(4)
    S, tol, gm = rng.uniform(-1.0, 1.0, (5, 4, N16)), rng.uniform(0.0, 0.1, 4), rng.uniform(-1.0, 1.0, (5, 46))
    want_resp, want_vjp = s.measure_response(xs_, short, S, tol=tol), s.measure_vjp(xs_, short, gm)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    dev = lambda v: torch.tensor(v, device="cuda")
    xld, xsd, Sd, told, gmd = dev(xl), dev(xs_), dev(S), dev(tol), dev(gm)
    out = lambda shape, dtype=torch.float64: torch.full(shape, 9, dtype=dtype, device="cuda")
    ml, fl, gl = out((1025, 300)), out((1025, 300), torch.uint8), out((1025, 300, 8))
    ms, fs, gs = out((5, 46)), out((5, 46), torch.uint8), out((5, 46, 8))
    D, w, q, gx = out((5, 46, 4)), out((5, 46)), out((5, 46)), out((5, N16))
    torch.cuda.synchronize()

    def both():
        s.measure_device(xld.data_ptr(), LIST300, 1025, ml.data_ptr(), fl.data_ptr(), gl.data_ptr(), stream=a.cuda_stream)
        s.measure_device(xsd.data_ptr(), short, 5, ms.data_ptr(), fs.data_ptr(), gs.data_ptr(), stream=b.cuda_stream)

    _, stamps = _trace(E, both)
    assert stamps.count(UPLOADED) == 2 and stamps.count(LAUNCHED) == 2, stamps
    torch.cuda.synchronize()
    for got, want in zip((ml, gl, fl, ms, gs, fs), want_long + want_short):
        assert got.cpu().numpy().tobytes() == want.tobytes()

    def rest():
        s.measure_response_device(xsd.data_ptr(), short, Sd.data_ptr(), 4, 5, D.data_ptr(), told.data_ptr(), w.data_ptr(), q.data_ptr(),
                                  stream=b.cuda_stream)
        s.measure_vjp_device(xsd.data_ptr(), short, gmd.data_ptr(), 5, gx.data_ptr(), stream=a.cuda_stream)
        s.measure_device(xsd.data_ptr(), short, 5, ms.data_ptr(), stream=b.cuda_stream)

    rest()  # (the workspace and the vjp's table appear on first use)
    _, stamps = _trace(E, rest)
    assert UPLOADED not in stamps and stamps.count(LAUNCHED) == 3, stamps  # the list repeated: calls only enqueue
    torch.cuda.synchronize()
    for got, want in zip((D, w, q, gx, ms), want_resp + (want_vjp, want_short[0])):
        assert got.cpu().numpy().tobytes() == want.tobytes()
