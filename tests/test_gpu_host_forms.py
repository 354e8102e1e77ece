"""GPU tests (-m gpu) of the host forms' staging (csrc/host_stage.hpp): every host form that stages its arrays through the one list
-- measure, measure_response, measure_vjp, redundancy, param_sensitivity, seek_targets, cluster_branches, solve_branches,
mc_moments, sweep_guarded, tolerance_mc -- called small, larger, small again on one system gives the same bytes the first and the
third time, and the bytes of its device form on the same inputs (the comparison of tests/test_gpu_device_entries.py: bytes); with
every optional output absent the others keep their bytes; a chunked form gives the same bytes whatever the chunk; a staged x keeps
the 16-byte alignment the measure entry's ROW placement asks for; a failing request leaves the outputs as they were.

The systems are the smallest the entries' own tests use: the connected triangle of tests/test_gpu_seek.py (6 variables, the three
side lengths driven), the rectangle and the block system of tests/redundancy_ref.py, and 600 Fixed variables for the ROW window."""
import numpy as np
import pytest

import redundancy_ref as RR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MEASURE_PLACED_ROW = 52
PATTERN = 0xA5
_CACHE = {}

A, B, Cc = (0, 1), (2, 3), (4, 5)
TRI = O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(3, 0.0), O.distance(A, B, 5.0), O.distance(B, Cc, 3.0), O.distance(Cc, A, 4.0)])
TRI_X0 = np.array([0.0, 0.0, 5.0, 0.0, 3.2, 2.4])  # the 3-4-5 triangle's solution
POS = [3, 4, 5]
P0 = np.array([5.0, 3.0, 4.0])
RECS = O.stack([O.distance(A, B, 0.0), O.distance(B, Cc, 0.0), O.distance(Cc, A, 0.0)])
SIZES = (3, 70, 3)  # small, larger, small again


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


def triangle(E):
    if "tri" not in _CACHE:
        _CACHE["tri"] = E.System(TRI, 6)
    return _CACHE["tri"]


def rows(batch, width, key, spread=0.01):
    return np.random.default_rng(1000 * key + batch).uniform(-spread, spread, (batch, width))


def tri_inputs(E, batch):
    """(x, params): `batch` solved triangles, each with side lengths of its own."""
    if ("tri_in", batch) not in _CACHE:
        params = P0[None, :] + rows(batch, 3, 1, 0.05)
        x, st, _ = triangle(E).solve_batch_params(np.tile(TRI_X0, (batch, 1)), POS, params)
        assert np.all(st["n_unsatisfied"] == 0)
        _CACHE[("tri_in", batch)] = (np.ascontiguousarray(x), params)
    return _CACHE[("tri_in", batch)]


def as_bytes(outputs):
    return [np.ascontiguousarray(o).tobytes() for o in outputs]


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def out_like(a):
    """A device buffer of a's bytes, every byte the pattern."""
    import torch

    return torch.full((max(np.asarray(a).nbytes, 1),), PATTERN, dtype=torch.uint8, device="cuda")


def back(t, like):
    import torch

    torch.cuda.synchronize()
    like = np.asarray(like)
    return np.frombuffer(t.cpu().numpy().tobytes()[: like.nbytes], dtype=like.dtype).reshape(like.shape)


def device_outputs(host_outputs, enqueue):
    """The device form's outputs for the shapes of the host form's: enqueue(pointers of the outputs, in order)."""
    outs = [out_like(h) for h in host_outputs]
    enqueue(*(o.data_ptr() for o in outs))
    return [back(o, h) for o, h in zip(outs, host_outputs)]


# ---- every entry: (host form, device form) of `batch` systems; both return the same list of arrays --------------------------------
def measure_pair(E, batch):
    s, (x, _) = triangle(E), tri_inputs(E, batch)
    host = lambda: list(s.measure(x, RECS, want_grad=True, want_flags=True))  # m, grad, flags
    xd = dev(x)
    device = lambda h: device_outputs(h, lambda m, grad, flags: s.measure_device(xd.data_ptr(), RECS, batch, m, flags, grad))
    return host, device


def sens_of(E, batch):
    s, (x, params) = triangle(E), tri_inputs(E, batch)
    return s.param_sensitivity(x, POS, params)[0]


def response_pair(E, batch):
    s, (x, _) = triangle(E), tri_inputs(E, batch)
    S, tol = sens_of(E, batch), np.array([0.1, 0.2, 0.05])
    host = lambda: list(s.measure_response(x, RECS, S, tol))  # D, worst, rss
    xd, Sd, td = dev(x), dev(S), dev(tol)
    device = lambda h: device_outputs(h, lambda D, worst, rss: s.measure_response_device(xd.data_ptr(), RECS, Sd.data_ptr(), 3, batch, D,
                                                                                         td.data_ptr(), worst, rss))
    return host, device


def vjp_pair(E, batch):
    s, (x, _) = triangle(E), tri_inputs(E, batch)
    gm = rows(batch, len(RECS), 2, 1.0)
    host = lambda: [s.measure_vjp(x, RECS, gm)]
    xd, gd = dev(x), dev(gm)
    device = lambda h: device_outputs(h, lambda gx: s.measure_vjp_device(xd.data_ptr(), RECS, gd.data_ptr(), batch, gx))
    return host, device


def redundancy_case(E, name):
    if ("red", name) not in _CACHE:
        c = RR.case(name)
        _CACHE[("red", name)] = (c, E.System(c["recs"], c["n_vars"]))
    return _CACHE[("red", name)]


def redundancy_pair(E, batch, name="blocks"):
    c, s = redundancy_case(E, name)
    x = np.tile(np.atleast_2d(c["x"]), (batch, 1))[:batch] + rows(batch, c["n_vars"], 3, 1e-3)
    focus = list(c["focus"] or [0])
    keys = ("con_status", "rank", "row_status", "group")

    def host():
        r = s.redundancy(x, focus=focus, want_rows=True)
        return [r[k] for k in keys]

    xd = dev(x)
    device = lambda h: device_outputs(h, lambda con, rank, rows_, group: s.redundancy_device(xd.data_ptr(), batch, con, rows_, rank, focus, group))
    return host, device


def sensitivity_pair(E, batch):
    s, (x, params) = triangle(E), tri_inputs(E, batch)
    host = lambda: list(s.param_sensitivity(x, POS, params, want_degenerate=True))  # S, status, degenerate counts
    xd, pd = dev(x), dev(params)
    device = lambda h: device_outputs(h, lambda S, st, deg: s.param_sensitivity_device(xd.data_ptr(), POS, pd.data_ptr(), batch, S, st,
                                                                                       degenerate_ptr=deg))
    return host, device


def seek_inputs(E, batch):
    x, params = tri_inputs(E, batch)
    targets = triangle(E).measure(x, RECS) + rows(batch, len(RECS), 4, 0.02)
    return x, params, targets


def seek_pair(E, batch, chunk=0):
    s, (x, params, targets) = triangle(E), seek_inputs(E, batch)
    cfg = E.SeekConfig(max_iterations=6, chunk=chunk)

    def host():
        r = s.seek_targets(x, POS, params, RECS, targets, cfg, want_trace=True)
        return [r.params, r.x, r.m, r.info, r.cost_trace]

    xd, pd, td = dev(x), dev(params), dev(targets)
    device = lambda h: device_outputs(h, lambda p, xo, m, info, trace: s.seek_targets_device(xd.data_ptr(), POS, pd.data_ptr(), RECS, td.data_ptr(),
                                                                                            batch, p, xo, m, info, trace, config=cfg))
    return host, device


def branch_dists(E):
    return [E.McDist.fixed(), E.McDist.fixed(), E.McDist.uniform(-0.5, 0.5), E.McDist.fixed(), E.McDist.uniform(-4.0, 4.0), E.McDist.uniform(-6.0, 6.0)]


def branches_pair(E, batch):
    s, (x, _) = triangle(E), tri_inputs(E, batch)
    samples, branch = 40, E.BranchConfig(max_branches=4)

    def host():
        r = s.solve_branches(x, branch_dists(E), samples, seed=5, branch=branch, keep=True)
        return [r.info, r.branches, r.x, r.labels]

    xd = dev(x)
    device = lambda h: device_outputs(h, lambda info, br, xb, lab: s.solve_branches_device(xd.data_ptr(), branch_dists(E), batch, samples, info, br, xb,
                                                                                         lab, seed=5, branch=branch))
    return host, device


def cluster_pair(E, batch):
    samples, n = 50, 4
    x = np.round(rows(batch * samples, n, 5, 3.0)).reshape(batch, samples, n)  # (a handful of distinct rows: several branches)
    ok = (np.arange(batch * samples).reshape(batch, samples) % 7 != 3).astype(np.uint8)
    branch = E.BranchConfig(max_branches=4)

    def host():
        r = E.cluster_branches(x, ok=ok, branch=branch, keep=True)
        return [r.info, r.branches, r.x, r.labels]

    xd, okd, bc = dev(x), dev(ok), branch._c()

    def device(h):
        import ctypes as C

        def enqueue(info, br, xb, lab):
            rc = E.lib().ezpz_branch_cluster_device(xd.data_ptr(), okd.data_ptr(), None, batch, samples, n, C.byref(bc), info, br, xb, lab, None)
            assert rc == 0, rc

        return device_outputs(h, enqueue)

    return host, device


def moments_inputs(samples, with_flags=True):
    params, m = rows(samples, 2, 6, 1.0), rows(samples, 3, 7, 1.0)
    flags = (np.arange(samples * 3).reshape(samples, 3) % 11 == 0).astype(np.uint8) if with_flags else None
    ok = (np.arange(samples) % 13 != 5).astype(np.uint8) if with_flags else None
    return params, m, flags, ok, np.array([0.1, -0.2]), np.array([0.0, 0.3, -0.1])


def moments_pair(E, samples, chunk=256):
    from ezpz_amd._lib import MC_MOMENTS_INFO_DTYPE

    params, m, flags, ok, np_, nm = moments_inputs(samples)

    def host():
        moments, n_complete = E.mc_moments(params, m, flags, ok, np_, nm, chunk=chunk)
        return [np.asarray(moments), np.array([(samples, n_complete)], dtype=MC_MOMENTS_INFO_DTYPE)]

    d = [dev(a) for a in (params, m, flags, ok, np_, nm)]

    def device(h):
        def enqueue(moments, info):
            rc = E.lib().ezpz_mc_moments_device(*(t.data_ptr() for t in d), samples, 2, 3, chunk, moments, info, None)
            assert rc == 0, rc

        return device_outputs(h, enqueue)

    return host, device


def guarded_inputs(E, batch, steps=3):
    x, params = tri_inputs(E, batch)
    walk = np.stack([params + (k + 1) * np.array([0.05, -0.03, 0.04]) for k in range(steps)])
    walk[-1, 0] = [50.0, 1.0, 1.0]  # (no triangle: the sweep halves, gives up and holds its last answer; its log has entries)
    return x, params, np.ascontiguousarray(walk)


def guarded_system(E):
    """The triangle on a route that has a guarded kernel: the host form is then the one launch, staged."""
    if "guarded" not in _CACHE:
        _CACHE["guarded"] = E.System(TRI, 6, team_size=E.TEAM_AUTO_LISTS)
        assert _CACHE["guarded"].sweep_guarded_plan(POS)["in_kernel"] == 1
    return _CACHE["guarded"]


def guarded_pair(E, batch):
    s, (x, params, walk) = guarded_system(E), guarded_inputs(E, batch)
    guard = E.GuardConfig(max_attempts=5)

    def host():
        xo, st, mask, gs, reached = s.sweep_guarded(x, POS, params, walk, guard=guard, want_mask=True)
        return [xo, st, mask, gs, reached]

    xd, pd, wd = dev(x), dev(params), dev(walk)
    device = lambda h: device_outputs(h, lambda xo, st, mask, gs, reached: s.sweep_guarded_device(xd.data_ptr(), POS, pd.data_ptr(), wd.data_ptr(), len(walk),
                                                                                                batch, xo, st, gs, reached, mask_ptr=mask, guard=guard))
    return host, device


def mc_dists3(E):
    return [E.McDist.normal(0.01), E.McDist.uniform(-0.02, 0.02), E.McDist.normal(0.01, 3.0)]


def tolerance_pair(E, n_meas):
    """300 samples (rounds of 256 and 44) measured by n_meas records: the outputs staged are per record."""
    s, samples = triangle(E), 300
    recs = O.stack([RECS[i % len(RECS)] for i in range(n_meas)])
    kw = dict(seed=9, hist=(np.full(n_meas, -1.0), np.full(n_meas, 9.0), 8), chunk=256)

    def host():
        r = s.tolerance_mc(TRI_X0, POS, mc_dists3(E), recs, samples, **kw)
        return [r.stats, r.totals, r.hist]

    x0 = dev(TRI_X0)
    device = lambda h: device_outputs(h, lambda stats, totals, hist: s.tolerance_mc_device(x0.data_ptr(), POS, mc_dists3(E), recs, samples, stats, totals,
                                                                                         hist, **kw))
    return host, device


PAIRS = {"measure": measure_pair, "measure_response": response_pair, "measure_vjp": vjp_pair, "redundancy": redundancy_pair,
         "param_sensitivity": sensitivity_pair, "seek_targets": seek_pair, "solve_branches": branches_pair, "cluster_branches": cluster_pair,
         "sweep_guarded": guarded_pair}
# (mc_moments' sizes are samples -- its inputs are what grows, up to a round of 256 -- and tolerance_mc's are records)
SAMPLED = {"mc_moments": (moments_pair, (100, 700, 100)), "tolerance_mc": (tolerance_pair, SIZES)}


# ---- A. growth ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sorted(PAIRS) + sorted(SAMPLED))
def test_small_larger_small_again(E, entry):
    """The staging buffer grows for the second call and is larger than it need be for the third: the first and the third call give
    the same bytes, and each of the three the bytes of the device form."""
    pair, sizes = (PAIRS[entry], SIZES) if entry in PAIRS else SAMPLED[entry]
    got = []
    for size in sizes:
        host, device = pair(E, size)
        h = host()
        got.append(as_bytes(h))
        d = device(h)
        assert len(d) == len(h)
        for k, (a, b) in enumerate(zip(as_bytes(d), got[-1])):
            assert a == b, (entry, size, "output %d: the device form's bytes differ" % k)
    assert got[0] == got[2], entry
    if entry != "mc_moments":  # (its outputs are as long whatever the samples)
        assert [len(b) for b in got[1]] != [len(b) for b in got[0]], entry


# ---- B. optional outputs ----------------------------------------------------------------------------------------------------------------
def test_optional_outputs_absent_and_present(E):
    """Every optional output absent, then all present: what both calls return has the same bytes."""
    s, batch = triangle(E), 5
    x, params = tri_inputs(E, batch)
    S = sens_of(E, batch)
    sg = guarded_system(E)
    same = lambda a, b, what: np.testing.assert_array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8), err_msg=what)
    # measure: flags / grad
    same(s.measure(x, RECS), s.measure(x, RECS, want_grad=True, want_flags=True)[0], "measure")
    # measure_response: tol with worst / rss
    same(s.measure_response(x, RECS, S), s.measure_response(x, RECS, S, np.array([0.1, 0.2, 0.05]))[0], "measure_response")
    # param_sensitivity: params, the degenerate counts
    bare, full = s.param_sensitivity(x, POS, params), s.param_sensitivity(x, POS, params, want_degenerate=True)
    same(bare[0], full[0], "S"), same(bare[1], full[1], "status")
    # redundancy: row_status, focus empty (and rank, which the Python layer always asks for: through the C entry)
    c, r = redundancy_case(E, "blocks")
    xr = np.ascontiguousarray(np.tile(np.atleast_2d(c["x"]), (batch, 1))[:batch], dtype=np.float64)
    bare, full = r.redundancy(xr), r.redundancy(xr, focus=list(c["focus"] or [0]), want_rows=True)
    same(bare["con_status"], full["con_status"], "con_status"), same(bare["rank"], full["rank"], "rank")
    con = np.full_like(full["con_status"], 9)
    assert E.lib().ezpz_system_redundancy(r._h, xr.ctypes.data, batch, None, con.ctypes.data, None, None, None, 0, None) == 0
    same(con, full["con_status"], "con_status without rank")
    # seek_targets: cost_trace
    _, _, targets = seek_inputs(E, batch)
    cfg = E.SeekConfig(max_iterations=6)
    bare, full = s.seek_targets(x, POS, params, RECS, targets, cfg), s.seek_targets(x, POS, params, RECS, targets, cfg, want_trace=True)
    assert bare.cost_trace is None and full.cost_trace is not None
    for f in ("params", "x", "m", "info"):
        same(getattr(bare, f), getattr(full, f), "seek " + f)
    # solve_branches and cluster_branches: keep_label (and ok)
    bare, full = (s.solve_branches(x, branch_dists(E), 40, seed=5, branch=E.BranchConfig(max_branches=4), keep=k) for k in (False, True))
    assert bare.labels is None and full.labels is not None
    for f in ("info", "branches", "x"):
        same(getattr(bare, f), getattr(full, f), "solve_branches " + f)
    xc = np.round(rows(2 * 50, 4, 5, 3.0)).reshape(2, 50, 4)
    bare, full = E.cluster_branches(xc), E.cluster_branches(xc, ok=np.ones((2, 50), np.uint8), keep=True)
    for f in ("info", "branches", "x"):
        same(getattr(bare, f), getattr(full, f), "cluster_branches " + f)
    # mc_moments: flags / ok (absent: clear / set)
    p, m, _, _, np_, nm = moments_inputs(300, with_flags=False)
    bare, full = E.mc_moments(p, m, None, None, np_, nm), E.mc_moments(p, m, np.zeros((300, 3), np.uint8), np.ones(300, np.uint8), np_, nm)
    same(bare[0], full[0], "moments")
    assert bare[1] == full[1] == 300
    # sweep_guarded: unsat_mask, the warning log
    xg, pg, walk = guarded_inputs(E, batch)
    guard = E.GuardConfig(max_attempts=5)
    log = np.full(walk.shape[:2] + (4,), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    bare, full = sg.sweep_guarded(xg, POS, pg, walk, guard=guard), sg.sweep_guarded(xg, POS, pg, walk, guard=guard, want_mask=True, warn_log=log)
    assert bare[2] is None and full[2] is not None
    for k in (0, 1, 3, 4):
        same(bare[k], full[k], "sweep_guarded output %d" % k)
    # the log: a row's first min(n_warnings, 4) entries are written, the others are the caller's still
    written = np.minimum(full[1]["n_warnings"], 4)
    for row, n in zip(log.reshape(-1, 4), written.reshape(-1)):
        assert np.all(row[n:] == 0xA5A5A5A5A5A5A5A5) and np.all(row[:n] != 0xA5A5A5A5A5A5A5A5), (row, n)
    # tolerance_mc: the histogram, and a kind's outputs (the contributors')
    kw = dict(seed=9, chunk=256)
    bare = s.tolerance_mc(TRI_X0, POS, mc_dists3(E), RECS, 300, **kw)
    full = s.tolerance_mc(TRI_X0, POS, mc_dists3(E), RECS, 300, hist=(np.full(len(RECS), -1.0), np.full(len(RECS), 9.0), 8), contributors=True, **kw)
    assert bare.hist is None and full.hist is not None and full.moments is not None
    same(bare.stats, full.stats, "stats"), same(bare.totals, full.totals, "totals")


# ---- C. chunked forms -------------------------------------------------------------------------------------------------------------------
def test_chunks_that_do_not_divide_the_batch(E):
    """seek_targets over 150 systems in chunks of 64 (64 + 64 + 22) and mc_moments over 700 samples in rounds of 256 (256 + 256 + 188)
    against one chunk that covers everything.  seek: bytes, as tests/test_gpu_seek.py holds for any chunk; the moments: the info and
    every sum to 1e-12 relative to the sum of the magnitudes (700 terms below 2 in another order: 700 * 2^-53 * 4 < 1e-12)."""
    whole, parts = seek_pair(E, 150, chunk=192)[0](), seek_pair(E, 150, chunk=64)[0]()
    assert as_bytes(whole) == as_bytes(parts)
    (mw, iw), (mp, ip) = moments_pair(E, 700, chunk=1024)[0](), moments_pair(E, 700, chunk=256)[0]()
    assert iw.tobytes() == ip.tobytes()
    params, m = moments_inputs(700)[:2]
    scale = 700 * max(np.abs(params).max(), np.abs(m).max(), 1.0) ** 2
    assert np.all(np.abs(mw - mp) <= 1e-12 * scale), np.abs(mw - mp).max()


# ---- D. the staged x of ezpz_system_measure keeps ROW's alignment ----------------------------------------------------------------------------
def test_measure_of_a_row_sized_system_is_placed_row(E):
    """600 variables lie inside the ROW window (512 .. 1536, csrc/policy.hpp), and ROW needs x 16-byte aligned: a staged x that lost
    its alignment would quietly take DIRECT."""
    n = 600
    s = E.System(O.stack([O.fixed(v, float(v)) for v in range(n)]), n)
    recs = O.stack([O.distance((2 * k, 2 * k + 1), (2 * k + 2, 2 * k + 3), 0.0) for k in range(7)])
    trace = np.zeros(4096, dtype=np.uint64)
    for batch in (3, 40, 3):  # (x moves as little as anything in front of it in the list: it is first; the outputs behind it grow)
        x = rows(batch, n, 8, 5.0)
        E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
        try:
            m, grad, flags = s.measure(x, recs, want_grad=True, want_flags=True)
        finally:
            k = E.lib().ezpz_debug_call_trace(None, 0)
        assert MEASURE_PLACED_ROW in [int(v) for v in trace[:k:2]], trace[:k:2]
        xd = dev(x)
        d = device_outputs([m, grad, flags], lambda mp, gp, fp: s.measure_device(xd.data_ptr(), recs, batch, mp, fp, gp))
        assert as_bytes(d) == as_bytes([m, grad, flags])


# ---- E. a failing request leaves the outputs alone -------------------------------------------------------------------------------------------
def test_failing_requests_touch_no_output(E):
    """One entry per file, through the C entries with the outputs filled beforehand: a position past the list (the driven entries), a
    record of another system's variable (measure), a non-finite target (seek), a focus past the constraints (redundancy), no compared
    variable (the branches), a shape past the moments' limit."""
    import ctypes as C

    from ezpz_amd._lib import BRANCH_DTYPE, BRANCH_INFO_DTYPE, GUARD_STEP_DTYPE, MC_MOMENTS_INFO_DTYPE, MC_STATS_DTYPE, MC_TOTALS_DTYPE, SEEK_INFO_DTYPE, STATUS_DTYPE

    s, sg, L, batch = triangle(E), guarded_system(E), E.lib(), 4
    recs_c = E.api.stack_records(RECS)
    x, params = tri_inputs(E, batch)
    _, _, targets = seek_inputs(E, batch)
    filled = lambda shape, dtype=np.float64: np.frombuffer(bytes([PATTERN]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()
    untouched = lambda *arrays: all(np.all(a.view(np.uint8) == PATTERN) for a in arrays)
    p = lambda a: a.ctypes.data
    pos, bad_pos = np.array(POS, np.uint32), np.array([3, 4, 99], np.uint32)
    bad_recs = E.api.stack_records(O.stack([O.distance(A, (6, 7), 0.0)]))
    # sensitivity.hip
    S, st, deg = filled((batch, 3, 6)), filled(batch, np.uint32), filled(batch, np.uint32)
    assert L.ezpz_system_param_sensitivity(s._h, p(x), p(bad_pos), 3, p(params), batch, C.c_double(1e-3), p(S), p(st), p(deg)) != 0
    assert untouched(S, st, deg)
    # measure.hip
    m, flags, grad = filled((batch, 1)), filled((batch, 1), np.uint8), filled((batch, 1, 8))
    assert L.ezpz_system_measure(s._h, p(bad_recs), 1, p(x), batch, p(m), p(flags), p(grad)) != 0
    assert untouched(m, flags, grad)
    # seek.hip
    bad_targets = targets.copy()
    bad_targets[2, 1] = np.inf
    po, xo, mo, info = filled((batch, 3)), filled((batch, 6)), filled((batch, len(RECS))), filled(batch, SEEK_INFO_DTYPE)
    assert L.ezpz_system_seek_targets(s._h, p(x), p(pos), 3, p(params), p(recs_c), len(RECS), p(bad_targets), batch, None, p(po), p(xo), p(mo), p(info), None) != 0
    assert untouched(po, xo, mo, info)
    # guarded_sweep.hip
    walk = np.ascontiguousarray(guarded_inputs(E, batch)[2][:2])
    xs, sts, gs, reached = filled((2, batch, 6)), filled((2, batch), STATUS_DTYPE), filled((2, batch), GUARD_STEP_DTYPE), filled((2, batch, 3))
    assert L.ezpz_system_sweep_guarded(sg._h, p(x), p(bad_pos), 3, p(params), p(walk), 2, batch, None, None, p(xs), p(sts), p(gs), p(reached), None, None, 0) != 0
    assert untouched(xs, sts, gs, reached)
    # redundancy.hip
    c, r = redundancy_case(E, "blocks")
    xr = np.ascontiguousarray(np.tile(np.atleast_2d(c["x"]), (batch, 1))[:batch], dtype=np.float64)
    n_cs = len(c["recs"])
    con, rank, group = filled((batch, n_cs), np.uint8), filled(batch, np.uint32), filled((batch, 1, n_cs), np.uint8)
    bad_focus = np.array([n_cs], np.uint32)
    assert L.ezpz_system_redundancy(r._h, p(xr), batch, None, p(con), None, p(rank), p(bad_focus), 1, p(group)) != 0
    assert untouched(con, rank, group)
    # branches.hip (both host forms)
    none_compared = np.zeros(6, np.uint8)
    binfo, br, xb = filled(batch, BRANCH_INFO_DTYPE), filled((batch, 32), BRANCH_DTYPE), filled((batch, 32, 6))
    d = E.api.mc_dists(branch_dists(E))
    assert L.ezpz_system_solve_branches(s._h, p(x), p(d), p(none_compared), batch, 40, None, None, p(binfo), p(br), p(xb), None) != 0
    xc = np.ascontiguousarray(np.tile(x[:, None, :], (1, 40, 1)))
    assert L.ezpz_branch_cluster(p(xc), None, p(none_compared), batch, 40, 6, None, p(binfo), p(br), p(xb), None) != 0
    assert untouched(binfo, br, xb)
    # mc_moments.hip
    mom, minfo = filled(10), filled(1, MC_MOMENTS_INFO_DTYPE)
    wide = np.zeros((4, 4096))
    assert L.ezpz_mc_moments(p(wide), p(wide), None, None, p(wide), p(wide), 4, 4096, 4096, 0, p(mom), p(minfo)) != 0
    assert untouched(mom, minfo)
    # tolerance_mc.hip
    stats, totals = filled(len(RECS), MC_STATS_DTYPE), filled(1, MC_TOTALS_DTYPE)
    with pytest.raises(E.NonLinearSystemError):
        s.tolerance_mc(TRI_X0, [3, 4, 99], mc_dists3(E), RECS, 100)
    d3 = E.api.mc_dists(mc_dists3(E))
    assert L.ezpz_system_tolerance_mc(s._h, p(TRI_X0), p(bad_pos), 3, p(d3), None, p(recs_c), len(RECS), None, None, None, None, 100, None, None, p(stats),
                                      p(totals), None, None, None, None, None) != 0
    assert untouched(stats, totals)
