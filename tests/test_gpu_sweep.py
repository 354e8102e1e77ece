"""Dimension sweeps (ezpz_system_sweep_params): a chain of driven solves per system in one launch.  Against the oracle run once
per (sweep, step), and bit for bit against the chain of solve_batch_params calls the sweep is defined as -- on every launch shape,
for a team's second sweep, with the workspace in global memory, through steps that fail and steps that warn -- and the entry's
errors and device form.  Bars: tests/sensitivity.py (1e-6, or the oracle's own measured sensitivity)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from oracle import textual as T
from sensitivity import assert_batch_matches_oracle
from sweep_common import (CASES, P0, P1, ROUTES, STEPS, SWEEPS, chain, chain_of_calls, driven_walk, oracle_chain, oracle_inputs,
                          shapes, substituted)

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
IN_KERNEL_ROUTES = {"interpreter", "barrier workgroup", "record walk", "sub-wavefront teams"}
# (shape, how many of its parametrised constraints are driven -- None: all of them --, EzpzSweepPlan::params_in_lds): which form
# of the driven values each case runs.  The list-walk teams stage them in LDS where that costs the CU no workgroup
# (par_lds_plan), the interpreter never does.  The partitioned workgroup keeps TWO copies that alternate by (sweep, step): all
# 192 values of its system do not fit twice and are read from global memory, 16 are staged -- so it runs both.
SHAPE_CASES = [("sub-wavefront teams", None, 1), ("partitioned workgroup", None, 0), ("partitioned workgroup", 16, 1),
               ("interpreter", None, 0), ("barrier workgroup", None, 1), ("record walk", None, 1)]
SHAPE_IDS = [name + ("" if n is None else ", %d driven" % n) for name, n, _ in SHAPE_CASES]


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


@pytest.fixture(scope="module")
def shape_of(E):
    return {name: (recs, g, team, mode) for name, recs, g, team, mode in shapes(E)}


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _same(a, b, what):
    (xa, sa, ma), (xb, sb, mb) = a, b
    assert xa.shape == xb.shape and sa.shape == sb.shape, what
    assert np.array_equal(xa, xb, equal_nan=True), what
    assert sa.tobytes() == sb.tobytes(), what
    if ma is not None or mb is not None:
        assert np.array_equal(ma, mb), what


@pytest.mark.parametrize("name", sorted(CASES))
def test_kind_by_kind_against_the_oracle_chain(E, name):
    """64 sweeps x 12 steps of every parametrised kind.  Every device step is judged against an oracle step started from the device's
    own previous answer, so that a difference within the bar at one step is not carried through the bar of the next."""
    recs, pos, params, x0 = oracle_inputs(name)
    s = E.System(recs, x0.shape[1], team_size=E.TEAM_AUTO_LISTS)
    assert s.info()["team_mode"] == 0
    x, st, mask = s.sweep_params(x0, pos, params, want_mask=True)
    assert x.shape == (STEPS, SWEEPS, x0.shape[1]) and st.shape == (STEPS, SWEEPS) and mask.shape == (STEPS, SWEEPS, len(recs))
    xo, it, conv, nun, mo, begin = oracle_chain(recs, pos, params, x0, starts=x)
    print(name, "oracle converged on", int(conv.sum()), "of", conv.size, "| largest relative coordinate error",
          float(np.nanmax(np.abs(x - xo) / np.maximum(1.0, np.abs(xo)))))
    assert conv.mean() >= 0.9, name
    assert np.array_equal(st["iterations"], it) and np.array_equal(st["converged"], conv), name
    assert np.array_equal(st["n_unsatisfied"], nun) and np.array_equal(mask, mo), name
    for k in range(STEPS):
        for b in range(SWEEPS):
            assert_batch_matches_oracle(substituted(recs, pos, params[k, b]), begin[k, b][None, :], x[k, b][None, :],
                                        st["iterations"][k, b:b + 1], st["converged"][k, b:b + 1], None,
                                        oracle_result=(xo[k, b][None, :], it[k, b:b + 1], conv[k, b:b + 1]), what=f"{name}[{k}, {b}]")


@pytest.mark.parametrize("name, n_drive, in_lds", SHAPE_CASES, ids=SHAPE_IDS)
def test_same_bits_as_the_chain_of_calls(E, shape_of, name, n_drive, in_lds):
    recs, g, team, mode = shape_of[name]
    s = E.System(recs, len(g), team_size=team)
    assert s.info()["team_mode"] == mode, (name, s.info())
    pos, params, x0 = driven_walk(E, recs, g, 8, 6, 21, n_drive=n_drive)
    plan = s.sweep_params_plan(pos)
    print(name, len(pos), "driven", plan)
    assert plan["route_name"] == name and plan["params_in_lds"] == in_lds, plan
    if name in IN_KERNEL_ROUTES:
        assert plan["in_kernel"] == 1, plan
    got = s.sweep_params(x0, pos, params, want_mask=True)
    _same(got, chain_of_calls(s, x0, pos, params), name)
    assert not np.array_equal(got[0][0], got[0][5])  # (the steps do differ)
    # one step is the params entry
    x1, st1, m1 = s.sweep_params(x0, pos, params[:1], want_mask=True)
    xp, stp, mp = s.solve_batch_params(x0, pos, params[0], want_mask=True)
    _same((x1[0], st1[0], m1[0]), (xp, stp, mp), name + ", one step")
    # no driven parameter: re-solves with the system's own values, each from the one before
    x3, st3, m3 = s.sweep_params(x0, [], np.zeros((3, 8, 0)), want_mask=True)
    xa = x0
    for k in range(3):
        xa, sta, ma = s.solve_batch(xa, want_mask=True)
        _same((x3[k], st3[k], m3[k]), (xa, sta, ma), name + ", no parameters, step %d" % k)
    # nothing to do: EZPZ_OK, shapes only
    xe, ste, _ = s.sweep_params(x0, pos, params[:0])
    assert xe.shape == (0, 8, len(g)) and ste.shape == (0, 8)


@pytest.mark.parametrize("name, n_drive, in_lds", SHAPE_CASES, ids=SHAPE_IDS)
def test_a_teams_second_sweep(E, shape_of, name, n_drive, in_lds):
    """More sweeps than the launch has teams, parameters that differ between consecutive steps and sweeps: what a team carries over
    from a finished sweep -- the values in its workspace, the parity of its copies, the warning counter, the driven values in
    LDS -- would show.  (The launches' grids: at most 32 x 8 workgroups per CU of one sweep each; 32 workgroups per CU of
    256 / team_size teams each for sub-wavefront teams.)  The partitioned workgroup with 16 driven values is the case whose two
    LDS copies must alternate by (sweep, step): with a copy chosen by sweep, a wavefront that is a step ahead would overwrite the
    values under a wavefront still in the step before; 3 steps per sweep, so a team's sweeps also begin on alternating copies."""
    recs, g, team, mode = shape_of[name]
    s = E.System(recs, len(g), team_size=team)
    info = s.info()
    assert info["team_mode"] == mode, (name, info)
    cus = _cus()
    teams = cus * 32 * (256 // info["team_size"]) if mode == 0 else cus * 32 * 8
    sweeps = teams + 64
    # (parameter sets repeat with period 8 sweeps -- every step has its own -- the starts all differ)
    pos, p8, _ = driven_walk(E, recs, g, 8, 3, 33, n_drive=n_drive)
    plan = s.sweep_params_plan(pos)
    assert plan["route_name"] == name and plan["params_in_lds"] == in_lds, plan
    params = np.ascontiguousarray(np.tile(p8, (1, sweeps // 8, 1)))
    x0 = g[None, :] + np.random.default_rng(34).uniform(-0.03, 0.03, (sweeps, len(g)))
    _same(s.sweep_params(x0, pos, params, want_mask=True), chain_of_calls(s, x0, pos, params), name)


def test_workspace_in_global_memory(E):
    recs, g = chain(2000)
    s = E.System(recs, len(g), team_size=256)
    info = s.info()
    assert info["workspace_in_lds"] == 0 and info["grid_workgroups"] == 1 and info["team_mode"] == 2, info
    cfg = E.Config().with_max_iterations(3)
    plan = s.sweep_params_plan([2])
    assert plan["route_name"] == "barrier workgroup" and plan["in_kernel"] == 1 and plan["params_in_lds"] == 1, plan
    for sweeps, steps in ((4, 3), (_cus() * 16 + 8, 2)):
        pos, p4, _ = driven_walk(E, recs, g, 4, steps, 35)
        # (every parametrised constraint driven: 16 KB of values beside 50 KB of LDS would cost the CU a workgroup, so these runs
        # read them from global memory; the one-value list above would be staged)
        assert s.sweep_params_plan(pos)["params_in_lds"] == 0
        params = np.ascontiguousarray(np.tile(p4, (1, sweeps // 4, 1)))
        x0 = g[None, :] + np.random.default_rng(36).uniform(-0.03, 0.03, (sweeps, len(g)))
        _same(s.sweep_params(x0, pos, params, config=cfg, want_mask=True), chain_of_calls(s, x0, pos, params, cfg), (sweeps, steps))


@pytest.mark.parametrize("name", ["sub-wavefront teams", "barrier workgroup", "record walk"])
def test_a_step_that_fails_does_not_break_the_chain(E, shape_of, name):
    """One iteration per step on non-linear systems: most steps end unconverged, and the next starts from what they left."""
    recs, g, team, mode = shape_of[name]
    s = E.System(recs, len(g), team_size=team)
    cfg = E.Config().with_max_iterations(1)
    pos, params, x0 = driven_walk(E, recs, g, 16, 5, 41, amplitude=0.3, jitter=0.1)
    got = s.sweep_params(x0, pos, params, config=cfg, want_mask=True)
    print(name, "converged", int(got[1]["converged"].sum()), "of", got[1].size)
    assert got[1]["converged"].mean() < 0.5
    _same(got, chain_of_calls(s, x0, pos, params, cfg), name)


def _logged_chain(s, x0, pos, params, warn_cap):
    """The chain of calls with the warning log of every step: ezpz_system_solve_batch_params, host form."""
    import ezpz_amd
    from ezpz_amd._lib import STATUS_DTYPE

    steps, batch = params.shape[:2]
    cfg = ezpz_amd.Config()._c()
    xs, sts, logs = [], [], []
    x = np.ascontiguousarray(x0)
    for k in range(steps):
        xo = np.empty_like(x)
        st = np.zeros(batch, dtype=STATUS_DTYPE)
        log = np.zeros((batch, warn_cap), dtype=np.uint64)
        p = np.ascontiguousarray(params[k])
        rc = ezpz_amd.lib().ezpz_system_solve_batch_params(s._h, x.ctypes.data, pos.ctypes.data, len(pos), p.ctypes.data, batch, C.byref(cfg),
                                                           xo.ctypes.data, st.ctypes.data, None, log.ctypes.data, warn_cap)
        assert rc == 0
        xs.append(xo), sts.append(st), logs.append(log)
        x = xo
    return np.stack(xs), np.stack(sts), np.stack(logs)


def test_warnings_per_step(E):
    """A distance whose points are driven onto each other: P1's two Fixed constraints and the distance's length are driven so that
    step 2's answer has P1 on P0.  The distance's Jacobian is degenerate where the points are within EPSILON (solver.rs:340-346): at
    the refresh after the accepted step of step 2, and at the evaluation that opens step 3, which starts from that answer -- so
    those two steps log warnings in their own rows, and the steps before and after log none.  Counts and (sorted) log rows are
    the chain's."""
    cons = [O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(2, 1.0), O.fixed(3, 0.0), O.distance(P0, P1, 1.0)]
    recs = O.stack(cons)
    s = E.System(recs, 4, team_size=E.TEAM_AUTO_LISTS)
    pos = np.asarray([2, 4], dtype=np.uint32)
    a = np.asarray([1.0, 0.5, 0.0, 0.75, 1.5])  # where P1.x is fixed, step by step (P0 stays at the origin)
    sweeps, cap = 4, 16
    params = np.ascontiguousarray(np.repeat(np.stack([a, np.abs(a)], axis=1)[:, None, :], sweeps, axis=1))
    x0 = np.asarray([0.0, 0.0, 1.0, 0.0])[None, :] + np.random.default_rng(5).uniform(-0.01, 0.01, (sweeps, 4))
    log = np.zeros((len(a), sweeps, cap), dtype=np.uint64)
    x, st, _ = s.sweep_params(x0, pos, params, warn_log=log)
    xc, stc, logc = _logged_chain(s, x0, pos, params, cap)
    print("warnings per step:", st["n_warnings"].tolist())
    assert np.array_equal(x, xc) and st.tobytes() == stc.tobytes()
    for k in range(len(a)):
        for b in range(sweeps):
            nw = int(st["n_warnings"][k, b])
            assert nw <= cap
            assert np.array_equal(np.sort(log[k, b, :nw]), np.sort(logc[k, b, :nw])), (k, b)
            assert np.all(log[k, b, nw:] == 0), (k, b)  # (nothing of another step's in this row)
    warned = sorted(set(np.nonzero(st["n_warnings"].sum(axis=1))[0].tolist()))
    assert warned == [2, 3], warned


def _assert_declined(E, s, x0, pos, params, steps):
    from ezpz_amd._lib import STATUS_DTYPE

    batch = len(x0)
    x = np.full((steps, batch, x0.shape[1]), -777.0)
    st = np.full(steps * batch, 0xAB, dtype=np.uint8).repeat(STATUS_DTYPE.itemsize).view(STATUS_DTYPE)
    st_before = st.copy()
    pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.uint32)
    params = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    cfg = E.Config()._c()
    n_param = 1 if pos is None else len(pos)
    rc = E.lib().ezpz_system_sweep_params(s._h, x0.ctypes.data, None if pos is None else pos.ctypes.data, n_param,
                                          None if params is None else params.ctypes.data, steps, batch, C.byref(cfg), x.ctypes.data,
                                          st.ctypes.data, None, None, 0)
    assert rc == ERR_INVALID_ARGUMENT, rc
    assert np.all(x == -777.0) and st.tobytes() == st_before.tobytes()


def test_errors_leave_outputs_untouched_and_a_grid_team_is_declined(E):
    recs, g, _ = CASES["axis_distances_and_fixed"]
    recs = O.stack(list(recs) + [O.horizontal(P0, P1)])  # position 4: a constraint without a parameter
    s = E.System(recs, len(g), team_size=E.TEAM_AUTO_LISTS)
    x0 = np.repeat(g[None, :], 4, axis=0)
    one = np.ones((3, 4, 1))
    _assert_declined(E, s, x0, [5], one, 3)                    # a position >= n_cs
    _assert_declined(E, s, x0, [2, 2], np.ones((3, 4, 2)), 3)  # a duplicate
    _assert_declined(E, s, x0, [4], one, 3)                    # no parameter
    _assert_declined(E, s, x0, None, one, 3)                   # null positions
    _assert_declined(E, s, x0, [2], None, 3)                   # null params
    with pytest.raises(ValueError):
        s.sweep_params(x0, [2], np.ones((3, 3, 1)))
    with pytest.raises(ValueError):
        s.sweep_params(x0, [2], np.ones((4, 1)))
    # a system that one solve spreads over several workgroups
    lad = T.load(T.gen_big_problem(12000))
    lrecs = O.stack(lad.constraints)
    big = E.System(lrecs, lad.num_vars)
    assert big.info()["grid_workgroups"] > 1, big.info()
    pos, params, x0 = driven_walk(E, lrecs, lad.guesses, 2, 2, 2)
    _assert_declined(E, big, x0, pos, params, 2)
    with pytest.raises(E.NonLinearSystemError):
        big.sweep_params_plan(pos)


def _device_sweep(E, s, torch, x0, pos, params, stream, in_place):
    from ezpz_amd._lib import STATUS_DTYPE

    steps, batch = params.shape[:2]
    n = x0.shape[1]
    with torch.cuda.stream(stream):
        pd = torch.from_numpy(params).cuda()
        xo = torch.zeros((steps, batch, n), dtype=torch.float64, device="cuda")
        if in_place:
            xo[0].copy_(torch.from_numpy(x0))
            xin = xo
        else:
            xin = torch.from_numpy(x0).cuda()
        std = torch.zeros(steps * batch * STATUS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        s.sweep_params_device(xin.data_ptr(), pos, pd.data_ptr(), steps, batch, xo.data_ptr(), std.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return xo.cpu().numpy(), std.cpu().numpy().view(STATUS_DTYPE).reshape(steps, batch)


def _trace(E, call):
    """The stamps of csrc/call_trace.hpp a call left (ids only)."""
    trace = np.zeros(64, dtype=np.uint64)
    E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
    try:
        call()
    finally:
        k = E.lib().ezpz_debug_call_trace(None, 0)
    return [int(v) for v in trace[:k:2]]


SWEEP_TABLE_UPLOADED, SWEEP_LAUNCHED = 30, 31


def test_device_form(E):
    import torch

    from ezpz_amd._lib import STATUS_DTYPE

    recs, g, driven = CASES["arc_radius"]
    _, pos, params, x0 = oracle_inputs("arc_radius", seed=11)
    params, x0 = np.ascontiguousarray(params[:5]), x0
    s = E.System(recs, len(g), team_size=E.TEAM_AUTO_LISTS)
    x, st, _ = chain_of_calls(s, x0, pos, params, want_mask=False)
    stream = torch.cuda.Stream()
    for in_place in (False, True):
        xd, std = _device_sweep(E, s, torch, x0, pos, params, stream, in_place)
        assert np.array_equal(xd, x) and std.tobytes() == st.tobytes(), in_place
    # a list the system has not seen is turned into its table first; repeated, the call only enqueues
    other = np.asarray([4, 0], dtype=np.uint32)
    p2 = np.ascontiguousarray(np.stack([params[..., 0], np.zeros(params.shape[:2])], axis=2))
    first = _trace(E, lambda: _device_sweep(E, s, torch, x0, other, p2, stream, False))
    again = _trace(E, lambda: _device_sweep(E, s, torch, x0, other, p2, stream, False))
    assert first == [SWEEP_TABLE_UPLOADED, SWEEP_LAUNCHED] and again == [SWEEP_LAUNCHED], (first, again)
    # a params call in between, on the same system and list, and the sweep again: right answers both
    with torch.cuda.stream(stream):
        xd1 = torch.from_numpy(x0).cuda()
        pd1 = torch.from_numpy(np.ascontiguousarray(p2[0])).cuda()
        st1 = torch.zeros(len(x0) * STATUS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        s.solve_batch_params_device(xd1.data_ptr(), other, pd1.data_ptr(), len(x0), xd1.data_ptr(), st1.data_ptr(), stream=stream.cuda_stream)
    xs, sts = _device_sweep(E, s, torch, x0, other, p2, stream, True)
    stream.synchronize()
    xc, stc, _ = chain_of_calls(s, x0, other, p2, want_mask=False)
    assert np.array_equal(xs, xc) and sts.tobytes() == stc.tobytes()
    assert np.array_equal(xd1.cpu().numpy(), xc[0]) and st1.cpu().numpy().view(STATUS_DTYPE).tobytes() == stc[0].tobytes()


def _answer(E, call, s):
    """What a call gives on `s`: its results, or the error code it is declined with."""
    try:
        return call(s), None
    except E.NonLinearSystemError as e:
        return None, e.code


@pytest.mark.parametrize("name", list(ROUTES) + ["fronts"])
def test_entries_interleaved_on_one_system(E, shape_of, monkeypatch, name):
    """The three driven entries take turns on ONE system with two lists: what the system keeps of a `positions` list -- the params
    and sweep entries' shared table, the sensitivity route's plan -- is replaced, matched and reused between them.  Every result is
    bit for bit that of the same call made as the first and only call on a fresh system; a sensitivity call that a fresh system
    declines (a component above EZPZ_SENSITIVITY_MAX_COMPONENT_VARS on the default route) is declined here with the same error."""
    if name == "fronts":
        (recs, g), team, mode = chain(40), E.TEAM_FRONTS, 5
        monkeypatch.setenv("EZPZ_FRONT_WGS", "1")
    else:
        recs, g, team, mode = shape_of[name]

    def system():
        s = E.System(recs, len(g), team_size=team)
        assert s.info()["team_mode"] == mode, (name, s.info())
        if name == "fronts":
            assert s.info()["grid_workgroups"] == 1
            s.set_params_route("fronts")
            s.set_sensitivity_route("fronts")
        return s

    pos_a, par_a, x0_a = driven_walk(E, recs, g, 8, 3, 61)
    pos_b, par_b, x0_b = driven_walk(E, recs, g, 8, 3, 62, n_drive=2)
    assert len(pos_a) != len(pos_b)
    lists = {"A": (pos_a, par_a, x0_a), "B": (pos_b, par_b, x0_b)}

    def params(which):
        pos, par, x0 = lists[which]
        return lambda s: s.solve_batch_params(x0, pos, par[0], want_mask=True)

    def sweep(which):
        pos, par, x0 = lists[which]
        return lambda s: s.sweep_params(x0, pos, par, want_mask=True)

    def sensitivity(which):
        pos, par, x0 = lists[which]
        return lambda s: s.param_sensitivity(x0, pos, par[1], want_degenerate=True)

    order = [("params", params, "A"), ("sweep", sweep, "B"), ("params", params, "A"), ("sensitivity", sensitivity, "A"),
             ("sweep", sweep, "A"), ("sensitivity", sensitivity, "B"), ("params", params, "B")]
    shared = system()
    for i, (entry, make, which) in enumerate(order):
        what = "%s: call %d, %s(%s)" % (name, i, entry, which)
        call = make(which)
        got, got_err = _answer(E, call, shared)
        want, want_err = _answer(E, call, system())
        assert got_err == want_err, (what, got_err, want_err)
        if entry != "sensitivity":
            assert want_err is None, (what, want_err)
            _same(got, want, what)
        elif want_err is None:
            for a, b in zip(got, want):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), what
        else:
            assert want_err == ERR_INVALID_ARGUMENT, (what, want_err)
            print(what, "declined on both with", want_err)


def test_device_form_under_graph_capture(E):
    """A one-workgroup shape captured into a graph replays to the same bits.  Skipped, with the reason, where the params entry
    itself cannot be captured: the sweep enqueues exactly what that entry enqueues (a wait for the system's event, one launch,
    the event's record)."""
    import torch

    from ezpz_amd._lib import STATUS_DTYPE

    recs, g = chain(40)
    s = E.System(recs, len(g), team_size=256)
    assert s.info()["team_mode"] == 2
    pos, params, x0 = driven_walk(E, recs, g, 1, 4, 51)
    want = chain_of_calls(s, x0, pos, params, want_mask=False)
    steps, batch, n = params.shape[0], 1, len(g)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xin = torch.from_numpy(x0).cuda()
        pd = torch.from_numpy(params).cuda()
        xo = torch.zeros((steps, batch, n), dtype=torch.float64, device="cuda")
        std = torch.zeros(steps * batch * STATUS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        # (both entries once outside capture: tables uploaded, kernels loaded)
        s.sweep_params_device(xin.data_ptr(), pos, pd.data_ptr(), steps, batch, xo.data_ptr(), std.data_ptr(), stream=stream.cuda_stream)
        s.solve_batch_params_device(xin.data_ptr(), pos, pd.data_ptr(), batch, xo.data_ptr(), std.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    try:
        probe = torch.cuda.CUDAGraph()
        with torch.cuda.graph(probe, stream=stream):
            s.solve_batch_params_device(xin.data_ptr(), pos, pd.data_ptr(), batch, xo.data_ptr(), std.data_ptr(),
                                        stream=torch.cuda.current_stream().cuda_stream)
    except Exception as e:  # noqa: BLE001
        pytest.skip("the params entry itself is not capturable here: %r" % (e,))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        s.sweep_params_device(xin.data_ptr(), pos, pd.data_ptr(), steps, batch, xo.data_ptr(), std.data_ptr(),
                              stream=torch.cuda.current_stream().cuda_stream)
    xo.zero_(), std.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(xo.cpu().numpy(), want[0])
    assert std.cpu().numpy().view(STATUS_DTYPE).reshape(steps, batch).tobytes() == want[1].tobytes()
