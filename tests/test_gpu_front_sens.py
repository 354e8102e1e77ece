"""Dimension sensitivities on the FRONTAL shape (ezpz_system_set_sensitivity_route; csrc/front_sens.hip, front_sens_kernel: one
factorisation on the fronts, many right-hand sides): against the numpy reference of tests/sensitivity_ref.py at
its own rule max(1e-10, 20 x spread) -- tests/test_front_sens_cpu.py measures the spreads of exactly these systems --, above the
1024-variable limit of the default route, bit for bit however the rows are asked for, failures that stay local, exact zeros,
their meaning (finite differences of two solves), the device form, autograd above the limit, and the setter.  From section 10 on,
what connected_sketch and graph_sketch never put on the device: every kind with a parameter as a right-hand side (the second row
of ArcRadius, ArcLength, PointsAtAngle; the sincos branches of con_dparam per degree and per radian), weights that are not 1,
guards that fire on listed constraints, and the linear build (the conditions on those inputs: tests/test_front_sens_cpu.py)."""
import contextlib
import os
import warnings

import numpy as np
import pytest

import front_sens_ref as FS
import sensitivity_ref as R
from oracle import oracle as O
from test_gpu_front_params import env, front_system

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
_LOG_STARTED = False


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


def _log(line):
    """sensitivity_ref.log's rule, into $EZPZ_PROFILE_DIR/front_sens_bar.txt."""
    global _LOG_STARTED
    out = os.environ.get("EZPZ_PROFILE_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "front_sens_bar.txt"), "a" if _LOG_STARTED else "w") as f:
            f.write(line + "\n")
        _LOG_STARTED = True


@contextlib.contextmanager
def logging_here():
    """sensitivity_ref.assert_matches logs through sensitivity_ref.log: into this file's profile while the block runs."""
    old, R.log = R.log, _log
    try:
        yield
    finally:
        R.log = old


_SYSTEMS = {}


def _system(E, name, wgs, route="fronts"):
    """A system on the fronts with `wgs` workgroups (0: what the planner gives), the sensitivity route set."""
    key = (name, wgs, route)
    if key not in _SYSTEMS:
        recs, g = FS.inputs(name)
        if wgs:
            s = front_system(E, recs, len(g), wgs, route=None)
        else:
            s = E.System(recs, len(g), team_size=E.TEAM_FRONTS)
            assert s.info()["team_mode"] == 5 and s.info()["front_max_batch"] == 0xFFFFFFFF, s.info()
        if route:
            s.set_sensitivity_route(route)
        _SYSTEMS[key] = s
    return _SYSTEMS[key]


@contextlib.contextmanager
def rhs_per_item(n):
    with env(EZPZ_SENS_FRONTS_RHS_PER_ITEM=n):
        yield


# ---- 1. against the numpy reference -------------------------------------------------------------------------------------------------
WIDE_CASES = [(name, wgs) for name in FS.WIDE for wgs in FS.WIDE_WGS[name]]


@pytest.mark.parametrize("name,wgs", [("sketch25", 1), ("sketch75", 2), ("sketch150", 3), ("band", 1), ("band", 4), ("hub", 1), ("hub", 4),
                                      ("mixed40", 1), ("mixed40", 3), ("mixed40:unit", 3)] + WIDE_CASES)
def test_against_the_numpy_reference(E, name, wgs):
    """If a system exceeded the rule, the default route's error on it (the parent's code, an independent implementation) would be
    measured and 4 x that granted instead: it has not been needed -- the errors are logged beside the bars.
    The wide inputs (front_sens_ref.WIDE; their plans' shapes: test_wide_inputs_are_what_they_claim): fronts of 58, 36, 59 and 63
    rows -- at 63 lane 63 holds the right-hand side's row --, remote children of 52, 30, 34 and 56 rows whose last rows arrive as
    chunks, minimum-degree plans (tree108, tree144).  (Measured, profiles/front_sens_bar.txt: tree60 6.5e-13 at most, tree108
    1.5e-9 against 2.9e-8, tree144 1.3e-10 against 2.0e-9, comb213 1.8e-7 against 2.5e-6.)"""
    sysobj, s = _system(E, name, wgs), FS.system(name)
    plan = sysobj.param_sensitivity_plan(s["pos"])
    print(name, wgs, plan)
    assert plan["route"] == 1 and plan["front_workgroups"] == wgs and plan["rhs_per_item"] * plan["items_per_system"] >= len(s["pos"])
    S, st, deg = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"], want_degenerate=True)
    assert S.shape == (len(s["x"]), len(s["pos"]), s["n_vars"]) and not st.any()
    with logging_here():
        for b, (Sref, spread) in enumerate(FS.references(name)):
            assert deg[b] == R.degenerate_count(s["recs"], s["x"][b], s["pos"], s["params"][b]), (name, b)
            R.assert_matches(S[b], Sref, spread, f"fronts, {name} on {wgs} workgroup(s) [{b}]")


@pytest.mark.parametrize("name,wgs", WIDE_CASES)
def test_wide_inputs_on_the_default_route(E, name, wgs):
    """The same systems with the route set to "default" and back: each is one component under that route's 1024-variable limit,
    so it serves them too -- an independent device implementation beside the reference, at the same bar.  An error of the fronts
    alone belongs to the fronts' kernel, one on both routes to the input.  (Measured: tree60 4.5e-13, tree108 3.1e-9, tree144
    1.5e-10, comb213 1.9e-7 -- the size of the fronts' own errors.)"""
    sysobj, s = _system(E, name, wgs), FS.system(name)
    sysobj.set_sensitivity_route("default")
    try:
        assert sysobj.param_sensitivity_plan(s["pos"])["route"] == 0
        S, st, deg = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"], want_degenerate=True)
    finally:
        sysobj.set_sensitivity_route("fronts")
    assert sysobj.param_sensitivity_plan(s["pos"])["route"] == 1
    assert S.shape == (len(s["x"]), len(s["pos"]), s["n_vars"]) and not st.any() and not deg.any()
    with logging_here():
        for b, (Sref, spread) in enumerate(FS.references(name)):
            R.assert_matches(S[b], Sref, spread, f"default route, {name} created on {wgs} workgroup(s) [{b}]")


# ---- 2. above the limit ---------------------------------------------------------------------------------------------------------------
def test_above_the_limit(E):
    """sketch600: 1200 variables in one component.  The default route declines and touches nothing; the fronts serve it."""
    s = FS.system("sketch600", 2, FS.sixteen)
    sysobj = _system(E, "sketch600", 0, route=None)
    n, k = s["n_vars"], len(s["pos"])
    assert n == 1200 and k == 16
    x, p = np.ascontiguousarray(s["x"]), np.ascontiguousarray(s["params"])
    S = np.full((2, k, n), 7.0)
    st, deg = np.full(2, 9, np.uint32), np.full(2, 5, np.uint32)
    call = lambda: E.lib().ezpz_system_param_sensitivity(sysobj._h, x.ctypes.data, s["pos"].ctypes.data, k, p.ctypes.data, 2, s["lam"],
                                                         S.ctypes.data, st.ctypes.data, deg.ctypes.data)
    assert call() == ERR_INVALID_ARGUMENT and np.all(S == 7.0) and np.all(st == 9) and np.all(deg == 5)
    sysobj.set_sensitivity_route("fronts")
    try:
        plan = sysobj.param_sensitivity_plan(s["pos"])
        print("sketch600", plan, "grid_workgroups", sysobj.info()["grid_workgroups"])
        assert plan["route"] == 1 and plan["front_workgroups"] == sysobj.info()["grid_workgroups"]
        assert call() == 0 and not st.any()
        with logging_here():
            for b, (Sref, spread) in enumerate(FS.references("sketch600", 2, FS.sixteen)):
                assert deg[b] == R.degenerate_count(s["recs"], s["x"][b], s["pos"], s["params"][b])
                R.assert_matches(S[b], Sref, spread, f"fronts, sketch600 on {plan['front_workgroups']} workgroup(s) [{b}]")
    finally:
        sysobj.set_sensitivity_route("default")


# ---- 3. the same bits, however asked ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,wgs", [("sketch75", 2), ("hub", 1), ("tree60", 2), ("comb213", 4)])
def test_the_same_bits_however_asked(E, name, wgs):
    """Parameters are the system's own values (None), so that a shorter list leaves the constraints it drops at the same values.
    (comb213: S is 426 x 426 doubles per system, so its tiled call has 16 systems, the others' 64.)"""
    sysobj, s = _system(E, name, wgs), FS.system(name)
    pos, x = s["pos"], s["x"]
    k = len(pos)
    full, st = sysobj.param_sensitivity(x, pos, None, lam=s["lam"])
    assert not st.any()
    again, _ = sysobj.param_sensitivity(x, pos, None, lam=s["lam"])
    assert np.array_equal(full, again)
    perm = np.random.default_rng(3).permutation(k)
    a, _ = sysobj.param_sensitivity(x, pos[perm], None, lam=s["lam"])
    assert np.array_equal(a, full[:, perm])
    a, _ = sysobj.param_sensitivity(x, pos[: k // 2], None, lam=s["lam"])
    assert np.array_equal(a, full[:, : k // 2])
    a, _ = sysobj.param_sensitivity(x, pos[k // 3: k // 3 + 1], None, lam=s["lam"])
    assert np.array_equal(a, full[:, k // 3: k // 3 + 1])
    for n in (1, 3):
        with rhs_per_item(n):
            assert sysobj.param_sensitivity_plan(pos)["rhs_per_item"] == n
            a, _ = sysobj.param_sensitivity(x, pos, None, lam=s["lam"])
        assert np.array_equal(a, full), n
    one, _ = sysobj.param_sensitivity(x[:1], pos, None, lam=s["lam"])
    assert np.array_equal(one[0], full[0])
    tiled, st = sysobj.param_sensitivity(np.tile(x[:1], (16 if name == "comb213" else 64, 1)), pos, None, lam=s["lam"])
    assert not st.any() and np.array_equal(tiled, np.broadcast_to(one, tiled.shape))
    order = np.asarray([1, 0])
    a, _ = sysobj.param_sensitivity(x[order], pos, None, lam=s["lam"])
    assert np.array_equal(a, full[order])
    # with a parameter row per system the rows are those of the list's own values
    a, _ = sysobj.param_sensitivity(x, pos, s["params"], lam=s["lam"])
    b, _ = sysobj.param_sensitivity(x[order], pos[perm], s["params"][order][:, perm], lam=s["lam"])
    assert np.array_equal(b, a[order][:, perm])


def _second_item(E, name, wgs, tiles):
    """8 listed positions make one item per system; a 512-thread workgroup has a quarter of a CU at the least, so a launch has at
    most 4 x CUs / wgs slots: with twice as many tiled systems every slot takes a further item."""
    import torch

    sysobj, s = _system(E, name, wgs), FS.system(name)
    pos = s["pos"][np.linspace(0, len(s["pos"]) - 1, 8).astype(int)]
    plan = sysobj.param_sensitivity_plan(pos)
    assert plan["front_workgroups"] == wgs and plan["rhs_per_item"] == 8 and plan["items_per_system"] == 1, plan
    assert tiles >= 2 * (4 * int(torch.cuda.get_device_properties(0).multi_processor_count) // wgs)
    one, _ = sysobj.param_sensitivity(s["x"][:1], pos, None, lam=s["lam"])
    big, st = sysobj.param_sensitivity(np.tile(s["x"][:1], (tiles, 1)), pos, None, lam=s["lam"])
    assert not st.any() and np.array_equal(big, np.broadcast_to(one, big.shape))


def test_a_workgroups_second_item(E):
    """sketch25, 8 listed positions, 4096 tiled systems (13 MB of S): persistent workgroups take further items."""
    _second_item(E, "sketch25", 1, 4096)


def test_a_slots_second_item_with_a_wide_remote_child(E):
    """tree60 on 2 workgroups, 8 listed positions, 2048 tiled systems (16 MB of S): the chunks of the 52-row remote child are
    reused across items and epochs."""
    _second_item(E, "tree60", 2, 2048)


# ---- 4. failures stay local ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,wgs", [("sketch25", 1), ("sketch150", 3), ("tree144", 4)])
def test_failures_stay_local(E, name, wgs):
    """A lambda below minus the smallest eigenvalue of JtJ: status 1 and NaN rows (a numerical status, no fault).  A NaN start in
    system 2 of 4: its rows alone are NaN, the others' bits are the good call's, and so are those of the call after it."""
    sysobj, s = _system(E, name, wgs), FS.system(name)
    x = np.tile(s["x"], (2, 1))
    p = np.tile(s["params"], (2, 1))
    good, st = sysobj.param_sensitivity(x, s["pos"], p, lam=s["lam"])
    assert not st.any()
    J = R.jacobian(R.substituted(s["recs"], s["pos"], p[1]), x[1], s["n_vars"])
    lam_bad = -(np.linalg.eigvalsh(J.T @ J)[0] * 1.5 + 1.0)
    bad, st = sysobj.param_sensitivity(x[1:2], s["pos"], p[1:2], lam=lam_bad)
    assert st[0] == 1 and np.isnan(bad).all()
    xx = x.copy()
    xx[2] = np.nan
    S, st = sysobj.param_sensitivity(xx, s["pos"], p, lam=s["lam"])
    assert st.tolist() == [0, 0, 1, 0] and np.isnan(S[2]).all()
    assert np.array_equal(S[[0, 1, 3]], good[[0, 1, 3]])
    after, st = sysobj.param_sensitivity(x, s["pos"], p, lam=s["lam"])
    assert not st.any() and np.array_equal(after, good)


# ---- 5. exact zeros -----------------------------------------------------------------------------------------------------------------------
def test_exact_zeros(E):
    """Two disjoint copies of sketch25 in one system; only constraints of the first are listed."""
    recs, g = FS.inputs("sketch25")
    second = recs.copy()
    for i in range(len(second)):
        second["ids"][i][: O.KIND_NUM_IDS[int(second["kind"][i])]] += 50
    both = np.concatenate([recs, second])
    s = FS.system("sketch25")
    sysobj = front_system(E, both, 100, 1, route=None)
    sysobj.set_sensitivity_route("fronts")
    x = np.concatenate([s["x"], s["x"]], axis=1)
    S, st = sysobj.param_sensitivity(x, s["pos"], s["params"], lam=s["lam"])
    assert not st.any()
    assert np.all(S[:, :, 50:] == 0.0) and not np.signbit(S[:, :, 50:]).any()
    assert np.any(S[:, :, :50] != 0.0)
    with logging_here():
        for b, (Sref, spread) in enumerate(FS.references("sketch25")):
            R.assert_matches(S[b][:, :50], Sref, spread, f"fronts, two copies of sketch25, the listed one [{b}]")


# ---- 6. meaning ------------------------------------------------------------------------------------------------------------------------------
def test_meaning_finite_differences_of_two_solves(E):
    """(x(p + delta e_j) - x(p)) / delta of two solve_batch_params calls on the fronts route, sketch150 on 3 workgroups, residual
    tolerance 1e-13, against S; granted: 4 x the distance between the ORACLE's same finite difference and the numpy S."""
    sysobj, s = _system(E, "sketch150", 3), FS.system("sketch150")
    sysobj.set_params_route("fronts")
    recs, pos, n = s["recs"], s["pos"], s["n_vars"]
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
    Sref, _ = R.reference(recs, n, xo[0], pos, rows[0], s["lam"])
    assert not status.any()
    for k, j in enumerate(picks):
        fd_dev, fd_orc = (x[k + 1] - x[0]) / delta, (xo[k + 1] - xo[0]) / delta
        scale = max(1.0, np.abs(Sref[j]).max())
        granted = 4.0 * np.abs(fd_orc - Sref[j]).max() / scale
        err = np.abs(fd_dev - S[0, j]).max() / scale
        print("meaning", j, "oracle's finite difference to numpy S", granted / 4.0, "device", err)
        _log(f"meaning, fronts, sketch150 parameter {j}: oracle's finite difference to the numpy S {granted / 4.0:.3e}; device's to its S {err:.3e} (granted {granted:.3e})")
        assert err <= granted, (j, err, granted)


# ---- 7. device form ---------------------------------------------------------------------------------------------------------------------------
def _device_call(sysobj, s, torch, stream, S, st, deg, x, p):
    sysobj.param_sensitivity_device(x.data_ptr(), s["pos"], p.data_ptr(), len(s["x"]), S.data_ptr(), st.data_ptr(), lam=s["lam"],
                                    degenerate_ptr=deg.data_ptr(), stream=stream.cuda_stream)


@pytest.mark.parametrize("name,wgs", [("sketch25", 1), ("sketch75", 2)])
def test_device_form(E, name, wgs):
    import torch

    sysobj, s = _system(E, name, wgs), FS.system(name)
    host, _, hdeg = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"], want_degenerate=True)
    x, p = torch.tensor(s["x"], device="cuda"), torch.tensor(s["params"], device="cuda")
    fresh = lambda: (torch.full(host.shape, 3.0, dtype=torch.float64, device="cuda"), torch.full((len(s["x"]),), 9, dtype=torch.int32, device="cuda"),
                     torch.full((len(s["x"]),), 9, dtype=torch.int32, device="cuda"))
    S, st, deg = fresh()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _device_call(sysobj, s, torch, stream, S, st, deg, x, p)
    stream.synchronize()
    assert np.array_equal(S.cpu().numpy(), host) and not st.cpu().numpy().any()
    assert np.array_equal(deg.cpu().numpy().astype(np.uint32), hdeg)
    S, st, deg = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    if wgs == 1:
        # a call captured after the list was planned replays the same bits
        with torch.cuda.graph(graph, stream=stream):
            _device_call(sysobj, s, torch, torch.cuda.current_stream(), S, st, deg, x, p)
        for _ in range(2):
            S.fill_(3.0)
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(S.cpu().numpy(), host) and not st.cpu().numpy().any()
    else:
        # several workgroups: a capturing stream is refused up front, nothing is enqueued, the outputs keep their sentinels
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # ("The CUDA Graph is empty")
            with pytest.raises(E.NonLinearSystemError) as err:
                with torch.cuda.graph(graph, stream=stream):
                    _device_call(sysobj, s, torch, torch.cuda.current_stream(), S, st, deg, x, p)
        assert err.value.code == ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert np.all(S.cpu().numpy() == 3.0) and np.all(st.cpu().numpy() == 9) and np.all(deg.cpu().numpy() == 9)
    # the next direct call gives the clean bits
    with torch.cuda.stream(stream):
        _device_call(sysobj, s, torch, stream, S, st, deg, x, p)
    stream.synchronize()
    assert np.array_equal(S.cpu().numpy(), host) and not st.cpu().numpy().any()


# ---- 8. autograd above the limit -----------------------------------------------------------------------------------------------------------
def test_autograd_above_the_limit(E):
    import torch

    from ezpz_amd import torch_ops

    s = FS.system("sketch600", 2, FS.sixteen)
    sysobj = _system(E, "sketch600", 0, route=None)
    sysobj.set_params_route("fronts")
    x0, p = torch.tensor(s["start"], device="cuda"), torch.tensor(s["params"], device="cuda")
    grad_x = torch.tensor(np.random.default_rng(2).uniform(-1.0, 1.0, s["x"].shape), device="cuda")
    # with the sensitivity route unset the forward runs on the fronts and the backward is declined, as it is today
    pt = p.clone().requires_grad_(True)
    xs = torch_ops.solve_params(sysobj, x0, s["pos"], pt, lam=s["lam"])
    with pytest.raises(E.NonLinearSystemError):
        xs.backward(grad_x)
    sysobj.set_sensitivity_route("fronts")
    try:
        pt = p.clone().requires_grad_(True)
        xs = torch_ops.solve_params(sysobj, x0, s["pos"], pt, lam=s["lam"])
        xs.backward(grad_x)
        got, gx, xf = pt.grad.cpu().numpy(), grad_x.cpu().numpy(), xs.detach().cpu().numpy()
        for b in range(len(xf)):
            Sref, spread = R.reference(s["recs"], s["n_vars"], xf[b], s["pos"], s["params"][b], s["lam"])
            scale = np.maximum(1.0, np.abs(Sref).max(axis=1))
            err = float((np.abs(got[b] - Sref @ gx[b]) / scale).max())
            print("autograd sketch600", b, err, R.bar(spread))
            _log(f"autograd, fronts, sketch600[{b}]: grad_params against S_ref grad_x: largest error {err:.3e} | bar granted {R.bar(spread):.3e} (spread {spread:.3e})")
            assert err <= R.bar(spread), (b, err, R.bar(spread))
    finally:
        sysobj.set_sensitivity_route("default")
        sysobj.set_params_route("default")


# ---- 9. the setter ---------------------------------------------------------------------------------------------------------------------------
def test_setter(E):
    L = E.lib()
    m = R.system("massive40")
    block = E.System(m["recs"], m["n_vars"])
    before, _ = block.param_sensitivity(m["x"], m["pos"], m["params"], lam=m["lam"])
    assert L.ezpz_system_set_sensitivity_route(block._h, 1) == ERR_INVALID_ARGUMENT
    with pytest.raises(E.NonLinearSystemError):
        block.set_sensitivity_route("fronts")
    after, _ = block.param_sensitivity(m["x"], m["pos"], m["params"], lam=m["lam"])
    assert np.array_equal(before, after) and block.param_sensitivity_plan(m["pos"])["route"] == 0
    s = FS.system("sketch150")
    plain = E.System(s["recs"], s["n_vars"])  # created by default: for batches
    never, _ = plain.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"])
    if plain.info()["front_max_batch"] != 0xFFFFFFFF:
        assert L.ezpz_system_set_sensitivity_route(plain._h, 1) == ERR_INVALID_ARGUMENT
        again, _ = plain.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"])
        assert np.array_equal(never, again)
    fronts = _system(E, "sketch150", 3, route=None)
    assert L.ezpz_system_set_sensitivity_route(fronts._h, 2) == ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        fronts.set_sensitivity_route("sideways")
    a, _ = fronts.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"])
    assert np.array_equal(a, never)  # the default route's bits do not depend on how the system was created
    fronts.set_sensitivity_route("fronts")
    on, _ = fronts.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"])
    assert fronts.param_sensitivity_plan(s["pos"])["route"] == 1
    fronts.set_sensitivity_route("default")
    off, _ = fronts.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"])
    assert fronts.param_sensitivity_plan(s["pos"])["route"] == 0
    assert np.array_equal(off, never) and not np.array_equal(on, never)


# ---- 10. kind by kind -----------------------------------------------------------------------------------------------------------------
SMALL = R.kind_names() + ["weighted", "under"]
# the small systems the planner of the fronts declines on their own: beside sketch25 as a disjoint second component
BESIDE_SKETCH25 = ()


def _small_system(E, name):
    """-> (the system on one workgroup, the first variable of `name` in it)."""
    key = (name, 1, "fronts")
    s = R.system(name)
    off = 50 if name in BESIDE_SKETCH25 else 0
    if key not in _SYSTEMS:
        recs = s["recs"]
        if off:
            first, g = FS.inputs("sketch25")
            assert len(g) == off
            recs = recs.copy()
            for i in range(len(recs)):
                recs["ids"][i][: O.KIND_NUM_IDS[int(recs["kind"][i])]] += off
            recs = np.concatenate([first, recs])
        sysobj = front_system(E, recs, off + s["n_vars"], 1, route=None)
        sysobj.set_sensitivity_route("fronts")
        _SYSTEMS[key] = sysobj
    return _SYSTEMS[key], off


@pytest.mark.parametrize("name", SMALL)
def test_kind_by_kind(E, name):
    """The 14 systems of tests/test_gpu_params.py's CASES -- one per kind with a parameter, the angle kinds per degree and per
    radian --, the over-determined `weighted` (weights change S in its first digit) and the under-determined `under`, on the
    fronts: S against the reference, the status, the degenerate count (a PointsAtAngle solve may end on a collapsed arm)."""
    sysobj, off = _small_system(E, name)
    s = R.system(name)
    x, pos = s["x"], s["pos"]
    if off:
        x = np.concatenate([np.repeat(FS.system("sketch25")["x"][:1], len(x), axis=0), x], axis=1)
        pos = pos + np.uint32(len(FS.inputs("sketch25")[0]))
    plan = sysobj.param_sensitivity_plan(pos)
    assert plan["route"] == 1 and plan["front_workgroups"] == 1, plan
    S, st, deg = sysobj.param_sensitivity(x, pos, s["params"], lam=s["lam"], want_degenerate=True)
    assert S.shape == (len(x), len(pos), off + s["n_vars"]) and not st.any()
    assert np.all(S[:, :, :off] == 0.0) and not np.signbit(S[:, :, :off]).any()
    with logging_here():
        for b, (Sref, spread) in enumerate(R.references(name)):
            assert deg[b] == R.degenerate_count(s["recs"], s["x"][b], s["pos"], s["params"][b]), (name, b)
            R.assert_matches(S[b][:, off:], Sref, spread, f"fronts, {name}[{b}]")


# ---- 11. the same bits however asked, two-row constraints in the list ------------------------------------------------------------------
def test_the_same_bits_with_two_row_constraints_in_the_list(E):
    """mixed40 on 3 workgroups.  A right-hand side of two rows leaves two entries in the residual-space vector; both are zero
    again before the next right-hand side of the chunk -- else the rows of a list [two-row, one-row, two-row, one-row] depend on
    how many right-hand sides share a work item.  Every row of a list is the row of its position asked alone."""
    sysobj, s = _system(E, "mixed40", 3), FS.system("mixed40")
    pos, x, lam = s["pos"], s["x"], s["lam"]
    k = len(pos)
    two = FS.two_row(s["recs"], pos)
    assert len(two) == 6
    full, st = sysobj.param_sensitivity(x, pos, None, lam=lam)
    assert not st.any()
    perm = np.random.default_rng(3).permutation(k)
    a, _ = sysobj.param_sensitivity(x, pos[perm], None, lam=lam)
    assert np.array_equal(a, full[:, perm])
    for j in two:
        a, st = sysobj.param_sensitivity(x, pos[j: j + 1], None, lam=lam)
        assert not st.any() and np.array_equal(a, full[:, j: j + 1]), j
    one = [j for j in range(k) if j not in two]
    angle = [j for j in one if int(s["recs"]["kind"][pos[j]]) in (O.LINES_AT_ANGLE, O.ARC_ANGLE)]
    mixed = np.asarray([two[0], angle[0], two[3], one[5]])  # (two[0] and two[3]: homes in workgroups 1 and 2)
    alone = np.concatenate([sysobj.param_sensitivity(x, pos[j: j + 1], None, lam=lam)[0] for j in mixed], axis=1)
    assert np.array_equal(alone, full[:, mixed])
    for n in (1, 2, 4):
        with rhs_per_item(n):
            assert sysobj.param_sensitivity_plan(pos[mixed])["rhs_per_item"] == n
            a, st = sysobj.param_sensitivity(x, pos[mixed], None, lam=lam)
        assert not st.any() and np.array_equal(a, alone), n
    single, _ = sysobj.param_sensitivity(x[:1], pos, None, lam=lam)
    assert np.array_equal(single[0], full[0])
    tiled, st = sysobj.param_sensitivity(np.tile(x[:1], (64, 1)), pos, None, lam=lam)
    assert not st.any() and np.array_equal(tiled, np.broadcast_to(single, tiled.shape))


# ---- 12. weights --------------------------------------------------------------------------------------------------------------------------
def test_weights_are_taken(E):
    """mixed40 with its drawn weights and with every weight 1.0, at the same values: S differs (each against its own reference:
    test_against_the_numpy_reference), by far more than either's bar."""
    s = FS.system("mixed40")
    a, st = _system(E, "mixed40", 3).param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"])
    b, stb = _system(E, "mixed40:unit", 3).param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"])
    assert not st.any() and not stb.any()
    scale = np.maximum(1.0, np.abs(a).max(axis=2))
    diff = float((np.abs(a - b).max(axis=2) / scale).max())
    print("weighted against unit weights at the same values:", diff)
    assert diff > 1e-3


@pytest.mark.parametrize("wgs", [1, 3])
def test_weights_of_two_and_four_lambda_give_the_bits_of_unit_weights(E, wgs):
    """Exact: every weight 2.0 scales J and g by 2 -- a power of two, so JtJ + 4 lam I and Jt g are 4 x those of unit weights
    in every bit, 1 / sqrt(pivot) is half, and every entry of S is the same double.  Unit weights take the kernel's unit_w
    path (weights not read), 2.0 the weighted one."""
    u, d = FS.system("mixed40:unit"), FS.system("mixed40:double")
    assert np.array_equal(u["x"], d["x"]) and d["lam"] == 4.0 * u["lam"] and np.all(d["recs"]["weight"] == 2.0)
    a, st = _system(E, "mixed40:unit", wgs).param_sensitivity(u["x"], u["pos"], u["params"], lam=u["lam"])
    b, stb = _system(E, "mixed40:double", wgs).param_sensitivity(d["x"], d["pos"], d["params"], lam=d["lam"])
    assert not st.any() and not stb.any()
    print("entries that differ:", int((a != b).sum()), "of", a.size)
    assert np.array_equal(a, b)


# ---- 13. guards that fire -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wgs", [1, 3])
def test_guards_on_listed_constraints(E, wgs):
    """mixed40+corner: three listed constraints on a line of length zero.  Each counts once (its Jacobian's guard and its
    residual's both fire), its g is zero, so its row of S is +0.0 in every entry -- as are the corner's variables in every row:
    no listed constraint with a g reaches that component."""
    name = "mixed40+corner"
    sysobj, s = _system(E, name, wgs), FS.system(name)
    n_base = FS.system("mixed40")["n_vars"]
    plan = sysobj.param_sensitivity_plan(s["pos"])
    assert plan["route"] == 1 and plan["front_workgroups"] == wgs, plan
    S, st, deg = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"], want_degenerate=True)
    assert not st.any() and deg.tolist() == [3, 3]
    assert np.all(S[:, -3:, :] == 0.0) and not np.signbit(S[:, -3:, :]).any()
    assert np.all(S[:, :, n_base:] == 0.0) and not np.signbit(S[:, :, n_base:]).any()
    with logging_here():
        for b, (Sref, spread) in enumerate(FS.references(name)):
            R.assert_matches(S[b][:-3], Sref[:-3], spread, f"fronts, {name} on {wgs} workgroup(s), the rows off the corner [{b}]")


# ---- 14. the linear build -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,wgs", [("linear100", 1), ("linear100", 3), ("linear100:weighted", 1), ("linear100:weighted", 3)])
def test_linear_build(E, name, wgs):
    """Fixed, HorizontalDistance, VerticalDistance only: front_sens_kernel<true> (the plan's linear_only follows from the kinds:
    tests/test_front_sens_cpu.py checks them; neither info() nor the sensitivity plan shows the flag).  J and g do not depend on
    x, so S at x and S at x + uniform(-1, 1) are the same bits."""
    sysobj, s = _system(E, name, wgs), FS.system(name)
    plan = sysobj.param_sensitivity_plan(s["pos"])
    assert plan["route"] == 1 and plan["front_workgroups"] == wgs, plan
    S, st, deg = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"], want_degenerate=True)
    assert not st.any() and not deg.any()
    with logging_here():
        for b, (Sref, spread) in enumerate(FS.references(name)):
            R.assert_matches(S[b], Sref, spread, f"fronts, {name} on {wgs} workgroup(s) [{b}]")
    moved = s["x"] + np.random.default_rng(9).uniform(-1.0, 1.0, s["x"].shape)
    again, st = sysobj.param_sensitivity(moved, s["pos"], s["params"], lam=s["lam"])
    assert not st.any() and np.array_equal(again, S)


# ---- 15. device form and autograd with every kind ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed40", "mixed40+corner"])
def test_device_form_with_every_kind(E, name):
    """On a stream, 3 workgroups: the host call's bits, the degenerate counts (0, and 3 with the corner) included."""
    import torch

    sysobj, s = _system(E, name, 3), FS.system(name)
    host, _, hdeg = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"], want_degenerate=True)
    x, p = torch.tensor(s["x"], device="cuda"), torch.tensor(s["params"], device="cuda")
    S = torch.full(host.shape, 3.0, dtype=torch.float64, device="cuda")
    st, deg = (torch.full((len(s["x"]),), 9, dtype=torch.int32, device="cuda") for _ in range(2))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _device_call(sysobj, s, torch, stream, S, st, deg, x, p)
    stream.synchronize()
    assert np.array_equal(S.cpu().numpy(), host) and not st.cpu().numpy().any()
    assert np.array_equal(deg.cpu().numpy().astype(np.uint32), hdeg) and hdeg.tolist() == ([3, 3] if name == "mixed40+corner" else [0, 0])


def test_autograd_with_every_kind(E):
    """mixed40 on 3 workgroups, both routes on the fronts: params.grad against S_ref grad_x at the forward's answer."""
    import torch

    from ezpz_amd import torch_ops

    s = FS.system("mixed40")
    sysobj = _system(E, "mixed40", 3, route=None)
    sysobj.set_params_route("fronts")
    sysobj.set_sensitivity_route("fronts")
    try:
        x0 = torch.tensor(s["start"], device="cuda")
        pt = torch.tensor(s["params"], device="cuda").requires_grad_(True)
        grad_x = torch.tensor(np.random.default_rng(2).uniform(-1.0, 1.0, s["x"].shape), device="cuda")
        xs = torch_ops.solve_params(sysobj, x0, s["pos"], pt, lam=s["lam"])
        xs.backward(grad_x)
        got, gx, xf = pt.grad.cpu().numpy(), grad_x.cpu().numpy(), xs.detach().cpu().numpy()
        for b in range(len(xf)):
            Sref, spread = R.reference(s["recs"], s["n_vars"], xf[b], s["pos"], s["params"][b], s["lam"])
            scale = np.maximum(1.0, np.abs(Sref).max(axis=1))
            err = float((np.abs(got[b] - Sref @ gx[b]) / scale).max())
            print("autograd mixed40", b, err, R.bar(spread))
            _log(f"autograd, fronts, mixed40[{b}]: grad_params against S_ref grad_x: largest error {err:.3e} | bar granted {R.bar(spread):.3e} (spread {spread:.3e})")
            assert err <= R.bar(spread), (b, err, R.bar(spread))
    finally:
        sysobj.set_sensitivity_route("default")
        sysobj.set_params_route("default")
