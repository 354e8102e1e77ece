"""Dimension sensitivities on the device (ezpz_system_param_sensitivity) against the numpy reference of
tests/sensitivity_ref.py -- every system checked, bar max(1e-10, 20 x the reference's own spread) * max(1, |S_j|_inf) --, their
meaning (finite differences of two solves), determinism, exact zeros, errors, the device form and the autograd layer."""
import numpy as np
import pytest

import sensitivity_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
MAX_COMPONENT_VARS = 1024


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


_SYSTEMS = {}


def _system(E, name):
    if name not in _SYSTEMS:
        s = R.system(name)
        _SYSTEMS[name] = E.System(s["recs"], s["n_vars"])
    return _SYSTEMS[name], R.system(name)


@pytest.mark.parametrize("name", R.all_names())
def test_against_the_numpy_reference(E, name):
    sysobj, s = _system(E, name)
    plan = sysobj.param_sensitivity_plan(s["pos"])
    print(name, plan)
    if name.startswith("kind:") or name == "massive40":
        assert plan["n_small"] == plan["n_active"] > 0
    if name == "sketch150":  # 300 variables in one component: the envelope (not the dense triangle) is what sits in LDS
        assert (plan["n_lds"], plan["n_workspace"], plan["max_component_vars"]) == (1, 0, 300) and plan["lds_bytes"] <= 64 * 1024
    if name == "hub512":  # the stated limit, on the global-memory workspace
        assert (plan["n_lds"], plan["n_workspace"], plan["max_component_vars"]) == (0, 1, MAX_COMPONENT_VARS)
    S, st, deg = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"], want_degenerate=True)
    assert S.shape == (len(s["x"]), len(s["pos"]), s["n_vars"]) and not st.any()
    for b, (Sref, spread) in enumerate(R.references(name)):
        # (a solve may end on a degenerate root -- PointsAtAngle with a collapsed arm: the count says so, rows of J and g are zero)
        assert deg[b] == R.degenerate_count(s["recs"], s["x"][b], s["pos"], s["params"][b]), (name, b)
        R.assert_matches(S[b], Sref, spread, f"{name}[{b}]")


def test_a_component_above_the_limit_is_declined(E):
    recs, g = R.hub_sketch(MAX_COMPONENT_VARS // 2 + 1)
    s = E.System(recs, len(g))
    S = np.full((1, 1, len(g)), 7.0)
    st, deg = np.full(1, 9, np.uint32), np.full(1, 5, np.uint32)
    pos = np.asarray([5], np.uint32)
    rc = E.lib().ezpz_system_param_sensitivity(s._h, g.ctypes.data, pos.ctypes.data, 1, None, 1, 1e-9, S.ctypes.data, st.ctypes.data, deg.ctypes.data)
    assert rc == ERR_INVALID_ARGUMENT and np.all(S == 7.0) and st[0] == 9 and deg[0] == 5


def test_meaning_finite_differences_of_two_solves(E):
    """(x(p + delta e_j) - x(p)) / delta on sketch150 at residual tolerance 1e-13 against S; the bar is 4 x the distance between the
    ORACLE's same finite difference and the numpy S (both share the first-order error; the margin covers the device's rounding)."""
    sysobj, s = _system(E, "sketch150")
    recs, pos, n = s["recs"], s["pos"], s["n_vars"]
    delta = 1e-6
    cfg = E.Config(max_iterations=60, residual_tolerance=1e-13)
    ocfg = O.Config(max_iterations=60, residual_tolerance=1e-13)
    p0 = recs["param"][pos].copy()  # the sketch's own dimensions: consistent with its hidden layout, so the solves reach a root
    picks = [0, len(pos) // 3, len(pos) // 2, len(pos) - 1]
    rows = np.stack([p0] + [p0 + delta * (np.arange(len(pos)) == j) for j in picks])
    x0 = np.repeat(s["start"][0][None, :], len(rows), axis=0)
    x, st, _ = sysobj.solve_batch_params(x0, pos, rows, cfg)
    print("meaning: iterations", st["iterations"].tolist(), "converged", st["converged"].tolist(), "final residual", st["final_residual_inf"].tolist())
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
        R.log(f"meaning, sketch150 parameter {j}: oracle's finite difference to the numpy S {granted / 4.0:.3e}; device's to its S {err:.3e} (granted {granted:.3e})")
        assert err <= granted, (j, err, granted)


def test_determinism_batch_size_and_place(E):
    for name in ("massive40", "sketch150", "kind:arc_length"):
        sysobj, s = _system(E, name)
        x, p = s["x"], s["params"]
        a, _ = sysobj.param_sensitivity(x, s["pos"], p, lam=s["lam"])
        b, _ = sysobj.param_sensitivity(x, s["pos"], p, lam=s["lam"])
        assert np.array_equal(a, b), name
        one, _ = sysobj.param_sensitivity(x[:1], s["pos"], p[:1], lam=s["lam"])
        assert np.array_equal(one[0], a[0]), name
        # 4096 systems (a quarter of the parameters where the list is long: S of sketch150 would be 2 GB otherwise)
        step = 4 if len(s["pos"]) > 16 else 1
        pos = s["pos"][::step]
        small, _ = sysobj.param_sensitivity(x[:1], pos, p[:1, ::step], lam=s["lam"])
        big, st = sysobj.param_sensitivity(np.tile(x[:1], (4096, 1)), pos, np.tile(p[:1, ::step], (4096, 1)), lam=s["lam"])
        assert not st.any() and np.array_equal(big, np.broadcast_to(small, big.shape)) and np.array_equal(small[0], a[0][::step]), name
        perm = np.random.default_rng(1).permutation(len(x))
        c, _ = sysobj.param_sensitivity(x[perm], s["pos"], p[perm], lam=s["lam"])
        assert np.array_equal(c, a[perm]), name


def test_zeros_are_exact_and_none_means_own_values(E):
    sysobj, s = _system(E, "massive40")
    S, _ = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"])
    Sref = np.stack([r for r, _ in R.references("massive40")])
    untouched = np.all(Sref == 0.0, axis=(0, 1))  # variables of components without a driven parameter
    assert untouched.sum() >= 4 and np.all(S[:, :, untouched] == 0.0) and not np.signbit(S[:, :, untouched]).any()
    assert np.array_equal(S == 0.0, Sref == 0.0)
    own = np.repeat(s["recs"]["param"][s["pos"]][None, :], len(s["x"]), axis=0)
    a, _ = sysobj.param_sensitivity(s["x"], s["pos"], None, lam=s["lam"])
    b, _ = sysobj.param_sensitivity(s["x"], s["pos"], own, lam=s["lam"])
    assert np.array_equal(a, b)


def test_declined_calls_leave_every_output_untouched(E):
    sysobj, s = _system(E, "kind:distance")
    L, x = E.lib(), np.ascontiguousarray(s["x"][:2])
    no_param = next(i for i in range(len(s["recs"])) if not E.constraint_has_param(s["recs"][i]))
    good = int(s["pos"][0])
    for pos, null_positions in (([len(s["recs"])], False), ([good, good], False), ([no_param], False), ([good], True)):
        pos = np.asarray(pos, np.uint32)
        S, st, deg = np.full((2, len(pos), s["n_vars"]), 7.0), np.full(2, 9, np.uint32), np.full(2, 5, np.uint32)
        rc = L.ezpz_system_param_sensitivity(sysobj._h, x.ctypes.data, None if null_positions else pos.ctypes.data, len(pos), None, 2, 1e-9,
                                             S.ctypes.data, st.ctypes.data, deg.ctypes.data)
        assert rc == ERR_INVALID_ARGUMENT and np.all(S == 7.0) and np.all(st == 9) and np.all(deg == 5), pos
    with pytest.raises(E.NonLinearSystemError):
        sysobj.param_sensitivity(x, [no_param])


def test_a_failed_pivot_marks_its_system_only(E):
    sysobj, s = _system(E, "weighted")
    x, p = s["x"], s["params"]
    good, _ = sysobj.param_sensitivity(x, s["pos"], p, lam=s["lam"])
    # a negative lambda beyond the smallest eigenvalue of JtJ, for one system: per-call lambda, so that system goes alone ...
    J = R.jacobian(R.substituted(s["recs"], s["pos"], p[1]), x[1], s["n_vars"])
    lam_bad = -(np.linalg.eigvalsh(J.T @ J)[0] * 1.5 + 1.0)
    bad, st = sysobj.param_sensitivity(x[1:2], s["pos"], p[1:2], lam=lam_bad)
    assert st[0] == 1 and np.isnan(bad).all()
    # ... and inside a batch: a system whose values are not finite fails its pivot, its neighbours keep their bits
    xx = x.copy()
    xx[2] = np.nan
    S, st = sysobj.param_sensitivity(xx, s["pos"], p, lam=s["lam"])
    assert st.tolist() == [0, 0, 1, 0] and np.isnan(S[2]).all()
    assert np.array_equal(S[[0, 1, 3]], good[[0, 1, 3]])
    # the workgroup shape: an under-determined component has a zero eigenvalue, so any negative lambda fails a pivot
    sysobj, s = _system(E, "under")
    assert sysobj.param_sensitivity_plan(s["pos"])["n_lds"] == 1
    bad, st = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=-1.0)
    assert st.all() and np.isnan(bad).all()
    # the workspace shape: lambda below minus the largest eigenvalue (every pivot's sign turns), for one system of the two
    sysobj, s = _system(E, "hub512")
    assert sysobj.param_sensitivity_plan(s["pos"])["n_workspace"] == 1
    J = R.jacobian(R.substituted(s["recs"], s["pos"], s["params"][0]), s["x"][0], s["n_vars"])
    bad, st = sysobj.param_sensitivity(s["x"][:1], s["pos"], s["params"][:1], lam=-2.0 * float(np.linalg.eigvalsh(J.T @ J)[-1]))
    assert st[0] == 1 and np.isnan(bad).all()
    S, st = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"])
    assert not st.any() and not np.isnan(S).any()


def test_device_form_on_a_stream_and_autograd(E):
    import torch

    from ezpz_amd import torch_ops

    for name in ("sketch150", "massive40", "kind:points_at_angle_deg"):
        sysobj, s = _system(E, name)
        host, _ = sysobj.param_sensitivity(s["x"], s["pos"], s["params"], lam=s["lam"])
        x, p = torch.tensor(s["x"], device="cuda"), torch.tensor(s["params"], device="cuda")
        S = torch.full(host.shape, 3.0, dtype=torch.float64, device="cuda")
        st = torch.full((len(s["x"]),), 9, dtype=torch.int32, device="cuda")
        deg = torch.full((len(s["x"]),), 9, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            sysobj.param_sensitivity_device(x.data_ptr(), s["pos"], p.data_ptr(), len(s["x"]), S.data_ptr(), st.data_ptr(), lam=s["lam"],
                                            degenerate_ptr=deg.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(S.cpu().numpy(), host) and not st.cpu().numpy().any(), name
        assert deg.cpu().numpy().tolist() == [R.degenerate_count(s["recs"], s["x"][b], s["pos"], s["params"][b]) for b in range(len(s["x"]))], name
        # autograd: grad_params = S grad_x with the numpy reference's S at the forward's answer
        pt = p.clone().requires_grad_(True)
        xs = torch_ops.solve_params(sysobj, x, s["pos"], pt, lam=s["lam"])
        grad_x = torch.tensor(np.random.default_rng(2).uniform(-1.0, 1.0, host.shape[::2]), device="cuda")
        xs.backward(grad_x)
        got = pt.grad.cpu().numpy()
        gx = grad_x.cpu().numpy()
        xf = xs.detach().cpu().numpy()
        for b in range(len(xf)):
            Sref, spread = R.reference(s["recs"], s["n_vars"], xf[b], s["pos"], s["params"][b], s["lam"])
            # the bar of the comparison above, on every entry of grad_params: max(1e-10, 20 x spread) * max(1, |S_j|_inf)
            scale = np.maximum(1.0, np.abs(Sref).max(axis=1))
            err = float((np.abs(got[b] - Sref @ gx[b]) / scale).max())
            print("autograd", name, b, err, R.bar(spread))
            R.log(f"autograd {name}[{b}]: grad_params against S_ref grad_x: largest error {err:.3e} | bar granted {R.bar(spread):.3e} (spread {spread:.3e})")
            assert err <= R.bar(spread), (name, b, err, R.bar(spread))
