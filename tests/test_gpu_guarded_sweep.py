"""Guarded sweeps (ezpz_system_sweep_guarded): the sweep with step control in the team that owns it.  Bit for bit, every output,
against the rule run over System.solve_batch_params (guarded_sweep_common.params_entry_rule: the definition) -- on the three
shapes the device form serves, with sweeps of one wavefront and of one workgroup taking different numbers of attempts, for a
team's second sweep, with the driven values staged in LDS and read from global memory, with the workspace in global memory,
with rejects from non-convergence and with max_attempts cutting a step short; the crank against the oracle's tables; the plain
sweep; continuation; the declined routes; the device form and the argument errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from guarded_sweep_common import (CRANK_MAX_MOVE, CRANK_PLAIN_TABLE, CRANK_PLAIN_TARGETS, CRANK_TABLE, CRANK_TARGETS, assert_same_outputs,
                                  crank, crank_params, guard_table, guarded, guarded_shapes, oracle_rule, params_entry_rule, walk_inputs)
from sensitivity import assert_batch_matches_oracle
from sweep_common import chain, driven_walk, shapes, substituted

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
NAMES = ["sub-wavefront teams", "barrier workgroup", "record walk"]


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _system(E, name):
    recs, g, team, mode = guarded_shapes(E)[name]
    s = E.System(recs, len(g), team_size=team)
    assert s.info()["team_mode"] == mode, (name, s.info())
    return s, recs, g


def _both(s, pos, x0, params0, params, what, **kw):
    got, want = guarded(s, pos, x0, params0, params, **kw), params_entry_rule(s, pos, x0, params0, params, **kw)
    assert_same_outputs(got, want, what)
    return got


def _run_walks(E, name, say=print):
    """One shape's walk under four policies; every output bit for bit the rule's.  (Shared with the child process that reads the
    driven values from global memory.)"""
    s, recs, g = _system(E, name)
    sweeps, steps = (96, 5) if name == "sub-wavefront teams" else (12, 4)
    pos, params0, params, x0, max_move = walk_inputs(E, name, recs, g, sweeps, steps, 71)
    plan = s.sweep_guarded_plan(pos)
    assert plan["route_name"] == name and plan["in_kernel"] == 1, plan
    # the defaults with a displacement bound: rejects for the distance moved, attempts that differ from sweep to sweep
    got = _both(s, pos, x0, params0, params, name, max_move=max_move, warn_cap=8)
    att = got["guard"]["attempts"]
    say(name, plan, "attempts", np.bincount(att.ravel()).tolist(), "reached 1 on", float((got["guard"]["reached"] == 1).mean()))
    per_wave = max(1, 64 // s.info()["team_size"]) if name == "sub-wavefront teams" else 1
    assert any(len(set(att[k, :max(per_wave, 2)].tolist())) > 1 for k in range(steps)), (name, att[:, :max(per_wave, 2)])
    assert any(len(set(att[k].tolist())) > 1 for k in range(steps)), (name, att)
    assert (got["guard"]["accepted"] < att).any() and (got["guard"]["reached"] == 1).mean() >= 0.9
    # few iterations: rejects come from solves that do not converge (two: hardly a solve converges, on any shape, and the sweeps
    # hold on to where they started; three: the record walk's sweeps are a mixture)
    for iterations in (2, 3):
        cfg = E.Config().with_max_iterations(iterations)
        few = _both(s, pos, x0, params0, params, name + ", %d iterations" % iterations, config=cfg, warn_cap=8)
        if iterations == 2:
            assert (few["status"]["converged"] == 0).any() and (few["guard"]["attempts"] > 1).any() and (few["guard"]["accepted"] == 0).any(), name
    # three attempts per step: steps that are cut short behind an accept, and the next step catching up
    cut = _both(s, pos, x0, params0, params, name + ", 3 attempts", max_move=max_move, max_attempts=3, warn_cap=8)
    gs = cut["guard"]
    assert ((gs["attempts"] == 3) & (gs["accepted"] >= 1) & (gs["reached"] < 1)).any(), (name, gs)
    # no halving at all, and a fraction given up after one
    _both(s, pos, x0, params0, params, name + ", no halvings", max_move=max_move, max_halvings=0)
    _both(s, pos, x0, params0, params, name + ", one halving", max_move=max_move, max_halvings=1)
    return plan


@pytest.mark.parametrize("name", NAMES)
def test_same_bits_as_the_rule_over_the_params_entry(E, name):
    plan = _run_walks(E, name)
    assert plan["params_in_lds"] == 1, plan


def _child_main():
    """In a child process (EZPZ_PARAMS_LDS is read once per process)."""
    import ezpz_amd as E

    for name in NAMES:
        plan = _run_walks(E, name, say=lambda *a: None)
        print("same bits:", name, "params_in_lds", plan["params_in_lds"], flush=True)


def test_driven_values_read_from_global_memory(E):
    """EZPZ_PARAMS_LDS=0: the team forms p_u in the params_reached row it owns and every sweep over the constraints reads it there."""
    env = dict(os.environ, EZPZ_DEBUG="params", EZPZ_AMD_NO_BUILD="1", EZPZ_PARAMS_LDS="0")
    here = os.path.dirname(os.path.abspath(__file__))
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    run = subprocess.run([sys.executable, "-c", "import test_gpu_guarded_sweep as t; t._child_main()"], cwd=here, env=env,
                         capture_output=True, text=True, timeout=600)
    lines = [l for l in run.stderr.splitlines() if l.startswith("[ezpz guarded sweep]")]
    print(run.stdout, "\n".join(sorted(set(lines))))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stdout.count("same bits:") == 3 and run.stdout.count("params_in_lds 0") == 3 and lines
    assert all("read from global memory" in l for l in lines), lines


@pytest.mark.parametrize("name", NAMES)
def test_a_teams_second_sweep(E, name):
    """More sweeps than the launch has teams (test_gpu_sweep.py's count): what a team carries from a finished sweep into its next
    one -- the step's state, the gather flag, the driven values -- would show."""
    s, recs, g = _system(E, name)
    info = s.info()
    teams = _cus() * 32 * (256 // info["team_size"]) if info["team_mode"] == 0 else _cus() * 32 * 8
    sweeps = teams + 64
    pos, p0_8, p8, x8, max_move = walk_inputs(E, name, recs, g, 8, 2, 33)
    params = np.ascontiguousarray(np.tile(p8, (1, sweeps // 8, 1)))
    params0 = np.ascontiguousarray(np.tile(p0_8, (sweeps // 8, 1)))
    x0 = x8[0][None, :] + np.random.default_rng(34).uniform(-0.01, 0.01, (sweeps, len(g)))
    got = _both(s, pos, x0, params0, params, name, max_move=max_move, max_attempts=4)
    assert len(set(got["guard"]["attempts"][1].tolist())) > 1


def test_workspace_in_global_memory(E):
    recs, g = chain(2000)
    s = E.System(recs, len(g), team_size=256)
    info = s.info()
    assert info["workspace_in_lds"] == 0 and info["grid_workgroups"] == 1 and info["team_mode"] == 2, info
    cfg = E.Config().with_max_iterations(6)
    solved, st, _ = s.solve_batch(g[None, :])  # (the walk starts where the records' own values are solved: by the device itself)
    assert st["converged"][0] == 1
    for n_drive, in_lds in ((None, 0), (1, 1)):
        # (every link driven: its 16 KB of values beside 50 KB of LDS would cost the CU a workgroup, so they are read from global
        # memory, and the far end of the chain moves by the sum of 2000 changes -- further than max_move until the step is cut)
        pos, params, x0 = driven_walk(E, recs, solved[0], 6, 2, 35, amplitude=0.1, jitter=1e-3, n_drive=n_drive)
        plan = s.sweep_guarded_plan(pos)
        assert plan["route_name"] == "barrier workgroup" and plan["in_kernel"] == 1 and plan["params_in_lds"] == in_lds, plan
        params0 = np.ascontiguousarray(np.tile(recs["param"][pos].astype(np.float64), (6, 1)))
        got = _both(s, pos, x0, params0, params, n_drive, config=cfg, max_attempts=6, max_move=0.5)
        gs = got["guard"]
        print(n_drive, "attempts", gs["attempts"].tolist(), "accepted", gs["accepted"].tolist())
        assert (gs["accepted"] >= 1).any()
        if n_drive is None:
            assert (gs["accepted"] < gs["attempts"]).any()


def test_the_crank_takes_the_oracles_decisions(E):
    recs, pos, x0, params0 = crank()
    s = E.System(recs, 4, team_size=E.TEAM_AUTO_LISTS)
    assert s.info()["team_mode"] == 0 and s.sweep_guarded_plan(pos)["in_kernel"] == 1
    params = crank_params(CRANK_TARGETS)
    got = _both(s, pos, x0, params0, params, "crank", max_move=CRANK_MAX_MOVE)
    xo, go, ro = oracle_rule(recs, pos, x0, params0, params, max_move=CRANK_MAX_MOVE)
    table = guard_table(got["guard"], got["params_reached"])
    print("crank:", table)
    assert got["guard"].tobytes() == go.tobytes() and np.array_equal(got["params_reached"], ro), (table, guard_table(go, ro))
    assert [(r, a, c) for r, a, c, _ in table] == [(r, a, c) for r, a, c, _ in CRANK_TABLE]
    for k in range(len(CRANK_TARGETS)):  # (each row an accepted, converged answer at the value reached: test_gpu_sweep.py's bar)
        start = x0[0] if k == 0 else got["x"][k - 1, 0]
        assert_batch_matches_oracle(substituted(recs, pos, got["params_reached"][k, 0]), start[None, :], got["x"][k], np.zeros(1), np.ones(1),
                                    None, oracle_result=(xo[k], np.zeros(1), np.ones(1)), what="crank[%d]" % k, check_iterations=False)
    plain = _both(s, pos, x0, params0, crank_params(CRANK_PLAIN_TARGETS), "crank, plain", max_halvings=0, max_move=0.0)
    assert [(float(r), int(a)) for r, a in zip(plain["guard"]["reached"][:, 0], plain["guard"]["attempts"][:, 0])] == CRANK_PLAIN_TABLE
    assert np.array_equal(plain["x"][1], plain["x"][0]) and np.allclose(plain["x"][1, 0, 2:], [0.5, 0.866], atol=1e-3)


@pytest.mark.parametrize("name", NAMES)
def test_without_halvings_and_bound_it_is_the_plain_sweep(E, name):
    s, recs, g = _system(E, name)
    pos, params0, params, x0, _ = walk_inputs(E, name, recs, g, 12, 4, 52)
    params = np.ascontiguousarray(params0[None] + 0.02 * (params - params0[None]))  # (a walk every step of which converges)
    log = np.zeros((4, 12, 8), dtype=np.uint64)
    x, st, mask = s.sweep_params(x0, pos, params, want_mask=True, warn_log=log)
    assert np.all(st["converged"] == 1) and np.all(st["n_unsatisfied"] == 0)
    got = guarded(s, pos, x0, params0, params, warn_cap=8, max_halvings=0, max_move=0.0)
    assert np.array_equal(got["x"], x) and got["status"].tobytes() == st.tobytes() and np.array_equal(got["mask"], mask)
    assert np.array_equal(np.sort(got["log"], axis=2), np.sort(log, axis=2))
    assert np.all(got["guard"]["reached"] == 1.0) and np.all(got["guard"]["attempts"] == 1) and np.all(got["guard"]["accepted"] == 1)
    assert np.array_equal(got["params_reached"], params)


@pytest.mark.parametrize("name", NAMES)
def test_continuation(E, name):
    """2K steps are K steps and K more from (x_out[K - 1], params_reached[K - 1])."""
    s, recs, g = _system(E, name)
    K = 3
    pos, params0, params, x0, max_move = walk_inputs(E, name, recs, g, 16, 2 * K, 53)
    kw = dict(max_move=max_move, max_attempts=5, warn_cap=4)
    whole = guarded(s, pos, x0, params0, params, **kw)
    first = guarded(s, pos, x0, params0, np.ascontiguousarray(params[:K]), **kw)
    second = guarded(s, pos, first["x"][K - 1], first["params_reached"][K - 1], np.ascontiguousarray(params[K:]), **kw)
    joined = {key: np.concatenate([first[key], second[key]]) for key in whole}
    assert_same_outputs(joined, whole, name)


def _device_call(E, s, torch, pos, x0, params0, params, stream, guard=None, fill=None):
    """The device form on `stream`; returns (error code or None, the outputs as numpy arrays)."""
    from ezpz_amd._lib import GUARD_STEP_DTYPE, STATUS_DTYPE

    steps, batch, k = params.shape
    n, n_cs = x0.shape[1], len(s.records)
    with torch.cuda.stream(stream):
        xin, p0, pd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x0, params0, params))
        byte = 0 if fill is None else fill
        out = {"x": (steps * batch * n * 8, np.float64), "status": (steps * batch * STATUS_DTYPE.itemsize, STATUS_DTYPE),
               "guard": (steps * batch * 16, GUARD_STEP_DTYPE), "params_reached": (steps * batch * k * 8, np.float64),
               "mask": (steps * batch * n_cs, np.uint8)}
        dev = {key: torch.full((size,), byte, dtype=torch.uint8, device="cuda") for key, (size, _) in out.items()}
        code = None
        try:
            s.sweep_guarded_device(xin.data_ptr(), pos, p0.data_ptr(), pd.data_ptr(), steps, batch, dev["x"].data_ptr(),
                                   dev["status"].data_ptr(), dev["guard"].data_ptr(), dev["params_reached"].data_ptr(),
                                   mask_ptr=dev["mask"].data_ptr(), stream=stream.cuda_stream, guard=guard)
        except E.NonLinearSystemError as e:
            code = e.code
    stream.synchronize()
    return code, {key: dev[key].cpu().numpy().view(out[key][1]) for key in out}


def test_declined_routes(E):
    import torch

    stream = torch.cuda.Stream()
    cases = []
    for name, recs, g, team, mode in shapes(E):
        if name in ("interpreter", "partitioned workgroup"):
            cases.append((name, recs, np.asarray(g, dtype=np.float64), team, mode, False))
    crecs, cg = chain(40)
    cases.append(("fronts", crecs, cg, E.TEAM_FRONTS, 5, True))
    for name, recs, g, team, mode, fronts in cases:
        s = E.System(recs, len(g), team_size=team)
        assert s.info()["team_mode"] == mode, (name, s.info())
        if fronts:
            s.set_params_route("fronts")
        pos, params, x0 = driven_walk(E, recs, g, 4, 2, 81, n_drive=8)
        params0 = np.ascontiguousarray(np.tile(recs["param"][pos].astype(np.float64), (4, 1)))
        plan = s.sweep_guarded_plan(pos)
        assert plan["in_kernel"] == 0 and plan["route_name"] == name, plan
        code, outs = _device_call(E, s, torch, pos, x0, params0, params, stream, fill=0xAB)
        assert code == ERR_INVALID_ARGUMENT, (name, code)
        for key, a in outs.items():
            assert np.all(a.view(np.uint8) == 0xAB), (name, key)
        if not fronts:  # the host form runs the rule as rounds of params calls: the same bits
            got = _both(s, pos, x0, params0, params, name + ", host form", max_move=0.2, max_attempts=4, warn_cap=4)
            print(name, "attempts", got["guard"]["attempts"].tolist())


def test_device_form_on_a_stream_and_argument_errors(E):
    import torch

    from ezpz_amd._lib import CGuardConfig, GUARD_STEP_DTYPE, STATUS_DTYPE

    name = "sub-wavefront teams"
    s, recs, g = _system(E, name)
    pos, params0, params, x0, max_move = walk_inputs(E, name, recs, g, 32, 4, 91)
    want = guarded(s, pos, x0, params0, params, max_move=max_move)
    stream = torch.cuda.Stream()
    code, outs = _device_call(E, s, torch, pos, x0, params0, params, stream, guard=E.GuardConfig(max_move=max_move))
    assert code is None
    for key in ("x", "status", "guard", "params_reached", "mask"):
        assert outs[key].tobytes() == want[key].tobytes(), key
    # ---- argument errors of the host form: EZPZ_ERR_INVALID_ARGUMENT, nothing written --------------------------------------------
    steps, batch, k = params.shape
    n = x0.shape[1]
    x = np.full((steps, batch, n), -777.0)
    st = np.full(steps * batch * STATUS_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    gs = np.full(steps * batch * GUARD_STEP_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    reached = np.full((steps, batch, k), -777.0)
    cfg = E.Config()._c()
    ok = dict(positions=pos, n_param=k, params0=params0, params=params, guard_cfg=CGuardConfig(4, 12, 0.0), guard=gs, reached=reached)

    def call(**change):
        a = {**ok, **change}
        ptr = lambda v: None if v is None else v.ctypes.data  # noqa: E731
        return E.lib().ezpz_system_sweep_guarded(s._h, x0.ctypes.data, ptr(a["positions"]), a["n_param"], ptr(a["params0"]), ptr(a["params"]),
                                                 steps, batch, C.byref(cfg), None if a["guard_cfg"] is None else C.byref(a["guard_cfg"]),
                                                 x.ctypes.data, st.ctypes.data, ptr(a["guard"]), ptr(a["reached"]), None, None, 0)

    def with_first(p):
        q = pos.copy()
        q[0] = p
        return q

    assert not E.constraint_has_param(recs[2]) and list(pos) == [0, 1, 3]  # (position 2, the horizontal, has no parameter)
    bad = [dict(n_param=0), dict(params0=None), dict(guard=None), dict(reached=None), dict(params=None), dict(positions=None),
           dict(guard_cfg=CGuardConfig(21, 12, 0.0)), dict(guard_cfg=CGuardConfig(4, 0, 0.0)), dict(guard_cfg=CGuardConfig(4, 12, float("inf"))),
           dict(guard_cfg=CGuardConfig(4, 12, float("nan"))), dict(positions=with_first(len(recs))), dict(positions=with_first(1)),
           dict(positions=with_first(2))]
    for change in bad:
        assert call(**change) == ERR_INVALID_ARGUMENT, change
        assert np.all(x == -777.0) and np.all(st == 0xAB) and np.all(gs == 0xAB) and np.all(reached == -777.0), change
    assert call(guard_cfg=None) == 0  # (NULL: the defaults)
    assert np.array_equal(x, guarded(s, pos, x0, params0, params)["x"])
    with pytest.raises(ValueError):
        s.sweep_guarded(x0, pos, params0[:1], params)
    with pytest.raises(ValueError):
        s.sweep_guarded(x0, [], None, np.zeros((2, batch, 0)))
