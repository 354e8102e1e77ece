"""Batch solves with per-system constraint parameters (ezpz_system_solve_batch_params): against the oracle run once per system on
the substituted constraints, bit for bit against systems rebuilt with the parameters baked in on every launch shape the entry
reaches, and the entry's semantics, errors and device form.  Bars: tests/test_gpu_parity.py's 1e-6 and tests/sensitivity.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from oracle import textual as T
from sensitivity import assert_batch_matches_oracle, residual_inf

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


P0, P1, P2, P3 = (0, 1), (2, 3), (4, 5), (6, 7)


def _fix(values):
    return [O.fixed(i, float(v)) for i, v in values]


# kind -> (constraints, guesses, [(position, nominal, half-width of the draw)]): small, determined, well-conditioned systems in
# which the constraint under test decides at least one coordinate
def _cases():
    c = {}
    c["distance"] = (_fix([(0, 0), (1, 0)]) + [O.horizontal(P0, P1), O.distance(P0, P1, 2.0)], [0, 0, 2.1, 0.1], [(3, 2.0, 0.5)])
    c["axis_distances_and_fixed"] = (_fix([(0, 1), (1, -1)]) + [O.vertical_distance(P1, P0, 1.5), O.horizontal_distance(P1, P0, 2.5)],
                                     [1, -1, 3, 1], [(0, 1.0, 0.5), (1, -1.0, 0.5), (2, 1.5, 1.0), (3, 2.5, 1.0)])
    c["circle_radius"] = (_fix([(0, 0), (1, 1)]) + [O.circle_radius(P0, 2, 1.5)], [0, 1, 1.0], [(2, 1.5, 1.0)])
    c["arc_radius"] = (_fix([(0, 0), (1, 0), (3, 0), (4, 0)]) + [O.arc_radius(P0, P1, P2, 2.0)], [0, 0, 2.1, 0, 0, 1.9], [(4, 2.0, 0.5)])
    line = _fix([(2, 0), (3, 0), (4, 4), (5, 0)])
    c["point_line_distance"] = (line + _fix([(0, 1)]) + [O.point_line_distance(P0, P1, P2, 1.5)], [1, 1.4, 0, 0, 4, 0], [(5, 1.5, 1.0)])
    c["vertical_point_line_distance"] = (line + _fix([(0, 1)]) + [O.vertical_point_line_distance(P0, P1, P2, 1.5)],
                                         [1, 1.4, 0, 0, 4, 0], [(5, 1.5, 1.0)])
    c["horizontal_point_line_distance"] = (_fix([(2, 0), (3, 0), (4, 0), (5, 4), (1, 1)]) + [O.horizontal_point_line_distance(P0, P1, P2, 1.5)],
                                           [1.4, 1, 0, 0, 0, 4], [(5, 1.5, 1.0)])
    c["arc_length"] = (_fix([(0, 0), (1, 0), (2, 2), (3, 0)]) + [O.arc_length(P0, P1, P2, 2.0)], [0, 0, 2, 0, 1.1, 1.7], [(4, 2.0, 0.4)])
    for unit, nominal, half in (("deg", 30.0, 15.0), ("rad", 0.5, 0.25)):
        c["lines_at_angle_" + unit] = (_fix([(0, 0), (1, 0), (2, 2), (3, 0), (4, 0), (5, 0)]) +
                                       [O.distance(P2, P3, 2.0), O.lines_at_angle(P0, P1, P2, P3, (unit, nominal))],
                                       [0, 0, 2, 0, 0, 0, 1.7, 1.0], [(7, nominal, half)])
        c["arc_angle_" + unit] = (_fix([(0, 0), (1, 0), (2, 2), (3, 0)]) + [O.distance(P0, P2, 2.0), O.arc_angle(P0, P1, P2, (unit, nominal))],
                                  [0, 0, 2, 0, 1.7, 1.0], [(5, nominal, half)])
        c["points_at_angle_" + unit] = (_fix([(0, 0), (1, 0), (2, 2), (3, 0)]) + [O.points_at_angle(P0, P1, P2, (unit, nominal))],
                                        [0, 0, 2, 0, 1.7, 1.0], [(4, nominal, half)])
    return {k: (O.stack(cons), np.asarray(g, dtype=float), drv) for k, (cons, g, drv) in c.items()}


CASES = _cases()


def _draw(recs, g, driven, batch, seed):
    rng = np.random.default_rng(seed)
    pos = np.asarray([p for p, _, _ in driven], dtype=np.uint32)
    params = np.stack([rng.uniform(nom - half, nom + half, batch) for _, nom, half in driven], axis=1)
    x0 = g[None, :] + rng.uniform(-0.05, 0.05, (batch, len(g)))
    return pos, params, x0


def _substituted(recs, pos, row):
    r = recs.copy()
    r["param"][pos] = row
    return r


def _oracle_each(recs, pos, params, x0, cfg=None):
    """The oracle once per system on the substituted constraints: values, iterations, converged, n_unsatisfied, mask."""
    xo, it, conv, nun, mask = [], [], [], [], np.zeros((len(x0), len(recs)), np.uint8)
    for b in range(len(x0)):
        r = _substituted(recs, pos, params[b])
        rc, x, i, c, n = O.solve_batch(r, x0[b:b + 1], cfg, linsolve=O.LINSOLVE_SPARSE)
        assert rc == 0
        xo.append(x[0]), it.append(int(i[0])), conv.append(int(c[0])), nun.append(int(n[0]))
        mask[b, sorted(residual_inf(r, x[0])[1])] = 1
    return np.stack(xo), np.asarray(it), np.asarray(conv), np.asarray(nun), mask


def _check_against_oracle(recs, pos, params, x0, x, st, mask, what, cfg=None):
    xo, it, conv, nun, mo = _oracle_each(recs, pos, params, x0, cfg)
    print(what, "oracle converged on", int(conv.sum()), "of", len(conv), "| largest relative coordinate error",
          float(np.nanmax(np.abs(x - xo) / np.maximum(1.0, np.abs(xo)))))
    assert conv.mean() >= 0.9, what  # (the draw ranges are meant to keep the oracle itself converging)
    assert np.array_equal(st["iterations"], it) and np.array_equal(st["converged"], conv), what
    assert np.array_equal(st["n_unsatisfied"], nun) and np.array_equal(mask, mo), what
    assert np.array_equal(mo.sum(axis=1), nun), what
    for b in range(len(x0)):  # every system, converged or not: 1e-6, or the oracle's own measured sensitivity
        assert_batch_matches_oracle(_substituted(recs, pos, params[b]), x0[b:b + 1], x[b:b + 1], st["iterations"][b:b + 1],
                                    st["converged"][b:b + 1], cfg, oracle_result=(xo[b:b + 1], it[b:b + 1], conv[b:b + 1]),
                                    what=f"{what}[{b}]")


@pytest.mark.parametrize("name", sorted(CASES))
def test_kind_by_kind_against_the_oracle(E, name):
    recs, g, driven = CASES[name]
    pos, params, x0 = _draw(recs, g, driven, 64, 7)
    s = E.System(recs, len(g), team_size=E.TEAM_AUTO_LISTS)
    assert s.info()["team_mode"] == 0
    x, st, mask = s.solve_batch_params(x0, pos, params, want_mask=True)
    _check_against_oracle(recs, pos, params, x0, x, st, mask, name)


def _block_draw(ref, recs, pos, batch, seed):
    rng = np.random.default_rng(seed)
    params = recs["param"][pos][None, :] + rng.uniform(-0.5, 0.5, (batch, len(pos)))
    x0 = ref.guesses[None, :] + rng.uniform(-0.25, 0.25, (batch, ref.num_vars))
    return params, x0


def test_linear_block_system_bit_for_bit(E):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_cases", "massive_parallel_system", "problem.md")
    ref = T.load(open(path).read())
    recs = O.stack(ref.constraints)
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    assert len(pos) > 0
    params, x0 = _block_draw(ref, recs, pos, 64, 3)
    s = E.System(recs, ref.num_vars)
    assert s.info()["team_mode"] == 3
    x, st, mask = s.solve_batch_params(x0, pos, params, want_mask=True)
    xo, it, conv, nun, mo = _oracle_each(recs, pos, params, x0)
    assert np.array_equal(x, xo) and np.array_equal(st["iterations"], it) and np.array_equal(st["converged"], conv)
    assert np.array_equal(st["n_unsatisfied"], nun) and np.array_equal(mask, mo)


def _chain(n_pts):
    cons = [O.fixed(0, 0.0), O.fixed(1, 0.0)]
    guesses = [0.0, 0.0]
    for k in range(1, n_pts):
        a, b = (2 * (k - 1), 2 * k - 1), (2 * k, 2 * k + 1)
        cons.append(O.distance(a, b, 1.0))
        cons.append(O.horizontal(a, b) if k % 2 else O.vertical(a, b))
        guesses += [0.55 * k + 0.1, 0.45 * k - 0.1]
    return O.stack(cons), np.asarray(guesses)


def _shapes(E):
    """(name, records, guesses, team_size, expected team_mode) for every launch shape the entry reaches."""
    recs, g, _ = CASES["distance"]
    out = [("sub-wavefront teams", recs, g, E.TEAM_AUTO_LISTS, 0)]
    ref = T.load(T.gen_big_problem(64))
    brecs = O.stack(ref.constraints)
    out.append(("partitioned workgroup", brecs, ref.guesses, E.TEAM_AUTO_LISTS, 1))
    out.append(("interpreter", brecs, ref.guesses, 0, 3))
    crecs, cg = _chain(40)
    out.append(("barrier workgroup", crecs, cg, 256, 2))
    # one connected sketch whose linear solve is a record walk (the sketch of smoke(): points tied by a distance and a horizontal distance)
    rng = np.random.default_rng(0)
    npts = 70
    true = np.cumsum(rng.uniform(0.5, 2.0, (npts, 2)), axis=0)
    true[0] = 0.0
    cons = [O.fixed(0, 0.0), O.fixed(1, 0.0)]
    for i in range(1, npts):
        j = max(0, i - 2)
        cons += [O.distance((2 * i, 2 * i + 1), (2 * i - 2, 2 * i - 1), float(np.hypot(*(true[i] - true[i - 1])))),
                 O.horizontal_distance((2 * i, 2 * i + 1), (2 * j, 2 * j + 1), float(true[i][0] - true[j][0]))]
    out.append(("record walk", O.stack(cons), true.reshape(-1), E.TEAM_LATENCY_RECORDS, 4))
    return out


def _driven_draw(E, recs, g, batch, seed):
    rng = np.random.default_rng(seed)
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    params = recs["param"][pos][None, :] + rng.uniform(-0.1, 0.1, (batch, len(pos)))
    x0 = g[None, :] + rng.uniform(-0.03, 0.03, (batch, len(g)))
    return pos, params, x0


def test_same_bits_as_a_rebuilt_system_and_identity(E):
    for name, recs, g, team, mode in _shapes(E):
        s = E.System(recs, len(g), team_size=team)
        assert s.info()["team_mode"] == mode, (name, s.info())
        pos, params, x0 = _driven_draw(E, recs, g, 8, 21)
        x, st, mask = s.solve_batch_params(x0, pos, params, want_mask=True)
        for b in range(8):
            fresh = E.System(_substituted(recs, pos, params[b]), len(g), team_size=team)
            assert fresh.info()["team_mode"] == mode
            xf, stf, mf = fresh.solve_batch(x0[b:b + 1], want_mask=True)
            assert np.array_equal(x[b], xf[0]) and st[b] == stf[0] and np.array_equal(mask[b], mf[0]), (name, b)
        # identity: the system's own parameters, and no parameters at all, are solve_batch on the same route
        xp, stp, mp = s.solve_batch(x0, want_mask=True)
        own = np.repeat(recs["param"][pos][None, :], 8, axis=0)
        for xi, sti, mi in (s.solve_batch_params(x0, pos, own, want_mask=True),
                            s.solve_batch_params(x0, [], np.zeros((8, 0)), want_mask=True)):
            assert np.array_equal(xi, xp) and np.array_equal(sti, stp) and np.array_equal(mi, mp), name
        # a permuted list with its columns, and another list right after, on the same system
        perm = np.random.default_rng(5).permutation(len(pos))
        xq, stq, mq = s.solve_batch_params(x0, pos[perm], params[:, perm], want_mask=True)
        assert np.array_equal(xq, x) and np.array_equal(stq, st) and np.array_equal(mq, mask), name
        half = pos[: max(1, len(pos) // 2)]
        xh, sth, _ = s.solve_batch_params(x0, half, params[:, : len(half)])
        fresh = E.System(_substituted(recs, half, params[0, : len(half)]), len(g), team_size=team)
        xf, stf, _ = fresh.solve_batch(x0[:1])
        assert np.array_equal(xh[0], xf[0]) and sth[0] == stf[0], name
        x2, st2, _ = s.solve_batch_params(x0, pos, params)
        assert np.array_equal(x2, x) and np.array_equal(st2, st), name


def _rebuilt_check(E, name, s, recs, g, team, batch, cfg=None, chunk=2048, n_drive=None):
    """A call of `batch` systems whose parameters repeat with period 8 (their guesses all differ) against the 8 systems rebuilt
    with those parameters, each solving its share in pieces of at most `chunk` systems: values, statuses and masks bit for bit."""
    pos, p8, _ = _driven_draw(E, recs, g, 8, 33)
    if n_drive is not None:  # (only some of the parametrised constraints, spread over the list)
        keep = np.linspace(0, len(pos) - 1, n_drive).astype(int)
        pos, p8 = pos[keep], p8[:, keep]
    assert batch % 8 == 0
    params = np.tile(p8, (batch // 8, 1))
    x0 = g[None, :] + np.random.default_rng(34).uniform(-0.03, 0.03, (batch, len(g)))
    x, st, mask = s.solve_batch_params(x0, pos, params, config=cfg, want_mask=True)
    for b in range(8):
        fresh = E.System(_substituted(recs, pos, p8[b]), len(g), team_size=team)
        mine = np.arange(b, batch, 8)
        for k in range(0, len(mine), chunk):
            idx = mine[k:k + chunk]
            xf, stf, mf = fresh.solve_batch(x0[idx], cfg, want_mask=True)
            assert np.array_equal(x[idx], xf, equal_nan=True) and np.array_equal(st[idx], stf) and np.array_equal(mask[idx], mf), (name, b, k)


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def test_teams_that_solve_several_systems_in_a_launch(E):
    """More systems than the launch has teams, a different parameter set from one system of a team to its next: the copy of a
    system's values in LDS (two copies, by parity, on the partitioned workgroup) is replaced between systems without a team ever
    evaluating with its previous system's.  The launches' grids (launch.hip, comp.hip): at most 32 x 8 workgroups per CU of one
    system each; 32 workgroups per CU of 256 / team_size teams each for sub-wavefront teams."""
    cus = _cus()
    for name, recs, g, team, mode in _shapes(E):
        s = E.System(recs, len(g), team_size=team)
        info = s.info()
        assert info["team_mode"] == mode, (name, info)
        teams = cus * 32 * (256 // info["team_size"]) if mode == 0 else cus * 32 * 8
        _rebuilt_check(E, name, s, recs, g, team, teams + 8192)


def test_workspace_in_global_memory(E):
    """A connected system too large for the LDS, on one barrier workgroup with its workspace in global memory: same bits as the
    rebuilt systems -- 4 systems, and more systems than the launch has workgroups (2 x 8 per CU)."""
    recs, g = _chain(2000)
    s = E.System(recs, len(g), team_size=256)
    info = s.info()
    assert info["workspace_in_lds"] == 0 and info["grid_workgroups"] == 1 and info["team_mode"] == 2, info
    cfg = E.Config().with_max_iterations(3)
    _rebuilt_check(E, "global workspace", s, recs, g, 256, 8, cfg)
    _rebuilt_check(E, "global workspace, several systems per workgroup", s, recs, g, 256, _cus() * 16 + 64, cfg, chunk=1024)


def test_grid_team_is_declined(E):
    """A system that one solve spreads over several workgroups: EZPZ_ERR_INVALID_ARGUMENT, nothing written."""
    lad = T.load(T.gen_big_problem(12000))
    recs = O.stack(lad.constraints)
    s = E.System(recs, lad.num_vars)
    assert s.info()["grid_workgroups"] > 1, s.info()
    pos, params, x0 = _driven_draw(E, recs, lad.guesses, 2, 2)
    _assert_declined(E, s, x0, pos, params)
    x, st, _ = s.solve_batch(x0)  # (the plain entry serves it)
    assert np.all(st["converged"] == 1)


def _child_main():
    """In a child process (the form is chosen once per process, from the environment): every list-walk shape against rebuilt systems."""
    import ezpz_amd as E

    for name, recs, g, team, mode in _shapes(E):
        if mode == 3:
            continue
        s = E.System(recs, len(g), team_size=team)
        assert s.info()["team_mode"] == mode, (name, s.info())
        _rebuilt_check(E, name, s, recs, g, team, 16)
        if mode == 1:
            # 16 driven values: few enough for the partitioned workgroup's two copies to be staged beside its state -- with more
            # systems than the launch has workgroups, so that its wavefronts pass from one copy to the other
            _rebuilt_check(E, name, s, recs, g, team, int(os.environ["EZPZ_TEST_CUS"]) * 256 + 8192, n_drive=16)
        print("same bits:", name, flush=True)


@pytest.mark.parametrize("staged", [False, True])
def test_values_read_from_global_memory_and_staged_in_lds(E, staged):
    """EZPZ_PARAMS_LDS=0: no team stages its system's values, every sweep reads them where the caller left them -- same bits.  And
    without it every shape stages them, the partitioned workgroup's two copies included (EZPZ_DEBUG=params says which form each launch took)."""
    env = dict(os.environ, EZPZ_DEBUG="params", EZPZ_AMD_NO_BUILD="1", EZPZ_TEST_CUS=str(_cus()))
    env.pop("EZPZ_PARAMS_LDS", None)
    if not staged:
        env["EZPZ_PARAMS_LDS"] = "0"
    here = os.path.dirname(os.path.abspath(__file__))
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    run = subprocess.run([sys.executable, "-c", "import test_gpu_params as t; t._child_main()"], cwd=here, env=env, capture_output=True,
                         text=True, timeout=600)
    lines = [l for l in run.stderr.splitlines() if l.startswith("[ezpz params]")]
    print(run.stdout, "\n".join(sorted(set(lines))))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stdout.count("same bits:") == 4 and lines
    if staged:
        for mode in (0, 1, 2, 4):  # every list-walk shape stages at least one of its calls
            assert any("staged in LDS" in l and "team mode %d" % mode in l for l in lines), (mode, lines)
    else:
        assert all("read from global memory" in l for l in lines), lines


def test_undriven_keep_their_values_and_conflicts_are_reported(E):
    recs, g, _ = CASES["axis_distances_and_fixed"]
    extra = O.stack(list(recs) + [O.vertical_distance(P1, P0, 1.5)])  # agrees with constraint 2 as created, not once it is driven
    s = E.System(extra, len(g), team_size=E.TEAM_AUTO_LISTS)
    pos = np.asarray([2], dtype=np.uint32)
    rng = np.random.default_rng(9)
    params = rng.uniform(2.5, 3.5, (16, 1))
    x0 = g[None, :] + rng.uniform(-0.05, 0.05, (16, len(g)))
    x, st, mask = s.solve_batch_params(x0, pos, params, want_mask=True)
    xo, it, conv, nun, mo = _oracle_each(extra, pos, params, x0)
    assert np.all(nun == 2) and np.array_equal(mask, mo) and np.array_equal(st["n_unsatisfied"], nun)
    assert np.array_equal(st["iterations"], it) and np.array_equal(st["converged"], conv)
    assert np.all(np.abs(x - xo) <= 1e-6 * np.maximum(1.0, np.abs(xo)))
    assert np.all(np.abs(x[:, 2] - 3.5) <= 1e-6)  # the undriven horizontal distance (2.5 from x = 1) holds


def test_literal_trap_specialised_systems_still_take_per_system_parameters(E):
    ref = T.load(T.gen_big_problem(64))
    recs = O.stack(ref.constraints)
    s = E.System(recs, ref.num_vars)
    assert s.specialize(wait=True) == 2
    pos, params, x0 = _driven_draw(E, recs, ref.guesses, 16, 4)
    x, st, mask = s.solve_batch_params(x0, pos, params, want_mask=True)
    xo, it, conv, nun, mo = _oracle_each(recs, pos, params, x0)
    assert np.array_equal(x, xo) and np.array_equal(st["iterations"], it) and np.array_equal(mask, mo)
    xs, _, _ = s.solve_batch(x0)  # (the compiled kernel itself keeps the parameters the system was created with)
    assert not np.array_equal(xs, x)
    recs, g, driven = CASES["arc_length"]
    small = E.System(recs, len(g))
    assert small.specialize(wait=True) == 2  # the lane kernel, parameters as literals
    small.solve_batch(g[None, :])
    pos, params, x0 = _draw(recs, g, driven, 64, 7)
    x, st, mask = small.solve_batch_params(x0, pos, params, want_mask=True)
    _check_against_oracle(recs, pos, params, x0, x, st, mask, "arc_length on a specialised system")


def _assert_declined(E, s, x0, pos, params):
    import ctypes as C

    from ezpz_amd._lib import STATUS_DTYPE

    batch = len(x0)
    x = np.full_like(x0, -777.0)
    st = np.full(batch, 0xAB, dtype=np.uint8).repeat(STATUS_DTYPE.itemsize).view(STATUS_DTYPE)
    st_before = st.copy()
    pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.uint32)
    params = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    cfg = E.Config()._c()
    n_param = 1 if pos is None else len(pos)
    rc = E.lib().ezpz_system_solve_batch_params(s._h, x0.ctypes.data, None if pos is None else pos.ctypes.data, n_param,
                                                None if params is None else params.ctypes.data, batch, C.byref(cfg), x.ctypes.data,
                                                st.ctypes.data, None, None, 0)
    assert rc == ERR_INVALID_ARGUMENT, rc
    assert np.all(x == -777.0) and st.tobytes() == st_before.tobytes()


def test_errors_leave_outputs_untouched(E):
    recs, g, _ = CASES["axis_distances_and_fixed"]
    recs = O.stack(list(recs) + [O.horizontal(P0, P1)])  # position 4: a constraint without a parameter
    s = E.System(recs, len(g), team_size=E.TEAM_AUTO_LISTS)
    x0 = np.repeat(g[None, :], 4, axis=0)
    one = np.ones((4, 1))
    _assert_declined(E, s, x0, [5], one)            # a position >= n_cs
    _assert_declined(E, s, x0, [2, 2], np.ones((4, 2)))  # a duplicate
    _assert_declined(E, s, x0, [4], one)            # no parameter
    _assert_declined(E, s, x0, None, one)           # null positions
    _assert_declined(E, s, x0, [2], None)           # null params
    with pytest.raises(ValueError):
        s.solve_batch_params(x0, [2], np.ones((3, 1)))


def test_device_form_on_a_stream_same_bits_and_in_place(E):
    import torch

    recs, g, driven = CASES["arc_radius"]
    pos, params, x0 = _draw(recs, g, driven, 64, 11)
    s = E.System(recs, len(g), team_size=E.TEAM_AUTO_LISTS)
    x, st, _ = s.solve_batch_params(x0, pos, params)
    from ezpz_amd._lib import STATUS_DTYPE

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xd = torch.from_numpy(x0).cuda()
        pd = torch.from_numpy(params).cuda()
        std = torch.zeros(64 * STATUS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        s.solve_batch_params_device(xd.data_ptr(), pos, pd.data_ptr(), 64, xd.data_ptr(), std.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x)  # (x0 and x_out were the same buffer)
    assert np.array_equal(std.cpu().numpy().view(STATUS_DTYPE), st)
