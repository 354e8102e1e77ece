"""Driven dimensions and sweeps on the FRONTAL shape (ezpz_system_set_params_route; csrc/front_params.hip, the PAR and SWP builds of
front_solve_kernel): against the oracle run once per system, and -- the main bar -- bit for bit against systems rebuilt on the
fronts with the parameters baked in: values, statuses, masks, warning logs, on one workgroup per system and on several, for a
workgroup's second system, with the driven values staged in LDS and read from global memory; sweeps bit for bit against the
chain of params calls; the setter's errors and the entry's surface.  Bars: tests/sensitivity.py for the oracle comparison."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import front_sens_ref as FS
import gen
from oracle import oracle as O
from oracle import textual as T
from sensitivity import assert_batch_matches_oracle
from sweep_common import chain, chain_of_calls, driven_walk, substituted

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
SWEEP_FRONTS = 5
# EzpzSweepPlan::in_kernel of the fronts, as sweep.hip's table has it from profiles/front_params_rate.txt: one launch on one
# workgroup per system, and on several
IN_KERNEL = {"one workgroup": 1, "several workgroups": 1}


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


class env:
    """Environment switches the symbolic phase reads when a system is created."""

    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def front_system(E, recs, n, wgs=1, route="fronts"):
    """A system on the fronts with `wgs` workgroups per system (the planner gives every input of this file what it is asked for)."""
    with env(EZPZ_FRONT_WGS=wgs):
        s = E.System(recs, n, team_size=E.TEAM_FRONTS)
    info = s.info()
    assert info["team_mode"] == 5 and info["grid_workgroups"] == wgs and info["front_max_batch"] == 0xFFFFFFFF, info
    if route:
        s.set_params_route(route)
    return s


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _driven(E, recs):
    return np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)


def _draw(E, recs, g, batch, seed, amplitude=1e-3, jitter=0.02):
    rng = np.random.default_rng(seed)
    pos = _driven(E, recs)
    params = recs["param"][pos][None, :] + rng.uniform(-amplitude, amplitude, (batch, len(pos)))
    x0 = g[None, :] + rng.uniform(-jitter, jitter, (batch, len(g)))
    return pos, params, x0


def _same(a, b, what):
    (xa, sa, ma), (xb, sb, mb) = a, b
    assert xa.shape == xb.shape and sa.shape == sb.shape, what
    assert np.array_equal(xa, xb, equal_nan=True), what
    assert sa.tobytes() == sb.tobytes(), what
    if ma is not None or mb is not None:
        assert np.array_equal(ma, mb), what


def _rebuilt_each(E, recs, n, wgs, pos, params, x0, cfg=None):
    """System b rebuilt on the fronts with its parameters baked in, solved by the plain entry."""
    xs, sts, masks = [], [], []
    for b in range(len(x0)):
        fresh = front_system(E, substituted(recs, pos, params[b]), n, wgs, route=None)
        x, st, mask = fresh.solve_batch(x0[b:b + 1], cfg, want_mask=True)
        xs.append(x), sts.append(st), masks.append(mask)
    return np.concatenate(xs), np.concatenate(sts), np.concatenate(masks)


def _inputs(name):
    if name in FS.WIDE:
        return FS.inputs(name)
    if name.startswith("sketch"):
        return gen.connected_sketch(int(name[6:]), 1000 + int(name[6:]))
    return gen.graph_sketch(name, 50, np.random.default_rng(21))


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npts,wgs", [(40, 1), (200, 3)])
def test_chain_against_the_oracle(E, npts, wgs):
    """Every parameter of a chain of points driven +-0.1 on 8 systems: statuses equal to the oracle run once per system on the
    substituted constraints, coordinates at the fronts' bar (tests/test_front_params_cpu.py: the oracle converges on these inputs)."""
    recs, g = chain(npts)
    s = front_system(E, recs, len(g), wgs)
    pos, params, x0 = _draw(E, recs, g, 8, 21, amplitude=0.1, jitter=0.03)
    x, st, mask = s.solve_batch_params(x0, pos, params, want_mask=True)
    for b in range(8):
        r = substituted(recs, pos, params[b])
        rc, xo, it, conv, nun = O.solve_batch(r, x0[b:b + 1], None, linsolve=O.LINSOLVE_SPARSE)
        assert rc == 0
        assert (int(st["iterations"][b]), int(st["converged"][b]), int(st["n_unsatisfied"][b])) == (int(it[0]), int(conv[0]), int(nun[0])), b
        assert int(mask[b].sum()) == int(nun[0])
        assert_batch_matches_oracle(r, x0[b:b + 1], x[b:b + 1], st["iterations"][b:b + 1], st["converged"][b:b + 1], None,
                                    oracle_result=(xo, it, conv), what=("front params", npts, wgs, b))


# The draw of the wide inputs (front_sens_ref.WIDE: fronts of up to 63 rows, remote children of more than 50 rows arriving as
# chunks, minimum-degree plans; tests/test_front_sens_cpu.py pins those shapes).  At the file's default draw (1e-3, 0.02) the
# oracle converges on all 8 systems of tree60 in 3 iterations and runs to its 35-iteration limit on all 8 of tree108 and comb213
# and on 5 of tree144; at (1e-4, 1e-3) it converges on all 8 of tree108 in 3-4 iterations, on 4 of tree144 and on 5 of comb213
# (the device: 8 of tree60 in 2 iterations, 8 of tree108, 4 of tree144, 6 of comb213 -- the rebuilt systems end the same way).
WIDE_DRAW = dict(amplitude=1e-4, jitter=1e-3)


@pytest.mark.parametrize("name,wgs", [("tree60", 1), ("tree60", 2), ("tree60", 4), ("tree108", 1), ("tree108", 2), ("tree108", 4)])
def test_wide_fronts_against_the_oracle(E, name, wgs):
    """tree60 (fronts of 58 rows, a remote child of 52 rows on 2 workgroups) at the default draw, tree108 (a minimum-degree plan)
    at the small one: statuses equal to the oracle's, coordinates at the fronts' bar (tests/test_front_params_cpu.py: the oracle
    converges on exactly these 8 draws of each)."""
    recs, g = _inputs(name)
    s = front_system(E, recs, len(g), wgs)
    pos, params, x0 = _draw(E, recs, g, 8, 33, **({} if name == "tree60" else WIDE_DRAW))
    x, st, mask = s.solve_batch_params(x0, pos, params, want_mask=True)
    for b in range(8):
        r = substituted(recs, pos, params[b])
        rc, xo, it, conv, nun = O.solve_batch(r, x0[b:b + 1], None, linsolve=O.LINSOLVE_SPARSE)
        assert rc == 0 and int(conv[0]) == 1
        assert (int(st["iterations"][b]), int(st["converged"][b]), int(st["n_unsatisfied"][b])) == (int(it[0]), int(conv[0]), int(nun[0])), b
        assert int(mask[b].sum()) == int(nun[0])
        assert_batch_matches_oracle(r, x0[b:b + 1], x[b:b + 1], st["iterations"][b:b + 1], st["converged"][b:b + 1], None,
                                    oracle_result=(xo, it, conv), what=("front params", name, wgs, b))


# ---- 2. bit for bit against rebuilt systems ----------------------------------------------------------------------------------------
REBUILT = [("sketch25", 1), ("sketch75", 2), ("sketch150", 3), ("band", 1), ("band", 4), ("hub", 1), ("hub", 4),
           ("tree60", 1), ("tree60", 2), ("tree108", 2), ("tree144", 4), ("comb213", 4)]


@pytest.fixture(scope="module")
def rebuilt(E):
    """The inputs of a case and what its 8 rebuilt systems give, computed once and shared."""
    cache = {}

    def get(name, wgs):
        if (name, wgs) not in cache:
            recs, g = _inputs(name)
            pos, params, x0 = _draw(E, recs, g, 8, 33, **(WIDE_DRAW if name in FS.WIDE else {}))
            cache[(name, wgs)] = (recs, g, pos, params, x0, _rebuilt_each(E, recs, len(g), wgs, pos, params, x0))
        return cache[(name, wgs)]

    return get


@pytest.mark.parametrize("name,wgs", REBUILT, ids=["%s-%d" % c for c in REBUILT])
def test_same_bits_as_rebuilt_systems_on_the_fronts(E, rebuilt, name, wgs):
    recs, g, pos, params, x0, want = rebuilt(name, wgs)
    n = len(g)
    s = front_system(E, recs, n, wgs)
    got = s.solve_batch_params(x0, pos, params, want_mask=True)
    _same(got, want, (name, wgs))
    print(name, wgs, "converged", int(got[1]["converged"].sum()), "of 8, iterations", got[1]["iterations"].tolist())
    # a permuted list with its columns; half the list; the first list right after; the system's own values
    perm = np.random.default_rng(5).permutation(len(pos))
    _same(s.solve_batch_params(x0, pos[perm], params[:, perm], want_mask=True), want, (name, wgs, "permuted"))
    half = pos[: max(1, len(pos) // 2)]
    xh, sth, mh = s.solve_batch_params(x0[:2], half, params[:2, : len(half)], want_mask=True)
    _same((xh, sth, mh), _rebuilt_each(E, recs, n, wgs, half, params[:2, : len(half)], x0[:2]), (name, wgs, "half the list"))
    _same(s.solve_batch_params(x0, pos, params, want_mask=True), want, (name, wgs, "the list again"))
    own = np.repeat(recs["param"][pos][None, :], 8, axis=0)
    plain = s.solve_batch(x0, want_mask=True)
    _same(s.solve_batch_params(x0, pos, own, want_mask=True), plain, (name, wgs, "own values"))
    # the route unset: what the entry gave before there was a route to set (the list-walk teams' bits)
    never = front_system(E, recs, n, wgs, route=None)
    s.set_params_route("default")
    _same(s.solve_batch_params(x0, pos, params, want_mask=True), never.solve_batch_params(x0, pos, params, want_mask=True),
          (name, wgs, "route unset"))


# ---- 3. / 4. persistent workgroups and slots that take a second system --------------------------------------------------------------
def _period_8_check(E, name, wgs, batch, rebuilt):
    recs, g, pos, p8, _, _ = rebuilt(name, wgs)
    n = len(g)
    s = front_system(E, recs, n, wgs)
    assert batch % 8 == 0
    params = np.tile(p8, (batch // 8, 1))
    x0 = g[None, :] + np.random.default_rng(34).uniform(-0.02, 0.02, (batch, n))
    x, st, mask = s.solve_batch_params(x0, pos, params, want_mask=True)
    for b in range(8):
        fresh = front_system(E, substituted(recs, pos, p8[b]), n, wgs, route=None)
        mine = np.arange(b, batch, 8)
        _same((x[mine], st[mine], mask[mine]), fresh.solve_batch(x0[mine], want_mask=True), (name, wgs, b))


def test_persistent_workgroups_take_a_second_system(E, rebuilt):
    """More than twice the systems any occupancy of 512-thread workgroups holds: every workgroup goes on to a second system whose
    parameters differ from its first one's (they repeat with period 8, the grid is a multiple of 64)."""
    _period_8_check(E, "sketch25", 1, _cus() * 64 + 64, rebuilt)


def test_slots_of_two_workgroups_take_further_systems(E, rebuilt):
    """Two workgroups per system, more systems than the device has slots (at most one workgroup of 512 threads per CU and
    system half: CUs / 2 slots at least, 2 x CUs at most)."""
    _period_8_check(E, "sketch75", 2, _cus() * 4 + 64, rebuilt)


# ---- 5. both forms of the driven values ---------------------------------------------------------------------------------------------
def _child_main():
    """In a child process (EZPZ_PARAMS_LDS is read once per process): the params entry and a sweep, one and two workgroups."""
    import ezpz_amd as E

    for name, wgs in (("sketch25", 1), ("sketch75", 2)):
        recs, g = _inputs(name)
        pos, params, x0 = _draw(E, recs, g, 8, 33)
        s = front_system(E, recs, len(g), wgs)
        _same(s.solve_batch_params(x0, pos, params, want_mask=True), _rebuilt_each(E, recs, len(g), wgs, pos, params, x0), name)
        wpos, wparams, wx0 = driven_walk(E, recs, g, 4, 3, 21, amplitude=1e-3, jitter=0.02)
        plan = s.sweep_params_plan(wpos)
        _same(s.sweep_params(wx0, wpos, wparams, want_mask=True), chain_of_calls(s, wx0, wpos, wparams), name + " sweep")
        print("same bits:", name, "params_in_lds", plan["params_in_lds"], "lds_bytes", plan["lds_bytes"], flush=True)


@pytest.mark.parametrize("staged", [False, True])
def test_values_read_from_global_memory_and_staged_in_lds(E, staged):
    """EZPZ_PARAMS_LDS=0: the rows are read through L2 where the caller left them; without it a workgroup stages its system's row
    behind everything else in its LDS (a 512-thread workgroup has the CU to itself: the copy costs no workgroup).  Same bits, and
    the plan and EZPZ_DEBUG=params say which form ran."""
    env_ = dict(os.environ, EZPZ_DEBUG="params", EZPZ_AMD_NO_BUILD="1")
    env_.pop("EZPZ_PARAMS_LDS", None)
    if not staged:
        env_["EZPZ_PARAMS_LDS"] = "0"
    here = os.path.dirname(os.path.abspath(__file__))
    env_["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here] + ([env_["PYTHONPATH"]] if env_.get("PYTHONPATH") else []))
    run = subprocess.run([sys.executable, "-c", "import test_gpu_front_params as t; t._child_main()"], cwd=here, env=env_,
                         capture_output=True, text=True, timeout=600)
    lines = [l for l in run.stderr.splitlines() if l.startswith("[ezpz params] fronts")]
    print(run.stdout, "\n".join(sorted(set(lines))))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stdout.count("same bits:") == 2 and lines
    assert run.stdout.count("params_in_lds %d" % (1 if staged else 0)) == 2
    want = "staged in LDS" if staged else "read from global memory"
    assert all(want in l for l in lines), lines


# ---- 6. all 25 kinds with weights ---------------------------------------------------------------------------------------------------
def _params_logged(E, s, x0, pos, params, cfg, warn_cap):
    from ezpz_amd._lib import STATUS_DTYPE

    batch = len(x0)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    pos = np.ascontiguousarray(pos, dtype=np.uint32)
    params = np.ascontiguousarray(params, dtype=np.float64)
    x, st = np.empty_like(x0), np.zeros(batch, dtype=STATUS_DTYPE)
    mask = np.zeros((batch, len(s.records)), dtype=np.uint8)
    log = np.zeros((batch, warn_cap), dtype=np.uint64)
    c = cfg._c()
    rc = E.lib().ezpz_system_solve_batch_params(s._h, x0.ctypes.data, pos.ctypes.data, len(pos), params.ctypes.data, batch, C.byref(c),
                                                x.ctypes.data, st.ctypes.data, mask.ctypes.data, log.ctypes.data, warn_cap)
    assert rc == 0, rc
    logs = []
    for b in range(batch):
        e = np.sort(log[b, : min(int(st["n_warnings"][b]), warn_cap)])
        logs.append([(int(v >> np.uint64(32)), int(v & np.uint64(0xFFFFFFFF))) for v in e])
    return x, st, mask, logs


@pytest.mark.parametrize("wgs", [1, 3])
def test_all_kinds_weights_warnings_and_masks(E, wgs):
    """The random system of all 25 kinds of tests/test_gpu_fronts.py (guards fire, weights differ) with every parametrised
    constraint driven -- the angle kinds and ArcLength among them, on the non-linear build: values, statuses, masks and warning
    logs equal to the rebuilt systems'."""
    rng = np.random.default_rng(5)
    n = 40
    cons = []
    for kind in range(25):
        c = gen.arb_constraint(rng, kind, hi=32)
        c["weight"] = float(rng.uniform(0.5, 2.0))
        cons.append(c)
    recs = O.stack(cons)
    x0 = rng.uniform(-5.0, 5.0, (6, n))
    x0[5, :8] = 0.0  # coincident points: guards
    pos = _driven(E, recs)
    assert len(pos) >= 10
    params = recs["param"][pos][None, :] + np.random.default_rng(6).uniform(-0.2, 0.2, (6, len(pos)))
    s = front_system(E, recs, n, wgs)
    cfg = E.Config(max_iterations=25)
    x, st, mask, logs = _params_logged(E, s, x0, pos, params, cfg, 4096)
    assert int(st["n_warnings"].sum()) > 0
    for b in range(6):
        fresh = front_system(E, substituted(recs, pos, params[b]), n, wgs, route=None)
        xf, stf, lf = fresh.solve_batch_logged(x0[b:b + 1], cfg, warn_cap=4096)
        _, _, mf = fresh.solve_batch(x0[b:b + 1], cfg, want_mask=True)
        assert np.array_equal(x[b], xf[0], equal_nan=True) and st[b] == stf[0] and np.array_equal(mask[b], mf[0]), (wgs, b)
        assert logs[b] == lf[0], (wgs, b)


# ---- 7. a linear-only system --------------------------------------------------------------------------------------------------------
def test_linear_only_system(E):
    """Fixed, horizontal and vertical distances only: the linear build of the kernel, whose one Jacobian sweep rides in the first
    evaluation -- with the driven values in it.  Bit for bit against rebuilt systems, and the answer is the driven layout."""
    npts = 30
    cons = [O.fixed(0, 0.5), O.fixed(1, -0.5)]
    for k in range(1, npts):
        a, b = (2 * (k - 1), 2 * k - 1), (2 * k, 2 * k + 1)
        cons += [O.horizontal_distance(b, a, 1.0 + 0.01 * k), O.vertical_distance(b, a, 0.5)]
    recs = O.stack(cons)
    n = 2 * npts
    g = np.zeros(n)
    s = front_system(E, recs, n, 1)
    pos, params, x0 = _draw(E, recs, g, 8, 3, amplitude=0.3, jitter=0.5)
    assert len(pos) == len(recs)
    got = s.solve_batch_params(x0, pos, params, want_mask=True)
    _same(got, _rebuilt_each(E, recs, n, 1, pos, params, x0), "linear only")
    assert np.all(got[1]["converged"] == 1)
    assert np.allclose(got[0][:, 0], params[:, 0]) and np.allclose(got[0][:, 2] - got[0][:, 0], params[:, 2])


# ---- 8. sweeps ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,wgs", [("sketch25", 1), ("sketch75", 2), ("tree60", 2)])
def test_sweeps_same_bits_as_the_chain_of_calls(E, name, wgs):
    """tree60 on 2 workgroups (fronts of 58 rows, a remote child of 52 rows arriving as chunks at every iteration of every step):
    on the oracle all 24 of its steps converge within 5 iterations and none within 3, so its steps that run to the limit come
    from a second sweep at 2 iterations."""
    recs, g = _inputs(name)
    s = front_system(E, recs, len(g), wgs)
    pos, params, x0 = driven_walk(E, recs, g, 4, 6, 21, amplitude=1e-3, jitter=0.02)
    plan = s.sweep_params_plan(pos)
    print(name, wgs, plan)
    assert plan["route"] == SWEEP_FRONTS and plan["route_name"] == "fronts", plan
    assert plan["in_kernel"] == IN_KERNEL["one workgroup" if wgs == 1 else "several workgroups"], plan
    assert plan["params_in_lds"] == 1 and plan["lds_bytes"] >= len(pos) * 8, plan
    # (5 iterations: on the oracle 15 of the 24 steps of the smaller sketch and 21 of the larger one's converge, the others --
    # most first steps among them -- run to the limit, and the next step starts from what they left)
    cfg = E.Config(max_iterations=5)
    got = s.sweep_params(x0, pos, params, config=cfg, want_mask=True)
    want = chain_of_calls(s, x0, pos, params, config=cfg)
    _same(got, want, (name, wgs))
    conv = got[1]["converged"]
    print(name, wgs, "converged", int(conv.sum()), "of", conv.size)
    if name == "tree60":
        assert conv.all()
        short = E.Config(max_iterations=2)
        cut = s.sweep_params(x0, pos, params, config=short, want_mask=True)
        _same(cut, chain_of_calls(s, x0, pos, params, config=short), (name, wgs, "2 iterations"))
        assert not cut[1]["converged"].any()
    else:
        assert 0 < conv.sum() < conv.size  # (steps that converge and steps that run to the iteration limit)
    _same(s.sweep_params(x0, pos, params, want_mask=True), chain_of_calls(s, x0, pos, params), (name, wgs, "default limit"))
    assert not np.array_equal(got[0][0], got[0][5])
    # one step is the params entry
    x1, st1, m1 = s.sweep_params(x0, pos, params[:1], want_mask=True)
    _same((x1[0], st1[0], m1[0]), s.solve_batch_params(x0, pos, params[0], want_mask=True), (name, wgs, "one step"))
    # more sweeps than the launch has slots: a slot's second sweep, 3 steps each
    slots = _cus() * 2 + 8 if wgs == 1 else _cus() + 8
    pos, params, x0 = driven_walk(E, recs, g, slots, 3, 22, amplitude=1e-3, jitter=0.02)
    _same(s.sweep_params(x0, pos, params, want_mask=True), chain_of_calls(s, x0, pos, params), (name, wgs, "a slot's second sweep"))


# ---- 9. errors and surface ----------------------------------------------------------------------------------------------------------
def _assert_declined(E, s, x0, pos, params):
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


def test_systems_the_fronts_do_not_serve_keep_their_route(E):
    ref = T.load(T.gen_big_problem(64))
    brecs = O.stack(ref.constraints)
    crecs, cg = chain(40)
    for what, recs, g, team in (("block system", brecs, ref.guesses, 0), ("list-walk system", crecs, cg, E.TEAM_AUTO_LISTS)):
        s = E.System(recs, len(g), team_size=team)
        assert s.info()["front_max_batch"] != 0xFFFFFFFF, what
        pos, params, x0 = _draw(E, recs, g, 4, 9, amplitude=0.1)
        before = s.solve_batch_params(x0, pos, params, want_mask=True)
        with pytest.raises(E.NonLinearSystemError) as err:
            s.set_params_route("fronts")
        assert err.value.code == ERR_INVALID_ARGUMENT, what
        _same(s.solve_batch_params(x0, pos, params, want_mask=True), before, what)
        s.set_params_route("default")
    assert E.lib().ezpz_system_set_params_route(s._h, 2) == ERR_INVALID_ARGUMENT
    # a grid team (one system on several workgroups of the list walk): no frontal plan, so no route to set, and declined as before
    lad = T.load(T.gen_big_problem(12000))
    lrecs = O.stack(lad.constraints)
    grid = E.System(lrecs, lad.num_vars)
    assert grid.info()["grid_workgroups"] > 1 and grid.info()["front_max_batch"] == 0
    with pytest.raises(E.NonLinearSystemError):
        grid.set_params_route("fronts")
    lpos = _driven(E, lrecs)[:4]
    _assert_declined(E, grid, np.repeat(lad.guesses[None, :], 2, axis=0), lpos, np.repeat(lrecs["param"][lpos][None, :], 2, axis=0))
    with pytest.raises(ValueError):
        s.set_params_route("lists")


def test_argument_errors_leave_outputs_untouched(E):
    recs, g = chain(40)  # (its horizontal and vertical constraints have no parameter)
    s = front_system(E, recs, len(g), 1)
    pos = _driven(E, recs)
    no_param = [i for i in range(len(recs)) if not E.constraint_has_param(recs[i])][0]
    x0 = np.repeat(g[None, :], 4, axis=0)
    one = np.ones((4, 1))
    _assert_declined(E, s, x0, [len(recs)], one)                 # a position >= n_cs
    _assert_declined(E, s, x0, [pos[0], pos[0]], np.ones((4, 2)))  # a duplicate
    _assert_declined(E, s, x0, [no_param], one)                  # no parameter
    _assert_declined(E, s, x0, None, one)                        # null positions
    _assert_declined(E, s, x0, [pos[0]], None)                   # null params


def test_device_form_on_a_stream_in_place_and_capture_refused(E):
    import warnings

    import torch

    from ezpz_amd._lib import STATUS_DTYPE

    for name, wgs in (("sketch25", 1), ("sketch75", 2)):
        recs, g = _inputs(name)
        s = front_system(E, recs, len(g), wgs)
        pos, params, x0 = _draw(E, recs, g, 8, 33)
        x, st, _ = s.solve_batch_params(x0, pos, params)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            xd = torch.from_numpy(x0).cuda()
            pd = torch.from_numpy(params).cuda()
            std = torch.zeros(8 * STATUS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            s.solve_batch_params_device(xd.data_ptr(), pos, pd.data_ptr(), 8, xd.data_ptr(), std.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(xd.cpu().numpy(), x)  # (x0 and x_out were the same buffer)
        assert std.cpu().numpy().view(STATUS_DTYPE).tobytes() == st.tobytes()
        if wgs == 1:
            continue
        # several workgroups: a capture is refused up front, nothing enqueued, and the next direct call gives the same bits
        xin = torch.from_numpy(x0).cuda()
        xo = torch.full_like(xin, -777.0)
        graph = torch.cuda.CUDAGraph()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # ("The CUDA Graph is empty")
            with pytest.raises(E.NonLinearSystemError) as err:
                with torch.cuda.graph(graph, stream=stream):
                    s.solve_batch_params_device(xin.data_ptr(), pos, pd.data_ptr(), 8, xo.data_ptr(), std.data_ptr(),
                                                stream=torch.cuda.current_stream().cuda_stream)
        assert err.value.code == ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert bool((xo == -777.0).all())
        s.solve_batch_params_device(xin.data_ptr(), pos, pd.data_ptr(), 8, xo.data_ptr(), std.data_ptr(),
                                    stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(xo.cpu().numpy(), x)


# ---- 10. torch ----------------------------------------------------------------------------------------------------------------------
def test_torch_solve_params_takes_the_systems_route(E, rebuilt):
    import torch

    from ezpz_amd import torch_ops

    recs, g, pos, params, x0, want = rebuilt("sketch75", 2)
    s = front_system(E, recs, len(g), 2)
    p = torch.from_numpy(params).cuda().requires_grad_(True)
    x = torch_ops.solve_params(s, torch.from_numpy(x0).cuda(), pos, p)
    assert np.array_equal(x.detach().cpu().numpy(), want[0])
    x.sum().backward()
    grad = p.grad.cpu().numpy()
    assert grad.shape == params.shape and np.all(np.isfinite(grad)) and np.any(grad != 0.0)
