"""GPU tests (-m gpu) of the dimension targets (ezpz_system_seek_targets and its _device form; csrc/seek.hip): the run is the chain of
the entries it is made of plus the step tests/seek_ref.py restates from the header, byte for byte; known answers; bounds; a seek
never leaves an assembled answer; a system's bytes do not depend on its neighbours, the chunk, the stream or the form.  Every
system is 6 to 16 variables: the shapes are the team sizes (n_param 1 .. 16), the chunk of 64 systems and the rounds, not a
workload's.

Bars.  Against the chain: bytes.  The known answer a = 2 + sqrt(37): 2e-6 -- tol 1e-6 on c divided by dc/da = (2a - b) / (2c) ~ 0.87,
plus the inner solve's residual tolerance 1e-8.  worst = |7 - sqrt(21)| to 1e-9 holds with an inner residual tolerance of 1e-11 (the
measured side is as exact as the inner solve leaves the point; the default 1e-8 alone would exceed the bar)."""
import ctypes as C
import math

import numpy as np
import pytest

import measure_ref as M
import seek_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT, ERR_TOO_LARGE = -103, -102
COLD_STAMPS = {20, 21, 22, 23}  # csrc/call_trace.hpp: the symbolic phase of a system's first request, no launch
SEEK_LAUNCHED = 71
_CACHE = {}


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


def _trace(E, call):
    trace = np.zeros(4096, dtype=np.uint64)
    E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
    try:
        out = call()
    finally:
        k = E.lib().ezpz_debug_call_trace(None, 0)
    return out, [int(v) for v in trace[:k:2]]


def policies(E, n_param, n_meas, inner=None, chunk=0, **kw):
    """(the library's SeekConfig, the reference's Policy) of one policy."""
    return E.SeekConfig(inner=inner, chunk=chunk, **kw), R.Policy(n_param, n_meas, **kw)


def result_bytes(res):
    return [res.params.tobytes(), res.x.tobytes(), res.m.tobytes(), res.info.tobytes()] + ([res.cost_trace.tobytes()] if res.cost_trace is not None else [])


def assert_is_the_chain(E, s, x0, pos, p0, recs, targets, inner=None, **kw):
    cfg, pol = policies(E, len(pos), len(recs), inner=inner, **kw)
    res = s.seek_targets(x0, pos, p0, recs, targets, cfg, want_trace=True)
    params, x, m, info, trace = R.run(s, x0, pos, p0, recs, targets, pol, config=inner)
    for f in R.INFO_DTYPE.names:
        assert res.info[f].tobytes() == info[f].tobytes(), (f, res.info[f], info[f])
    assert res.params.tobytes() == params.tobytes(), (res.params, params)
    assert res.x.tobytes() == x.tobytes() and res.m.tobytes() == m.tobytes()
    assert res.cost_trace.tobytes() == trace.tobytes()
    return res


# ---- the 16-variable system: all Fixed, every parameter driven (x = p: the seek is m(p) = t) --------------------------------------
N16 = 16
KINDS13 = M.SUBTRACTING + M.CURVED
_rng = np.random.default_rng(7)
X16 = _rng.uniform(0.5, 3.0, N16) * _rng.choice([-1.0, 1.0], N16) + np.arange(N16) * 0.37


def records16(n_meas, seed=13):
    """n_meas records over the 16 variables, the 13 measurable kinds in turn (angles in degrees and radians alternately)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_meas):
        kind = KINDS13[i % 13]
        tag = (O.ANGLE_OTHER_DEG if (i // 13) % 2 == 0 else O.ANGLE_OTHER_RAD) if kind in M.ANGLES else 0
        out.append(O._mk(kind, list(rng.permutation(N16)[: O.KIND_NUM_IDS[kind]]), 0.0, tag=tag))
    return O.stack(out)


def system16(E):
    if "s16" not in _CACHE:
        _CACHE["s16"] = E.System(O.stack([O.fixed(v, float(X16[v])) for v in range(N16)]), N16)
    return _CACHE["s16"]


def targets16(E, recs, batch, seed):
    """Targets per system: the measurements of the point moved by 0 (already there), a little, more -- and one set out of reach."""
    rng = np.random.default_rng(seed)
    moved = X16[None, :] + rng.normal(size=(batch, N16)) * (np.arange(batch)[:, None] % 4) * 0.1
    t = system16(E).measure(moved, recs)
    if batch > 1:
        t[-1] = rng.normal(size=len(recs)) * 50.0
    return t


# ---- the connected triangle: A fixed, B on the horizontal line through A, three side lengths c = AB, a = BC, b = CA ----------------
A, B, Cc = (0, 1), (2, 3), (4, 5)
TRI = O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(3, 0.0), O.distance(A, B, 5.0), O.distance(B, Cc, 3.0), O.distance(Cc, A, 4.0)])
TRI_X0 = np.array([0.0, 0.0, 5.0, 0.0, 3.2, 2.4])  # the 3-4-5 triangle's solution
REC_C = O.stack([O.distance(A, B, 0.0)])


def triangle(E):
    if "tri" not in _CACHE:
        _CACHE["tri"] = E.System(TRI, 6)
    return _CACHE["tri"]


# ---- the known answers' triangle: C fixed, A on the horizontal line through C at b = 4, the angle at C 60 degrees, a = CB driven -----
KC, KA, KB = (0, 1), (2, 3), (4, 5)
KNOWN = O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(3, 0.0), O.distance(KC, KA, 4.0), O.lines_at_angle(KC, KA, KC, KB, ("deg", 60.0)),
                 O.distance(KC, KB, 3.0)])
REC_AB = O.stack([O.distance(KA, KB, 0.0)])


def known(E):
    if "known" not in _CACHE:
        rc, x0, _, conv, nun = O.solve_batch(KNOWN, np.array([[0.0, 0.0, 4.0, 0.0, 1.5, 2.6]]))
        assert rc == 0 and conv[0] and nun[0] == 0
        _CACHE["known"] = (E.System(KNOWN, 6), x0[0])
    return _CACHE["known"]


# ---- 1. the run is the chain ------------------------------------------------------------------------------------------------------
def test_the_run_is_the_chain_all_fixed_13_kinds(E):
    recs = records16(13)
    t = targets16(E, recs, 5, 1)
    res = assert_is_the_chain(E, system16(E), np.tile(X16, (5, 1)), list(range(N16)), np.tile(X16, (5, 1)), recs, t)
    assert res.status[0] == R.REACHED and res.iterations[0] == 0  # (already there)
    assert len(set(res.status.tolist())) >= 2 and res.accepted.max() >= 2, res.info


def test_the_run_is_the_chain_triangle(E):
    s = triangle(E)
    recs = O.stack([O.vertical_distance(Cc, A, 0.0), O.horizontal_distance(Cc, A, 0.0), O.distance(A, B, 0.0)])
    # targets: the apex and the base of other triangles; the last one asks for a base no triangle of these sides' range closes on
    t = np.array([[2.4, 3.2, 5.0], [2.0, 3.0, 5.5], [3.0, 2.5, 4.5], [1.0, 4.5, 6.5], [2.0, 3.0, 40.0]])
    res = assert_is_the_chain(E, s, np.tile(TRI_X0, (5, 1)), [3, 4, 5], np.tile([5.0, 3.0, 4.0], (5, 1)), recs, t, hi=[8.0, 8.0, 8.0])
    assert res.status[0] == R.REACHED and res.iterations[0] == 0
    assert (res.status[1:4] == R.REACHED).all() and res.status[4] != R.REACHED, res.info
    assert np.all(np.abs(res.m[1:4] - t[1:4]) <= 1e-6)


# ---- 2. known answers ---------------------------------------------------------------------------------------------------------------
def test_known_answer_side_from_the_law_of_cosines(E):
    s, x0 = known(E)
    res = s.seek_targets(x0[None, :], [5], [[3.0]], REC_AB, [[7.0]])
    assert res.status[0] == R.REACHED and 1 <= res.accepted[0] <= 40, res.info
    print("a - (2 + sqrt(37)) =", res.params[0, 0] - (2.0 + math.sqrt(37.0)), "iterations", res.iterations[0])
    assert abs(res.params[0, 0] - (2.0 + math.sqrt(37.0))) <= 2e-6
    assert abs(res.m[0, 0] - 7.0) <= 1e-6 and res.worst[0] <= 1e-6 and res.cost[0] < res.cost0[0]


def test_known_answer_angle_in_degrees_on_a_two_parameter_point(E):
    # O at the origin, X at (1, 0), P = (px, py) with both coordinates driven: the angle XOP from 30 to 120 degrees
    p0 = np.array([2.0 * math.cos(math.radians(30.0)), 2.0 * math.sin(math.radians(30.0))])
    x0 = np.array([0.0, 0.0, 1.0, 0.0, p0[0], p0[1]])
    s = E.System(O.stack([O.fixed(v, float(x0[v])) for v in range(6)]), 6)
    rec = O.stack([O.lines_at_angle((0, 1), (2, 3), (0, 1), (4, 5), ("deg", 0.0))])
    res = assert_is_the_chain(E, s, x0[None, :], [4, 5], p0[None, :], rec, np.array([[120.0]]))
    assert res.status[0] == R.REACHED and abs(res.m[0, 0] - 120.0) <= 1e-6, res.info
    assert abs(math.degrees(math.atan2(res.x[0, 5], res.x[0, 4])) - 120.0) <= 1e-5
    # three targets for the two dimensions that no point meets: x = 1, y = 1, |OP| = 2
    over = O.stack([O.fixed(4, 0.0), O.fixed(5, 0.0), O.distance((0, 1), (4, 5), 0.0)])
    res = assert_is_the_chain(E, s, x0[None, :], [4, 5], p0[None, :], over, np.array([[1.0, 1.0, 2.0]]))
    assert res.status[0] == R.MINIMUM and res.cost[0] < res.cost0[0], res.info


# ---- 3. bounds ------------------------------------------------------------------------------------------------------------------------
def test_a_bound_is_kept_exactly_and_a_frozen_dimension_comes_back_as_it_went_in(E):
    s, x0 = known(E)
    inner = E.Config(residual_tolerance=1e-11)
    res = assert_is_the_chain(E, s, x0[None, :], [5], np.array([[3.0]]), REC_AB, np.array([[7.0]]), inner=inner, hi=[5.0])
    assert res.params[0, 0] == 5.0 and res.status[0] == R.MINIMUM, res.info
    print("worst - |7 - sqrt(21)| =", res.worst[0] - abs(7.0 - math.sqrt(21.0)))
    assert abs(res.worst[0] - abs(7.0 - math.sqrt(21.0))) <= 1e-9
    # b (position 3) frozen at a value with many bits, a free: b comes back bit for bit, the target is still met through a
    b = 4.0 + 1.0 / 3.0
    rc, xb, _, conv, nun = O.solve_batch(_with(KNOWN, 3, b), x0[None, :])
    assert rc == 0 and conv[0] and nun[0] == 0
    res = assert_is_the_chain(E, s, xb, [3, 5], np.array([[b, 3.0]]), REC_AB, np.array([[7.0]]), lo=[b, -np.inf], hi=[b, np.inf])
    assert res.params[0, 0].tobytes() == np.float64(b).tobytes() and res.status[0] == R.REACHED, res.info


def _with(recs, position, value):
    out = recs.copy()
    out["param"][position] = value
    return out


# ---- 4. never leaves an assembled answer ----------------------------------------------------------------------------------------------
def test_a_seek_never_leaves_an_assembled_answer(E):
    # a = 3, b = 4, c driven from 5, reference dimension the distance across c, target 8 > a + b
    s = triangle(E)
    res = assert_is_the_chain(E, s, TRI_X0[None, :], [3], np.array([[5.0]]), REC_C, np.array([[8.0]]))
    assert res.rejected[0] >= 1 and res.params[0, 0] < 7.0, res.info  # (the first trial is c ~ 8: it cannot assemble)
    assert res.status[0] in (R.STALLED, R.ITERATIONS)
    x, st, _ = s.solve_batch_params(res.x, [3], res.params)
    assert st["converged"][0] != 0 and st["n_unsatisfied"][0] == 0
    rc, _, _, conv, nun = O.solve_batch(_with(TRI, 3, res.params[0, 0]), res.x)
    assert rc == 0 and conv[0] and nun[0] == 0
    assert abs(res.m[0, 0] - res.params[0, 0]) <= 1e-7 and res.cost[0] < res.cost0[0]


# ---- 5. a system's bytes do not depend on its neighbours ---------------------------------------------------------------------------
def _neighbour_targets(batch, at, probe):
    """Targets for the triangle's c: neighbours that are there at the start (5), that finish soon (5.5, 6.5) and that never do
    (8: out of reach, runs out its iterations), with the probe's target at `at`."""
    t = np.array([[5.0], [8.0], [5.5], [6.5]])[np.arange(batch) % 4]
    t[at] = probe
    return t


@pytest.mark.parametrize("probe", [6.0, 8.0])
def test_bytes_do_not_depend_on_the_neighbours(E, probe):
    """probe 6: finishes early and waits many rounds for the others; probe 8: never finishes, while others freeze beside it."""
    s = triangle(E)

    def one(batch, at):
        res = s.seek_targets(np.tile(TRI_X0, (batch, 1)), [3], np.full((batch, 1), 5.0), REC_C, _neighbour_targets(batch, at, probe), want_trace=True)
        return [v[at].tobytes() for v in (res.params, res.x, res.m, res.info, res.cost_trace)], res

    alone, res = one(1, 0)
    assert (res.status[0] == R.REACHED and res.iterations[0] < 20) if probe == 6.0 else res.iterations[0] == 40, res.info
    for batch, at in ((5, 0), (5, 3), (5, 4), (65, 63), (65, 64), (257, 256), (257, 64)):
        got, res = one(batch, at)
        assert got == alone, (batch, at)
        # the neighbours do finish earlier and later: some at the start, some never
        assert res.iterations.min() == 0 and res.iterations.max() == 40 and R.REACHED in res.status.tolist(), (batch, res.info)


# ---- 6. team sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_param", [1, 4, 5, 8, 9, 16])
def test_team_sizes_against_the_chain(E, n_param):
    s = system16(E)
    rng = np.random.default_rng(100 + n_param)
    accepted = 0
    for n_meas in sorted({1, n_param, 64}):
        recs = records16(n_meas, seed=n_meas)
        pos = sorted(rng.permutation(N16)[:n_param].tolist())
        t = targets16(E, recs, 3, n_param * 100 + n_meas)
        scale = 10.0 ** rng.uniform(-1, 1, n_param)
        res = assert_is_the_chain(E, s, np.tile(X16, (3, 1)), pos, np.tile(X16[pos], (3, 1)), recs, t, max_iterations=8, scale=scale,
                                  lo=X16[pos] - 0.3, hi=X16[pos] + 0.3)
        assert res.status[0] == R.REACHED and res.iterations[0] == 0, (n_meas, res.info)
        accepted += int(res.accepted.sum())
    assert accepted >= 3  # (the cases do take steps)


# ---- 7. cutting changes nothing; 8. the device form ----------------------------------------------------------------------------------
def _batch200():
    rng = np.random.default_rng(200)
    return np.tile(TRI_X0, (200, 1)), np.full((200, 1), 5.0), rng.uniform(4.0, 8.5, (200, 1))


def test_cutting_the_batch_changes_nothing(E):
    s = triangle(E)
    x0, p0, t = _batch200()
    want = result_bytes(s.seek_targets(x0, [3], p0, REC_C, t, want_trace=True))
    for chunk in (64, 128, 100):  # (100 rounds up to 128)
        assert result_bytes(s.seek_targets(x0, [3], p0, REC_C, t, E.SeekConfig(chunk=chunk), want_trace=True)) == want, chunk
    _CACHE["batch200"] = want


def test_device_form_on_another_stream_equals_the_host_form(E):
    import torch

    s = triangle(E)
    x0, p0, t = _batch200()
    want = _CACHE.get("batch200") or result_bytes(s.seek_targets(x0, [3], p0, REC_C, t, want_trace=True))
    dx0, dp0, dt = (torch.from_numpy(a).cuda() for a in (x0, p0, t))
    out = lambda n: torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")  # noqa: E731
    params, x, m, info, trace = out(200 * 8), out(200 * 6 * 8), out(200 * 8), out(200 * 48), out(200 * 41 * 8)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call():
        with torch.cuda.stream(stream):
            s.seek_targets_device(dx0.data_ptr(), [3], dp0.data_ptr(), REC_C, dt.data_ptr(), 200, params.data_ptr(), x.data_ptr(), m.data_ptr(),
                                  info.data_ptr(), trace.data_ptr(), config=E.SeekConfig(chunk=128), stream=stream.cuda_stream)

    _, stamps = _trace(E, call)
    stream.synchronize()
    assert [v.cpu().numpy().tobytes() for v in (params, x, m, info, trace)] == want
    # every round of both chunks was enqueued: 2 * 41 measure launches (and as many response launches) under one SEEK_LAUNCHED
    assert stamps.count(SEEK_LAUNCHED) == 1 and stamps.count(51) == 2 * 41 * 2, stamps.count(51)


# ---- 9. start failures ------------------------------------------------------------------------------------------------------------------
def test_start_failures_leave_the_neighbours_alone(E):
    s = triangle(E)
    x0 = np.tile(TRI_X0, (3, 1)) + np.array([[0.0], [1e-3], [0.0]])
    p0, t = np.array([[5.0], [9.0], [5.0]]), np.array([[6.0], [6.0], [5.5]])  # c = 9 against a + b = 7 does not assemble
    res = assert_is_the_chain(E, s, x0, [3], p0, REC_C, t, hi=[8.5])
    assert res.status.tolist() == [R.REACHED, R.START_FAILED, R.REACHED]
    assert res.params[1, 0] == 8.5 and res.x[1].tobytes() == x0[1].tobytes() and np.isnan(res.m[1]).all()  # (the clamped params0)
    assert np.isnan([res.cost0[1], res.cost[1], res.worst[1]]).all() and res.iterations[1] == 0 and np.isnan(res.cost_trace[1]).all()
    for b in (0, 2):
        solo = s.seek_targets(x0[b:b + 1], [3], p0[b:b + 1], REC_C, t[b:b + 1], E.SeekConfig(hi=[8.5]), want_trace=True)
        assert [v[0].tobytes() for v in (solo.params, solo.x, solo.m, solo.info, solo.cost_trace)] == \
               [v[b].tobytes() for v in (res.params, res.x, res.m, res.info, res.cost_trace)]
    # a record that is degenerate at the start of one system: a line from (1, 1) to (p4, 1), p4 = 1 puts its ends together
    values = np.array([0.3, 0.7, 1.0, 1.0, 2.0, 1.0])
    f = E.System(O.stack([O.fixed(v, float(values[v])) for v in range(6)]), 6)
    recs = O.stack([O.point_line_distance((0, 1), (2, 3), (4, 5), 0.0), O.fixed(0, 0.0)])
    x0 = np.tile(values, (2, 1))
    x0[1, 4] = 1.0
    p0 = x0[:, [0, 4]].copy()
    t = np.tile([f.measure(x0[:1], recs)[0, 0], 0.5], (2, 1))  # (the distance as it is -- neither dimension moves it -- and x of the point)
    res = assert_is_the_chain(E, f, x0, [0, 4], p0, recs, t, weight=[1.0, 1.0])
    assert res.status[1] == R.START_FAILED and res.status[0] != R.START_FAILED, res.info
    assert res.params[1].tobytes() == p0[1].tobytes() and res.x[1].tobytes() == x0[1].tobytes() and np.isnan(res.m[1]).all()
    # with weight 0 the degenerate record is reported, not sought: the same start is fine
    res = assert_is_the_chain(E, f, x0, [0, 4], p0, recs, t, weight=[0.0, 1.0])
    assert res.status.tolist() == [R.REACHED, R.REACHED], res.info


# ---- 10. argument errors: the return code, no output touched, nothing launched -------------------------------------------------------
N20 = 20


def _error_case(E, what):
    """The arguments of a legal host call on a 20-variable Fixed system (17 dimensions need 17 driven constraints), one thing wrong."""
    if "s20" not in _CACHE:
        cons = [O.fixed(v, 1.0 + v) for v in range(N20)] + [O.vertical((0, 1), (2, 3))]  # (the last one has no parameter)
        _CACHE["s20"] = E.System(O.stack(cons), N20)
    two = O.stack([O.fixed(0, 0.0), O.distance((0, 1), (2, 3), 0.0)])
    a = dict(sys=_CACHE["s20"], x0=np.tile(1.0 + np.arange(N20), (3, 1)), positions=np.arange(4, dtype=np.uint32), params0=np.ones((3, 4)),
             records=two, targets=np.ones((3, 2)), batch=3, cfg={}, n_param=None, n_meas=None, null=())
    bad = {
        "17 dimensions": (dict(positions=np.arange(17, dtype=np.uint32), params0=np.ones((3, 17))), ERR_TOO_LARGE),
        "65 records": (dict(records=O.stack([O.fixed(i % N20, 0.0) for i in range(65)]), targets=np.ones((3, 65))), ERR_TOO_LARGE),
        "record not measurable": (dict(records=O.stack([O.fixed(0, 0.0), O.vertical((0, 1), (2, 3))])), ERR_INVALID_ARGUMENT),
        "record id >= n_vars": (dict(records=O.stack([O.fixed(0, 0.0), O.distance((0, 1), (2, N20), 0.0)])), ERR_INVALID_ARGUMENT),
        "position without a parameter": (dict(positions=np.array([0, 1, 2, N20], np.uint32)), ERR_INVALID_ARGUMENT),
        "position listed twice": (dict(positions=np.array([0, 1, 2, 1], np.uint32)), ERR_INVALID_ARGUMENT),
        "lo > hi": (dict(cfg=dict(lo=[0.0, 2.0, 0.0, 0.0], hi=[1.0, 1.0, 1.0, 1.0])), ERR_INVALID_ARGUMENT),
        "negative weight": (dict(cfg=dict(weight=[1.0, -1.0])), ERR_INVALID_ARGUMENT),
        "non-finite weight": (dict(cfg=dict(weight=[np.inf, 1.0])), ERR_INVALID_ARGUMENT),
        "negative tol": (dict(cfg=dict(tol=[-1e-6, 1e-6])), ERR_INVALID_ARGUMENT),
        "non-finite tol": (dict(cfg=dict(tol=[np.nan, 1e-6])), ERR_INVALID_ARGUMENT),
        "negative scale": (dict(cfg=dict(scale=[1.0, -1.0, 1.0, 1.0])), ERR_INVALID_ARGUMENT),
        "zero scale": (dict(cfg=dict(scale=[1.0, 0.0, 1.0, 1.0])), ERR_INVALID_ARGUMENT),
        "non-finite scale": (dict(cfg=dict(scale=[1.0, np.inf, 1.0, 1.0])), ERR_INVALID_ARGUMENT),
        "non-finite target": (dict(targets=np.array([[1.0, 1.0], [1.0, np.nan], [1.0, 1.0]])), ERR_INVALID_ARGUMENT),
        "mu_up <= 1": (dict(cfg=dict(mu_up=1.0)), ERR_INVALID_ARGUMENT),
        "mu_down >= 1": (dict(cfg=dict(mu_down=1.0)), ERR_INVALID_ARGUMENT),
        "x0 NULL": (dict(null=("x0",)), ERR_INVALID_ARGUMENT),
        "positions NULL": (dict(positions=None, n_param=4), ERR_INVALID_ARGUMENT),
        "params0 NULL": (dict(null=("params0",)), ERR_INVALID_ARGUMENT),
        "records NULL": (dict(records=None, n_meas=2), ERR_INVALID_ARGUMENT),
        "targets NULL": (dict(null=("targets",)), ERR_INVALID_ARGUMENT),
        "params_out NULL": (dict(null=("params_out",)), ERR_INVALID_ARGUMENT),
        "x_out NULL": (dict(null=("x_out",)), ERR_INVALID_ARGUMENT),
        "m_out NULL": (dict(null=("m_out",)), ERR_INVALID_ARGUMENT),
        "info_out NULL": (dict(null=("info_out",)), ERR_INVALID_ARGUMENT),
    }
    change, code = bad[what] if what else ({}, 0)
    a.update(change)
    return a, code


ERROR_CASES = ["17 dimensions", "65 records", "record not measurable", "record id >= n_vars", "position without a parameter",
               "position listed twice", "lo > hi", "negative weight", "non-finite weight", "negative tol", "non-finite tol", "negative scale",
               "zero scale", "non-finite scale", "non-finite target", "mu_up <= 1", "mu_down >= 1", "x0 NULL", "positions NULL", "params0 NULL",
               "records NULL", "targets NULL", "params_out NULL", "x_out NULL", "m_out NULL", "info_out NULL"]


def _raw_host_call(E, a, outputs):
    n_param = a["n_param"] if a["n_param"] is not None else len(a["positions"])
    n_meas = a["n_meas"] if a["n_meas"] is not None else len(a["records"])
    c, keep = E.SeekConfig(**a["cfg"])._c(n_param, n_meas)
    ptr = lambda name, v: v.ctypes.data if v is not None and name not in a["null"] else None  # noqa: E731
    names = ("params_out", "x_out", "m_out", "info_out", "trace")
    rc = E.lib().ezpz_system_seek_targets(a["sys"]._h, ptr("x0", a["x0"]), ptr("positions", a["positions"]), n_param, ptr("params0", a["params0"]),
                                          ptr("records", a["records"]), n_meas, ptr("targets", a["targets"]), a["batch"], C.byref(c),
                                          *(ptr(n, o) for n, o in zip(names, outputs)))
    del keep
    return rc


def _outputs():
    return [np.full(n, 0xA5, np.uint8) for n in (3 * 17 * 8, 3 * N20 * 8, 3 * 65 * 8, 3 * 48, 3 * 41 * 8)]


@pytest.mark.parametrize("what", ERROR_CASES)
def test_argument_errors(E, what):
    outputs = _outputs()
    a, code = _error_case(E, what)
    rc, stamps = _trace(E, lambda: _raw_host_call(E, a, outputs))
    assert rc == code and not set(stamps) - COLD_STAMPS, (what, rc, stamps)
    assert all(np.all(o == 0xA5) for o in outputs), what


def test_the_legal_call_of_the_error_cases_and_the_empty_ones(E):
    a, _ = _error_case(E, None)
    outputs = _outputs()
    rc, stamps = _trace(E, lambda: _raw_host_call(E, a, outputs))
    assert rc == 0 and SEEK_LAUNCHED in stamps and 51 in stamps, (rc, stamps)
    info = outputs[3].view(R.INFO_DTYPE)
    assert np.all(info["status"] <= R.START_FAILED)
    # batch == 0, n_param == 0 or n_meas == 0: EZPZ_OK, nothing written, nothing launched -- but still an error where the request is wrong
    for empty in (dict(batch=0), dict(positions=np.zeros(0, np.uint32)), dict(records=O.stack([O.fixed(0, 0.0)])[:0])):
        b = dict(a)
        b.update(empty)
        outputs = _outputs()
        rc, stamps = _trace(E, lambda: _raw_host_call(E, b, outputs))
        assert rc == 0 and not set(stamps) - COLD_STAMPS and all(np.all(o == 0xA5) for o in outputs), empty
        b["cfg"] = dict(mu_up=0.5)
        assert _raw_host_call(E, b, outputs) == ERR_INVALID_ARGUMENT


def test_device_form_argument_error_touches_nothing(E):
    import torch

    s = triangle(E)
    x0, p0, t = (torch.from_numpy(a).cuda() for a in (TRI_X0[None, :].copy(), np.array([[5.0]]), np.array([[6.0]])))
    outs = [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (8, 48, 8, 48)]
    torch.cuda.synchronize()

    def call():
        with pytest.raises(E.NonLinearSystemError):
            s.seek_targets_device(x0.data_ptr(), [3], p0.data_ptr(), REC_C, t.data_ptr(), 1, *(o.data_ptr() for o in outs),
                                  config=E.SeekConfig(lo=[2.0], hi=[1.0]))

    _, stamps = _trace(E, call)
    torch.cuda.synchronize()
    assert not set(stamps) - COLD_STAMPS and all(bool((o == 0x5A).all()) for o in outs)


# ---- 11. the fronts as a composition ------------------------------------------------------------------------------------------------
def test_fronts_routes_as_a_composition(E):
    s = E.System(TRI, 6, team_size=E.TEAM_FRONTS)
    info = s.info()
    assert info["front_max_batch"] == 0xFFFFFFFF and info["front_workgroups"] == 1, info  # (one workgroup per system: what this case is for)
    s.set_params_route("fronts")
    s.set_sensitivity_route("fronts")
    t = np.array([[5.0], [6.0], [8.0]])
    res = assert_is_the_chain(E, s, np.tile(TRI_X0, (3, 1)), [3], np.full((3, 1), 5.0), REC_C, t, max_iterations=12)
    assert res.status[0] == R.REACHED and res.status[1] == R.REACHED and res.status[2] != R.REACHED, res.info
