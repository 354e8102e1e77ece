"""GPU tests (-m gpu) of the redundancy analysis (ezpz_system_redundancy, csrc/redundancy.hip.hpp) against its numpy restatement
(tests/redundancy_ref.py): statuses, rank and conflict groups EQUAL the reference's on every system.  The inputs are held to
margins around the tolerances by tests/test_redundancy_cpu.py, so equality is not a matter of rounding.  The cases cover the three
placements: one lane per component (one variable, every kind, the block system with and without groups), one workgroup per system
with its workspace in LDS (the rectangle, the 24-point sketches: more and fewer rows than variables) and in global memory (the
150-point sketch).

The drawn inputs of tests/redundancy_ref.py reach what the named cases do not: several systems per LANE workgroup, a lane with two
components, components of every lane-group width in one TEAM system, a focus list that changes the placement, a second round of
the grid loop in each placement.  Every such test asserts the placement stamp (csrc/call_trace.hpp) it means to reach."""
import ctypes as C

import numpy as np
import pytest

import redundancy_ref as R

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
REDUNDANCY_PREPARED, REDUNDANCY_LAUNCHED = 40, 41
PLACED = {R.LANE: 42, R.TEAM_LDS: 43, R.TEAM_GLOBAL: 44}  # REDUNDANCY_PLACED_LANE, _TEAM_LDS, _TEAM_GLOBAL
KEYS = ("con_status", "row_status", "rank", "group")


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


_SYSTEMS = {}


def system_of(E, name):
    if name not in _SYSTEMS:
        c = R.case(name)
        _SYSTEMS[name] = E.System(c["recs"], c["n_vars"])
    return _SYSTEMS[name]


def assert_equals_reference(name, out, focus=True):
    for b, ref_b in enumerate(R.references(name)):
        assert np.array_equal(out["row_status"][b], ref_b["row_status"]), (name, b, out["row_status"][b], ref_b["row_status"])
        assert np.array_equal(out["con_status"][b], ref_b["con_status"]), (name, b)
        assert int(out["rank"][b]) == ref_b["rank"], (name, b)
        if focus and R.case(name)["focus"]:
            assert np.array_equal(out["group"][b], ref_b["group"]), (name, b, [np.nonzero(g)[0] for g in out["group"][b]],
                                                                     [np.nonzero(g)[0] for g in ref_b["group"]])


@pytest.mark.parametrize("name", list(R.CASES))
def test_equals_reference(E, name):
    """With the case's focus list (conflict groups, the factor L kept) and without it (the smaller workspace)."""
    c = R.case(name)
    s = system_of(E, name)
    out = s.redundancy(c["x"], focus=c["focus"], want_rows=True)
    assert_equals_reference(name, out)
    plain = s.redundancy(c["x"], want_rows=True)
    assert "group" not in plain
    assert_equals_reference(name, plain, focus=False)
    # only what was asked for: no row statuses, the same constraint statuses
    short = s.redundancy(c["x"])
    assert "row_status" not in short and np.array_equal(short["con_status"], out["con_status"]) and np.array_equal(short["rank"], out["rank"])


def test_changed_tolerances(E):
    """The tolerances are arguments: a conflict bar above the rectangle's half unit calls the long side redundant, a group bar of one
    half (the shares are one or nothing) keeps the group -- as the reference does with the same bars."""
    name = "rectangle:side_conflict"
    c, s = R.case(name), system_of(E, name)
    for cfg in (dict(conflict_tol=0.75), dict(group_tol=0.5)):
        out = s.redundancy(c["x"], focus=c["focus"], want_rows=True, config=E.RedundancyConfig(**cfg))
        ref = R.analyse(c["recs"], c["n_vars"], c["x"][0], c["focus"], **cfg)
        for key in ("row_status", "con_status", "group"):
            assert np.array_equal(out[key][0], ref[key]), (cfg, key, out[key][0], ref[key])
    assert s.redundancy(c["x"], config=E.RedundancyConfig(conflict_tol=0.75))["con_status"][0].tolist() == [0] * 8 + [2]


def test_block_system_batches_and_order(E):
    """130 systems are not a multiple of the lanes' group of systems; the same systems one by one, as batches of 7 and in reversed
    order give the same outputs, byte for byte."""
    name = "blocks"
    c, s = R.case(name), system_of(E, name)
    x = c["x"]
    keys = ("con_status", "row_status", "rank", "group")
    whole = s.redundancy(x, focus=c["focus"], want_rows=True)
    back = s.redundancy(x[::-1], focus=c["focus"], want_rows=True)
    for key in keys:
        assert whole[key].tobytes() == back[key][::-1].tobytes(), key
    for size in (1, 7):
        picks = [0, 63, 129] if size == 1 else [0, 119]
        for start in picks:
            part = s.redundancy(x[start:start + size], focus=c["focus"], want_rows=True)
            for key in keys:
                assert part[key].tobytes() == whole[key][start:start + size].tobytes(), (key, size, start)


@pytest.mark.parametrize("name", ["blocks", "sketch24", "sketch150"])
def test_run_to_run(E, name):
    c, s = R.case(name), system_of(E, name)
    a = s.redundancy(c["x"], focus=c["focus"], want_rows=True)
    b = s.redundancy(c["x"], focus=c["focus"], want_rows=True)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


def _trace(E, call):
    """The stamps of csrc/call_trace.hpp a call left (ids only)."""
    trace = np.zeros(64, dtype=np.uint64)
    E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
    try:
        call()
    finally:
        k = E.lib().ezpz_debug_call_trace(None, 0)
    return [int(v) for v in trace[:k:2]]


@pytest.mark.parametrize("name", ["blocks", "sketch24"])
def test_device_form(E, name):
    """Device pointers on a stream of the caller's: the host form's results; a call the system has seen only enqueues."""
    import torch

    c, s = R.case(name), system_of(E, name)
    x = np.ascontiguousarray(c["x"][:5])
    host = s.redundancy(x, focus=c["focus"], want_rows=True)
    n_cs, m, nf = len(c["recs"]), host["row_status"].shape[1], len(c["focus"])
    stream = torch.cuda.Stream()

    def call(focus):
        with torch.cuda.stream(stream):
            xd = torch.from_numpy(x).cuda()
            con = torch.full((len(x), n_cs), 9, dtype=torch.uint8, device="cuda")
            rows = torch.full((len(x), m), 9, dtype=torch.uint8, device="cuda")
            rank = torch.zeros(len(x), dtype=torch.int32, device="cuda")
            group = torch.full((len(x), len(focus), n_cs), 9, dtype=torch.uint8, device="cuda")
            s.redundancy_device(xd.data_ptr(), len(x), con.data_ptr(), rows.data_ptr(), rank.data_ptr(), focus, group.data_ptr(),
                                stream=stream.cuda_stream)
        stream.synchronize()
        return con.cpu().numpy(), rows.cpu().numpy(), rank.cpu().numpy().astype(np.uint32), group.cpu().numpy()

    con, rows, rank, group = call(c["focus"])
    assert np.array_equal(con, host["con_status"]) and np.array_equal(rows, host["row_status"])
    assert np.array_equal(rank, host["rank"]) and np.array_equal(group, host["group"])
    # another focus list is turned into its table first (behind the system's earlier launches); repeated, the call only enqueues
    other = list(c["focus"][:2][::-1])
    first = _trace(E, lambda: call(other))
    again = _trace(E, lambda: call(other))
    placed = PLACED[R.LANE if name == "blocks" else R.TEAM_LDS]
    assert first == [REDUNDANCY_PREPARED, REDUNDANCY_LAUNCHED, placed] and again == [REDUNDANCY_LAUNCHED, placed], (first, again)
    assert np.array_equal(call(other)[3], host["group"][:, [1, 0]])
    assert nf >= 2


def test_argument_errors_touch_nothing(E):
    """EZPZ_ERR_INVALID_ARGUMENT for every case of the header, outputs left as they were; batch == 0 is EZPZ_OK and writes nothing."""
    name = "rectangle:side_conflict"
    c, s = R.case(name), system_of(E, name)
    L = E.lib()
    x = np.ascontiguousarray(c["x"][:1])
    n_cs = len(c["recs"])
    con = np.full((1, n_cs), 77, np.uint8)
    rows = np.full((1, 10), 77, np.uint8)
    rank = np.full(1, 77, np.uint32)
    group = np.full((1, 2, n_cs), 77, np.uint8)
    focus = np.asarray([8, 6], np.uint32)
    from ezpz_amd._lib import CRedundancyConfig

    def call(x_=x, batch=1, cfg=None, con_=con, focus_=focus, n_focus=2, group_=group):
        return L.ezpz_system_redundancy(s._h, x_.ctypes.data if x_ is not None else None, batch, C.byref(cfg) if cfg is not None else None,
                                        con_.ctypes.data if con_ is not None else None, rows.ctypes.data, rank.ctypes.data,
                                        focus_.ctypes.data if focus_ is not None else None, n_focus,
                                        group_.ctypes.data if group_ is not None else None)

    bad = [dict(x_=None), dict(con_=None), dict(focus_=np.asarray([8, n_cs], np.uint32)), dict(focus_=np.asarray([6, 6], np.uint32)),
           dict(focus_=None), dict(group_=None)]
    for t in (-1e-6, float("nan"), float("inf")):
        for field in range(3):
            v = [1e-6, 1e-4, 1e-6]
            v[field] = t
            bad.append(dict(cfg=CRedundancyConfig(*v)))
    for kw in bad:
        assert call(**kw) == ERR_INVALID_ARGUMENT, kw
        assert np.all(con == 77) and np.all(rows == 77) and np.all(rank == 77) and np.all(group == 77), kw
    assert call(batch=0) == 0 and call(batch=0, x_=None, con_=None) == 0
    assert np.all(con == 77) and np.all(rows == 77) and np.all(rank == 77) and np.all(group == 77)
    # the device entry checks the same before it enqueues anything (null pointers stand for device memory here: never read)
    assert L.ezpz_system_redundancy_device(s._h, None, 1, None, None, None, None, None, 0, None, None) == ERR_INVALID_ARGUMENT
    assert L.ezpz_system_redundancy_device(s._h, None, 0, None, None, None, None, None, 0, None, None) == 0
    d = CRedundancyConfig()
    L.ezpz_default_redundancy_config(C.byref(d))
    assert (d.rank_tol, d.conflict_tol, d.group_tol) == (1e-6, 1e-4, 1e-6)
    assert call() == 0 and np.array_equal(con[0], R.references(name, 1)[0]["con_status"])


# ---- drawn inputs ---------------------------------------------------------------------------------------------------------------
def _placed(E, call, want):
    """The call's result; it stamped the placement `want` (one launch, stamped behind REDUNDANCY_LAUNCHED)."""
    out = {}
    stamps = [v for v in _trace(E, lambda: out.update(call())) if 40 <= v < 50]  # (a system's first call stamps its cold plan too)
    assert stamps[-2:] == [REDUNDANCY_LAUNCHED, PLACED[want]] and stamps[:-2] in ([], [REDUNDANCY_PREPARED]), (stamps, want)
    return out


def _expected_placement(name, with_focus):
    c = R.case(name)
    return R.placement(c["recs"], c["n_vars"], with_focus)[0]


_FUZZ_PLACED = {}


def _fuzz_calls(E, name):
    c, s = R.case(name), system_of(E, name)
    with_l, without = _expected_placement(name, True), _expected_placement(name, False)
    out = _placed(E, lambda: s.redundancy(c["x"], focus=c["focus"], want_rows=True), with_l)
    plain = _placed(E, lambda: s.redundancy(c["x"], want_rows=True), without)
    short = _placed(E, lambda: s.redundancy(c["x"]), without)
    _FUZZ_PLACED[name] = {with_l, without}
    return out, plain, short


@pytest.mark.parametrize("name", R.FUZZ_NAMES)
def test_fuzz_equals_reference(E, name):
    """A drawn mosaic: components of different sizes in one system, their rows interleaved in request order.  With its focus list,
    without it and without rows, each call where test_redundancy_cpu.py says it runs."""
    out, plain, short = _fuzz_calls(E, name)
    assert_equals_reference(name, out)
    assert "group" not in plain
    assert_equals_reference(name, plain, focus=False)
    assert "row_status" not in short and np.array_equal(short["con_status"], out["con_status"]) and np.array_equal(short["rank"], out["rank"])


def test_fuzz_reaches_every_placement(E):
    for name in R.FUZZ_NAMES:
        if name not in _FUZZ_PLACED:
            _fuzz_calls(E, name)
    assert set().union(*_FUZZ_PLACED.values()) == set(PLACED)
    moved = [n for n in R.FUZZ_NAMES if _FUZZ_PLACED[n] == {R.LANE, R.TEAM_LDS}]
    assert len(moved) >= 3  # the focus list alone moved these from LANE to TEAM


@pytest.mark.parametrize("name", ["all_kinds:repeated", "all_kinds:moved"])
def test_all_kinds_with_a_focus_list(E, name):
    """Every flagged constraint in the focus list: the factor L no longer fits a lane, so 27 small components of every kind run one
    behind the other in a workgroup -- with the statuses of the LANE call."""
    c, s = R.case(name), system_of(E, name)
    focus = np.nonzero(R.references(name)[0]["con_status"] >= R.REDUNDANT)[0].tolist()
    assert len(focus) == 25
    out = _placed(E, lambda: s.redundancy(c["x"], focus=focus, want_rows=True), R.TEAM_LDS)
    lane = _placed(E, lambda: s.redundancy(c["x"], want_rows=True), R.LANE)
    for b in range(len(c["x"])):
        ref = R.analyse(c["recs"], c["n_vars"], c["x"][b], focus)
        assert not R.within_margins(ref)
        for key in KEYS:
            got = int(out[key][b]) if key == "rank" else out[key][b]
            assert np.array_equal(got, ref[key]), (name, b, key)
    for key in ("con_status", "row_status", "rank"):
        assert out[key].tobytes() == lane[key].tobytes(), key


def _assert_systems_equal_reference(name, out, focus=True):
    for b, ref_b in enumerate(R.references(name)):
        for key in KEYS if focus else KEYS[:3]:
            got = int(out[key][b]) if key == "rank" else out[key][b]
            assert np.array_equal(got, ref_b[key]), (name, b, key, got, ref_b[key])


@pytest.mark.parametrize("name", list(R.PAIRS))
def test_lane_groups_of_systems(E, name):
    """G systems per workgroup that differ from one another: batches of G - 1, G, G + 1 and 3 G + 1 (a partial group, a full one, a
    full one with a tail in the next workgroup, three and a tail), every system against the reference; the smaller batches, a
    batch that starts in the middle and the reversed batch byte for byte.  150 components: G = 1, lanes 0 .. 21 take two."""
    c, s = R.case(name), system_of(E, name)
    _, G, _, _ = R.placement(c["recs"], c["n_vars"], True)
    x = c["x"]
    assert len(x) == (3 * G + 1 if name != "pairs:150" else 3)
    whole = _placed(E, lambda: s.redundancy(x, focus=c["focus"], want_rows=True), R.LANE)
    _assert_systems_equal_reference(name, whole)
    _assert_systems_equal_reference(name, _placed(E, lambda: s.redundancy(x, want_rows=True), R.LANE), focus=False)
    assert len({row.tobytes() for row in whole["con_status"]}) > 1  # (systems that differ)
    for nb in sorted({G - 1, G, G + 1} - {0, len(x)}) if name != "pairs:150" else [1]:
        for start in sorted({0, 1, len(x) - nb}):
            part = _placed(E, lambda: s.redundancy(x[start:start + nb], focus=c["focus"], want_rows=True), R.LANE)
            for key in KEYS:
                assert part[key].tobytes() == whole[key][start:start + nb].tobytes(), (key, nb, start)
    back = s.redundancy(x[::-1], focus=c["focus"], want_rows=True)
    for key in KEYS:
        assert back[key][::-1].tobytes() == whole[key].tobytes(), key


@pytest.mark.parametrize("name,batch,placed,grid", [("grid:lane", 65536 + 3, R.LANE, 65536), ("grid:rectangle", 65536 + 3, R.TEAM_LDS, 65536),
                                                    ("grid:sketch45", 1024 + 5, R.TEAM_GLOBAL, 1024)])
def test_second_round_of_the_grid_loop(E, name, batch, placed, grid):
    """More systems than workgroups: the last few are a workgroup's second round, behind the reset of its rank counters, and (global
    workspace) in the workspace its first system left.  x repeats a period of systems that differ, of a length that does not
    divide the grid; the first period against the reference, every later system byte for byte equal to its place in the period."""
    c, s = R.case(name), system_of(E, name)
    period = len(c["x"])
    assert grid % period != 0 and R.placement(c["recs"], c["n_vars"], True)[:2] == (placed, 1)
    pick = np.arange(batch) % period
    out = _placed(E, lambda: s.redundancy(c["x"][pick], focus=c["focus"], want_rows=True), placed)
    _assert_systems_equal_reference(name, {key: out[key][:period] for key in KEYS})
    for key in KEYS:
        assert out[key][-3:].tobytes() == out[key][:period][pick[-3:]].tobytes(), (name, key, out[key][-3:])
        assert out[key].tobytes() == out[key][:period][pick].tobytes(), (name, key)


def test_placement_does_not_matter(E):
    """The records of pairs:3 analysed alone (LANE) and as one part of a mosaic whose largest part is a 24-point sketch (TEAM):
    the same statuses, and the same groups at the records' new positions -- nothing outside them."""
    alone, inside = R.case("pairs:3"), R.case("pairs:3:embedded")
    a = _placed(E, lambda: system_of(E, "pairs:3").redundancy(alone["x"], focus=alone["focus"], want_rows=True), R.LANE)
    b = _placed(E, lambda: system_of(E, "pairs:3:embedded").redundancy(inside["x"], focus=inside["focus"], want_rows=True), R.TEAM_LDS)
    _assert_systems_equal_reference("pairs:3", a)
    _assert_systems_equal_reference("pairs:3:embedded", b)
    at = inside["at"]
    assert np.array_equal(b["con_status"][:, at], a["con_status"])
    assert np.array_equal(b["group"][:, :, at], a["group"])
    assert b["group"].sum() == a["group"].sum() and a["group"].any()


@pytest.mark.parametrize("name", ["pairs:30", "fuzz:4", "fuzz:1", "fuzz:9"])
def test_weights_and_variable_numbers_do_not_matter(E, name):
    """Every weight times 1e-3 and times 7 (include/ezpz_amd.h: a weight does not change a class), and the variables renumbered
    (the components come in another order, other sizes behind one another in the workspace): all outputs stay as they are."""
    c = R.case(name)
    base = system_of(E, name).redundancy(c["x"], focus=c["focus"], want_rows=True)
    _assert_systems_equal_reference(name, base)
    for scale in (1e-3, 7.0):
        recs = c["recs"].copy()
        recs["weight"] = recs["weight"] * scale
        out = E.System(recs, c["n_vars"]).redundancy(c["x"], focus=c["focus"], want_rows=True)
        for key in KEYS:
            assert out[key].tobytes() == base[key].tobytes(), (name, scale, key)
    perm = np.random.default_rng(8).permutation(c["n_vars"])
    x = np.empty_like(c["x"])
    x[:, perm] = c["x"]
    for focus in (c["focus"], None):
        out = E.System(R.relabel(c["recs"], perm), c["n_vars"]).redundancy(x, focus=focus, want_rows=True)
        for key in KEYS if focus else KEYS[:3]:
            assert out[key].tobytes() == base[key].tobytes(), (name, "renumbered", key)


def _device_call(s, x, n_cs, focus):
    """con_status and group of the device form on a stream of the caller's, without the optional outputs."""
    import torch

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        con = torch.full((len(x), n_cs), 9, dtype=torch.uint8, device="cuda")
        group = torch.full((len(x), len(focus), n_cs), 9, dtype=torch.uint8, device="cuda")
        s.redundancy_device(xd.data_ptr(), len(x), con.data_ptr(), 0, 0, focus, group.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return con.cpu().numpy(), group.cpu().numpy()


@pytest.mark.parametrize("name", ["pairs:30", "fuzz:4"])
def test_device_form_without_rows_and_rank(E, name):
    """row_status_dev and rank_dev null: the row statuses go to the plan's scratch, nobody gets a rank -- the host form's constraint
    statuses and groups.  (pairs:30: four systems per workgroup.)"""
    c, s = R.case(name), system_of(E, name)
    host = s.redundancy(c["x"], focus=c["focus"], want_rows=True)
    _assert_systems_equal_reference(name, host)
    con, group = _device_call(s, c["x"], len(c["recs"]), c["focus"])
    assert np.array_equal(con, host["con_status"]) and np.array_equal(group, host["group"])


def test_device_form_scratch_grows(E):
    """A batch of 2, then 50, then 2 on a system of its own, the row statuses in the plan's scratch: the first call builds the tables,
    the second has to replace the scratch (both prepare), the third only launches.  Each gives the host form's statuses."""
    name = "pairs:30"
    c = R.case(name)
    s = E.System(c["recs"], c["n_vars"])
    x = c["x"][np.arange(50) % len(c["x"])]
    want = system_of(E, name).redundancy(x, focus=c["focus"])["con_status"]
    placed = PLACED[R.LANE]
    for nb, stamps in ((2, [REDUNDANCY_PREPARED, REDUNDANCY_LAUNCHED, placed]), (50, [REDUNDANCY_PREPARED, REDUNDANCY_LAUNCHED, placed]),
                       (2, [REDUNDANCY_LAUNCHED, placed])):
        got = []
        assert _trace(E, lambda: got.extend(_device_call(s, x[:nb], len(c["recs"]), c["focus"]))) == stamps, (nb, stamps)
        assert np.array_equal(got[0], want[:nb]), nb
