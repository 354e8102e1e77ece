"""GPU tests (-m gpu) of the redundancy analysis (ezpz_system_redundancy, csrc/redundancy.hip.hpp) against its numpy restatement
(tests/redundancy_ref.py): statuses, rank and conflict groups EQUAL the reference's on every system.  The inputs are held to
margins around the tolerances by tests/test_redundancy_cpu.py, so equality is not a matter of rounding.  The cases cover the three
placements: one lane per component (one variable, every kind, the block system with and without groups), one workgroup per system
with its workspace in LDS (the rectangle, the 24-point sketches: more and fewer rows than variables) and in global memory (the
150-point sketch)."""
import ctypes as C

import numpy as np
import pytest

import redundancy_ref as R

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
REDUNDANCY_PREPARED, REDUNDANCY_LAUNCHED = 40, 41


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
    assert first == [REDUNDANCY_PREPARED, REDUNDANCY_LAUNCHED] and again == [REDUNDANCY_LAUNCHED], (first, again)
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
