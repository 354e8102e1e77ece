"""The `_device` entries where two calls on ONE EzpzSystem meet (-m gpu).  Every analysis and driven entry keeps per-system scratch
on the device; what keeps two launches apart is a handful of events on the host side, which no
one-stream comparison with the oracle can see.

A. ezpz_system_freedom_batch_device on a stream of the test's own, on the smallest system of each placement: bytewise the host
   entry's mask and participation, the oracle's sets, the counts, guard regions, the calls that write nothing.
B. Two streams on one system: a long call and right behind it a short call of other values on another stream give the bits of
   the same calls made alone, and the short one does not finish first; another `positions` / focus list waits on the host for the
   launch that reads the first; a host form behind a device call in flight; a plain solve beside a params call on the shared
   global workspace; redundancy and FreedomAnalysis first used in either order.

All of these entries are bit-deterministic, so a correct ordering gives exactly the bits of the calls made alone: the tests
cannot fail by rounding or timing, only miss -- which is what the asserted preconditions (a long call at least ten times as long
as everything the short one needs) are for."""
import time

import numpy as np
import pytest

import device_entries_common as D
import redundancy_ref as RR
import sensitivity_ref as SR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
REDUNDANCY_LAUNCHED, REDUNDANCY_PLACED_TEAM_LDS = 41, 43
KIB = 1024


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


@pytest.fixture
def pivoted_qr(monkeypatch):
    """The host entry takes the pivoted QR too (tests/test_gpu_parity.py: a system the fronts serve would go to the probes)."""
    monkeypatch.setenv("EZPZ_FREEDOM_PROBES", "0")


# ---- A. freedom_batch_device against the host entry and the oracle ----------------------------------------------------------------
GUARD = 64  # elements of the pattern on either side of every output
MASK_PATTERN, PART_PATTERN, COUNT_PATTERN = 9, 7.0, 9


class _Guarded:
    """mask / participation / counts inside guard regions of their patterns."""

    def __init__(self, torch, batch, n):
        self.batch, self.n = batch, n
        self.mask = torch.full((2 * GUARD + batch * n,), MASK_PATTERN, dtype=torch.uint8, device="cuda")
        self.part = torch.full((2 * GUARD + batch * n,), PART_PATTERN, dtype=torch.float64, device="cuda")
        self.count = torch.full((2 * GUARD + batch,), COUNT_PATTERN, dtype=torch.int32, device="cuda")

    def ptr(self, t):
        return t.data_ptr() + GUARD * t.element_size()

    def host(self):
        m, p, c = self.mask.cpu().numpy(), self.part.cpu().numpy(), self.count.cpu().numpy()
        for a, pattern in ((m, MASK_PATTERN), (p, PART_PATTERN), (c, COUNT_PATTERN)):
            assert np.all(a[:GUARD] == pattern) and np.all(a[-GUARD:] == pattern), "a guard region was written"
        shape = (self.batch, self.n)
        return m[GUARD:-GUARD].reshape(shape), p[GUARD:-GUARD].reshape(shape), c[GUARD:-GUARD].astype(np.int64)


def _freedom_on_a_stream(torch, s, x, stream, with_part=True):
    batch, n = x.shape
    out = _Guarded(torch, batch, n)
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()  # (the fills and the copy ran on torch's current stream)
    s.freedom_batch_device(xd.data_ptr(), batch, out.ptr(out.mask), out.ptr(out.part) if with_part else 0, out.ptr(out.count),
                           stream=stream.cuda_stream)
    stream.synchronize()
    return out.host()


def _assert_placement(E, name, s):
    """The placement the case is named after, from build_freedom's rule applied to the system's own Jacobian pattern."""
    ncomp, ws, max_n = D.freedom_rule(E, s)
    group = 1 if ncomp >= 128 else 128 // ncomp
    head = (2 * group + (group + 1) // 2 + 16) * 8
    if name == "lane":
        assert ws <= 64 and ncomp >= 128 and group == 1, (ncomp, ws)
    elif name == "lane_groups":
        assert ws <= 64 and group == 4, (ncomp, ws)
    elif name == "lds":
        assert ws > 64 and head + ws * 8 <= 128 * KIB and s.n_vars == 48, (ncomp, ws)
    elif name == "global":
        assert max_n < 96 and ws * 8 > 128 * KIB and s.n_vars == 88, (ncomp, ws, max_n)
    else:
        assert max_n >= 96 and ws * 8 > 128 * KIB and s.n_vars == 240, (ncomp, ws, max_n)
    return head


# The fused / unfused split: one launch up to 64 systems AND batch * n_cons <= 4096 on the LDS layouts.  "lane" has 231
# constraints: 17 systems are fused, 18 are not, by the product alone; "lds" has 45: 3 fused, 65 and 70 unfused by the count alone
# (70 x 45 is 3150: on this system the product cannot decide below 65 systems), 92 unfused by both.
FREEDOM_CASES = [("lane", 5), ("lane", 17), ("lane", 18), ("lane", 130), ("lane_groups", 5), ("lane_groups", 130), ("lds", 3),
                 ("lds", 65), ("lds", 70), ("lds", 92), ("global", 3), ("wide", 3)]


@pytest.mark.parametrize("name, batch", FREEDOM_CASES, ids=["%s-%d" % c for c in FREEDOM_CASES])
def test_freedom_device_equals_the_host_entry_and_the_oracle(E, pivoted_qr, name, batch):
    import torch

    s, recs, n, values = D.freedom_system(E, name)
    _assert_placement(E, name, s)
    n_cons = s.info()["n_constraints"]
    assert n_cons == len(recs)
    if name == "lane":
        assert 17 * n_cons <= 4096 < 18 * n_cons
    if name == "lds":
        assert 64 * n_cons <= 4096 < 92 * n_cons
    if name == "lane_groups":
        assert 130 % 4 != 0
    x = values(batch)
    stream = torch.cuda.Stream()
    mask, part, count = _freedom_on_a_stream(torch, s, x, stream)
    host_mask, host_part = s.freedom_batch(x)
    assert mask.tobytes() == host_mask.tobytes(), name
    assert part.tobytes() == host_part.tobytes(), (name, float(np.abs(part - host_part).max()))
    assert mask.any() and not mask.all()
    assert np.array_equal(count, mask.sum(axis=1)), (count, mask.sum(axis=1))
    _, J, _ = s.eval_batch(x)
    atol = 1e-8 if name == "wide" else 1e-9  # (test_gpu_parity.py: 1e-8 on the 240-variable chain)
    for b in range(batch):
        under, want = O.freedom_analysis_dense(J[b])
        assert np.nonzero(mask[b])[0].tolist() == under, (name, b)
        assert np.allclose(part[b], want, atol=atol), (name, b, float(np.abs(part[b] - want).max()))
    assert all(0 < int(c) < n for c in count)  # at least one free and one held variable in every system
    if name == "wide":
        return  # (once, on one stream: the launch the host test makes)
    # without a participation buffer of the caller's (the system's own takes its place): the same mask and counts
    mask2, part2, count2 = _freedom_on_a_stream(torch, s, x, stream, with_part=False)
    assert mask2.tobytes() == mask.tobytes() and np.array_equal(count2, count) and np.all(part2 == PART_PATTERN)


def test_freedom_device_calls_that_write_nothing(E):
    import torch

    s, _, n, values = D.freedom_system(E, "lds")
    x = torch.from_numpy(values(3)).cuda()
    out = _Guarded(torch, 3, n)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    L = E.lib()
    args = lambda xp, batch, mp: (s._h, xp, batch, mp, out.ptr(out.part), out.ptr(out.count), stream.cuda_stream)
    assert L.ezpz_system_freedom_batch_device(*args(x.data_ptr(), 0, out.ptr(out.mask))) == 0
    assert L.ezpz_system_freedom_batch_device(*args(None, 0, None)) == 0
    assert L.ezpz_system_freedom_batch_device(*args(None, 3, out.ptr(out.mask))) == ERR_INVALID_ARGUMENT
    assert L.ezpz_system_freedom_batch_device(*args(x.data_ptr(), 3, None)) == ERR_INVALID_ARGUMENT
    assert L.ezpz_system_freedom_batch_device(None, x.data_ptr(), 3, out.ptr(out.mask), None, None, None) == ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.all(out.mask == MASK_PATTERN) and torch.all(out.part == PART_PATTERN) and torch.all(out.count == COUNT_PATTERN)


# ---- B. two streams on one system ---------------------------------------------------------------------------------------------------
def _alone(torch, call, stream):
    """The call made alone (after one warm-up: buffers grown, tables uploaded, kernels loaded): (milliseconds, its outputs)."""
    for _ in range(2):
        call.refill()
        torch.cuda.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        call.run(stream)
        end.record(stream)
        torch.cuda.synchronize()
    assert all(call.written()), call.written()
    return begin.elapsed_time(end), call.snapshot()


def _long_then_short(torch, a, b, what):
    """A on one stream, B right behind it on another with no host synchronisation between them."""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a_ms, a_ref = _alone(torch, a, s1)  # (A first: B's buffers fit what A grew)
    b_ms, b_ref = _alone(torch, b, s2)
    a.refill(), b.refill()
    end_a, end_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.run(s1)
    end_a.record(s1)
    b.run(s2)
    end_b.record(s2)
    gap_ms = (time.perf_counter() - t0) * 1e3  # from before A's enqueue until B and its event are enqueued
    torch.cuda.synchronize()
    print("%s: A alone %.3f ms (%d systems), B alone %.3f ms (%d systems), host gap %.3f ms" % (what, a_ms, a.batch, b_ms, b.batch, gap_ms))
    same_a, same_b, lead_ms = a.equals(a_ref), b.equals(b_ref), end_a.elapsed_time(end_b)
    # the precondition: without an ordering, B would be done long before A
    assert a_ms >= 10.0 * (gap_ms + b_ms), (what, a_ms, b_ms, gap_ms)
    assert lead_ms >= 0.0, (what, "B finished %.3f ms before A" % -lead_ms, "A's outputs as alone", same_a, "B's", same_b)
    assert all(same_a), (what, "A", same_a)
    assert all(same_b), (what, "B", same_b)
    return a_ms


LONG_SHORT = sorted(D.BATCHES)


@pytest.mark.parametrize("entry, placement", LONG_SHORT, ids=["%s-%s" % c for c in LONG_SHORT])
def test_long_call_then_short_call(E, monkeypatch, entry, placement):
    """Measured on an MI355X (A alone, B alone, host gap between the enqueues; ms):
    redundancy: blocks 1.855 / 0.043 / 0.054; sketch24 16.669 / 0.697 / 0.052; sketch150 254.212 / 18.583 / 0.052 (one system of B
    alone takes 18.6 ms on its one workgroup, so A cannot stay under 50 ms and be ten times as long)
    sensitivity: massive40 3.061 / 0.047 / 0.066; sketch150 41.165 / 2.298 / 0.063; hub512 72.197 / 4.968 / 0.086 (B: 5 ms for one
    system, so A is above 50 ms here too)
    params: sub-wavefront teams 2.647 / 0.035 / 0.035; barrier workgroup 3.615 / 0.100 / 0.076; record walk 19.645 / 0.842 / 0.035;
    global workspace 22.919 / 0.823 / 0.068; fronts 5.958 / 0.066 / 0.034
    sweep: sub-wavefront teams 2.866 / 0.057 / 0.034; barrier workgroup 3.903 / 0.176 / 0.040; record walk 42.779 / 2.482 / 0.032;
    global workspace 32.715 / 1.924 / 0.064; fronts 6.366 / 0.127 / 0.060
    freedom: lane 1.375 / 0.019 / 0.024; lds 9.162 / 0.213 / 0.025; global 20.213 / 1.293 / 0.030
    On builds without the entry's ordering (the event's wait taken out; FreedomAnalysis before it had one) the first case of each
    entry fails its second assertion: B ends 1.3 ... 3.0 ms before A.  (The bytes were still those of the calls alone in those
    runs -- B's few systems touch the head of the shared buffers, which A had used by then: the race shows only by luck, which is
    why the order of the two ends is asserted as well.)
    """
    import torch

    s, a, b = D.two_calls(E, entry, placement, monkeypatch.setenv)
    _long_then_short(torch, a, b, "%s, %s" % (entry, placement))


def _trace(E, call):
    """The stamps of csrc/call_trace.hpp a call left (ids only)."""
    trace = np.zeros(64, dtype=np.uint64)
    E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
    try:
        call()
    finally:
        k = E.lib().ezpz_debug_call_trace(None, 0)
    return [int(v) for v in trace[:k:2]]


def _other_list_cases(E, entry, monkeypatch):
    """make() -> (system, A with list 1, B with list 2, B's list again as a call of A's size class) on a fresh system each time."""
    if entry == "redundancy":
        c = RR.case("sketch24")
        batch_a, batch_b = D.BATCHES[("redundancy", "sketch24")]
        other = list(c["focus"][:2][::-1])

        def make():
            s = E.System(c["recs"], c["n_vars"])
            return s, D.redundancy_call(s, c, batch_a, 101, c["focus"]), D.redundancy_call(s, c, batch_b, 202, other)
    elif entry == "sensitivity":
        # (sketch150: planning another list costs the host milliseconds, so A has to be the long one of the sensitivity cases;
        # a quarter of its parameters, so that 8192 systems' S stays at 1.5 GB)
        ref = SR.system("sketch150")
        batch_a, batch_b = D.BATCHES[("sensitivity", "sketch150")]
        first, other = np.arange(0, len(ref["pos"]), 4), np.arange(1, len(ref["pos"]), 8)

        def make():
            s = E.System(ref["recs"], ref["n_vars"])
            return (s, D.sensitivity_call(s, ref, batch_a, 101, ref["pos"][first], first),
                    D.sensitivity_call(s, ref, batch_b, 202, ref["pos"][other], other))
    else:
        recs, g, config, fresh = D.driven_shape(E, "barrier workgroup", monkeypatch.setenv)
        batch_a, batch_b = D.BATCHES[("params", "barrier workgroup")]
        pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)

        def make():
            s = fresh()
            return s, D.driven_call(E, s, recs, g, batch_a, 101), D.driven_call(E, s, recs, g, batch_b, 202, pos=pos[::3])
    return make


@pytest.mark.parametrize("entry", ["redundancy", "sensitivity", "params"])
def test_another_list_while_the_first_is_in_flight(E, monkeypatch, entry):
    """A call with another list replaces the table the launch in flight reads: it waits for that launch ON THE HOST first
    (KeptList::before_overwrite), so when it returns A has ended.  What makes that mean something: A alone takes at least three
    times as long as B's whole call does on an idle system (list change included)."""
    import torch

    make = _other_list_cases(E, entry, monkeypatch)
    # the references: each call as the first and only one on a fresh system
    refs = []
    for which in (1, 2):
        call = make()[which]
        call.refill()
        torch.cuda.synchronize()
        call.run(torch.cuda.Stream())
        torch.cuda.synchronize()
        refs.append(call.snapshot())
    s, a, b = make()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    _alone(torch, a, s1)
    _alone(torch, b, s2)  # (kernels loaded and buffers grown for both lists)
    a_ms, _ = _alone(torch, a, s1)
    t0 = time.perf_counter()
    b.run(s2)
    b_host_ms = (time.perf_counter() - t0) * 1e3  # B's call on an idle system, its list change included
    torch.cuda.synchronize()
    a.refill(), b.refill()
    torch.cuda.synchronize()
    end_a = torch.cuda.Event()
    a.run(s1)
    end_a.record(s1)
    b.run(s2)
    ended = end_a.query()
    torch.cuda.synchronize()
    print("%s: A alone %.3f ms, B's call with another list on an idle system %.3f ms on the host" % (entry, a_ms, b_host_ms))
    assert a_ms >= 3.0 * b_host_ms, (entry, a_ms, b_host_ms)
    assert ended, entry
    assert all(a.equals(refs[0])), (entry, "A", a.equals(refs[0]))
    assert all(b.equals(refs[1])), (entry, "B", b.equals(refs[1]))
    # B's list again, on the other stream: nothing to prepare
    b.refill()
    torch.cuda.synchronize()
    stamps = _trace(E, lambda: b.run(s1))
    torch.cuda.synchronize()
    assert all(b.equals(refs[1])), entry
    if entry == "redundancy":
        assert stamps == [REDUNDANCY_LAUNCHED, REDUNDANCY_PLACED_TEAM_LDS], stamps  # (sketch24: a workgroup per system)


@pytest.mark.parametrize("entry", ["freedom", "redundancy", "sensitivity"])
def test_host_form_behind_a_device_call_in_flight(E, pivoted_qr, monkeypatch, entry):
    """A long device call on a torch stream, then the host entry of the same system with a few other values (FreedomAnalysis of 3
    systems: the zero-copy path on the calling thread's own stream): both give what they give alone."""
    import torch

    if entry == "freedom":
        s, a, _ = D.two_calls(E, "freedom", "lds", monkeypatch.setenv)
        x = D.freedom_system(E, "lds")[3](3)[::-1].copy()
        host = lambda: s.freedom_batch(x)
    elif entry == "redundancy":
        s, a, _ = D.two_calls(E, "redundancy", "sketch24", monkeypatch.setenv)
        c = RR.case("sketch24")
        host = lambda: tuple(v for _, v in sorted(s.redundancy(c["x"], focus=c["focus"], want_rows=True).items()))
    else:
        s, a, _ = D.two_calls(E, "sensitivity", "massive40", monkeypatch.setenv)
        ref = SR.system("massive40")
        host = lambda: s.param_sensitivity(ref["x"], ref["pos"], ref["params"], lam=ref["lam"], want_degenerate=True)
    s1 = torch.cuda.Stream()
    a_ms, a_ref = _alone(torch, a, s1)
    host()
    t0 = time.perf_counter()
    want = host()
    host_ms = (time.perf_counter() - t0) * 1e3
    a.refill()
    torch.cuda.synchronize()
    a.run(s1)
    got = host()
    torch.cuda.synchronize()
    print("%s: A alone %.3f ms, the host entry alone %.3f ms" % (entry, a_ms, host_ms))
    assert all(a.equals(a_ref)), (entry, a.equals(a_ref))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), entry


def test_solve_beside_params_on_the_shared_global_workspace(E, monkeypatch):
    """The plain entry and the params entry of a system whose workspace is in global memory share that workspace (and its event,
    list_walk_launch.hip.hpp: on_workspace): a long solve on one stream, a short params call on another."""
    import torch

    recs, g, config, make = D.driven_shape(E, "global workspace", monkeypatch.setenv)
    s = make()
    batch_a, batch_b = D.BATCHES[("params", "global workspace")]
    a = D.solve_call(s, g, len(recs), batch_a, 303, config)
    b = D.driven_call(E, s, recs, g, batch_b, 202, 0, config)
    _long_then_short(torch, a, b, "solve beside params, global workspace")


def test_first_use_in_either_order(E):
    """Redundancy before FreedomAnalysis on one fresh block system, the other way round on another: the second plan derives its
    tables from the first one's component lists.  Every output is the same, byte for byte."""
    c = RR.case("blocks")
    # (without every 28th record, from the third: six variables are free, and redundant and conflicting rows remain)
    recs = O.stack([r for i, r in enumerate(c["recs"]) if i % 28 != 2])
    x = c["x"][:9]
    focus = [f - sum(1 for i in range(f) if i % 28 == 2) for f in c["focus"][:2]]
    one, two = E.System(recs, c["n_vars"]), E.System(recs, c["n_vars"])
    red1 = one.redundancy(x, focus=focus, want_rows=True)
    free1 = one.freedom_batch(x)
    free2 = two.freedom_batch(x)
    red2 = two.redundancy(x, focus=focus, want_rows=True)
    for key in red1:
        assert red1[key].tobytes() == red2[key].tobytes(), key
    for u, v in zip(free1, free2):
        assert u.tobytes() == v.tobytes()
    assert free1[0].any() and not free1[0].all()
    assert (red1["row_status"] == 2).any() and (red1["row_status"] == 3).any() and red1["group"].any(axis=2).all()
