"""GPU tests (-m gpu) of the solution branches (ezpz_branch_cluster, ezpz_system_solve_branches and their _device forms;
csrc/branches.hip): the clustering alone is the sequential leader pass of tests/branch_ref.py byte for byte -- info, branches,
x_branch and the labels -- on data made to sit on the rule's edges; the run is the chain of the entries it is made of (ezpz_mc_sample,
solve_batch, then that reference), byte for byte; and cutting either into rounds changes no byte.  Every case is small: the shapes are
the boundaries of a round, of a lane group and of an LDS tile, not the workload's.

Bars.  Bytes everywhere but against the oracle, whose answers agree with the device's to rounding: there the device's leaders are
paired one to one with the oracle's under the rule itself at eps 1e-4 -- safe because tests/test_branches_cpu.py shows, on these very
starts, that labels at 1e-6 and at 1e-4 are identical."""
import ctypes as C

import numpy as np
import pytest

import branch_ref as R
from oracle import oracle as O
from test_branches_cpu import SAMPLES, SEED

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
COLD_STAMPS = {20, 21, 22, 23}  # csrc/call_trace.hpp: the symbolic phase of a system's first request (no launch)
GRID = dict(eps_abs=0.25, eps_rel=0.0)  # with values on a grid of 0.125 every difference and the threshold are exact
_CACHE = {}


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


def _trace(E, call):
    """(what call() returned, the stamps of csrc/call_trace.hpp it left: ids only)."""
    trace = np.zeros(256, dtype=np.uint64)
    E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
    try:
        out = call()
    finally:
        k = E.lib().ezpz_debug_call_trace(None, 0)
    return out, [int(v) for v in trace[:k:2]]


def device_bytes(res):
    return R.result_bytes(res.info, res.branches, res.x, res.labels)


def assert_is_the_reference(E, x, ok, compare=None, chunks=(0, 256), max_branches=32, **rule):
    """E.cluster_branches on x [batch, samples, n_vars] at every chunk against branch_ref, bytes; returns the reference."""
    want = R.cluster_batch(x, ok, compare=compare, max_branches=max_branches, **rule)
    for chunk in chunks:
        got = E.cluster_branches(x, ok, compare=compare, keep=True, branch=E.BranchConfig(max_branches=max_branches, chunk=chunk, **rule))
        for name, g, w in zip(("info", "branches", "x_branch", "labels"), device_bytes(got), R.result_bytes(*want)):
            assert g == w, (name, chunk, got.info, want[0])
    return want


def clustered(rng, batch, samples, n_vars, n_clusters, spacing=2.0):
    """Values on a grid of 0.125: cluster centres `spacing` apart in every variable, members within +-0.25 of the centre in two of
    them -- so a member lies within 0.25 of its leader, exactly at 0.25 from it, or beyond (up to 0.5): all three sides of the
    threshold."""
    centre = rng.integers(0, n_clusters, (batch, samples))
    x = centre[:, :, None] * spacing + np.zeros((1, 1, n_vars))
    for v in {0, n_vars - 1}:  # (the first and the last variable move; with all of them moving nearly every sample is a branch)
        x[:, :, v] += rng.integers(-2, 3, (batch, samples)) * 0.125
    return x, centre


# ---- the clustering alone -----------------------------------------------------------------------------------------------------------
def test_1000_samples_5_variables_3_compared(E):
    rng = np.random.default_rng(1)
    x, _ = clustered(rng, 2, 1000, 5, 4)
    x[:, :, [1, 3]] = rng.uniform(-50, 50, (2, 1000, 2))  # the uncompared variables are noise
    ok = rng.random((2, 1000)) < 0.9
    info, branches, _, labels = assert_is_the_reference(E, x, ok, compare=[1, 0, 1, 0, 1], chunks=(0, 256, 512), max_branches=64, **GRID)
    # the data reaches what it is meant to: several branches per centre (members beyond 0.25 of the first leader), not-ok samples,
    # and differences exactly at the threshold that joined
    assert np.all(info["n_branches"] > 4) and np.all(info["n_ok"] < 1000) and np.all(info["n_overflow"] == 0)
    lead = x[0, branches["first"][0, labels[0][labels[0] >= 0]]][:, [0, 2, 4]]
    assert np.any(np.abs(x[0, labels[0] >= 0][:, [0, 2, 4]] - lead).max(axis=1) == 0.25)


def test_the_intransitive_chain_and_one_variable(E):
    x = np.array([0.0, 0.75, 1.5, 0.5, 2.25]).reshape(1, 5, 1)
    want = assert_is_the_reference(E, x, np.ones((1, 5), bool), chunks=(0,), eps_abs=1.0, eps_rel=0.0)
    assert want[3][0].tolist() == [0, 0, 1, 0, 1]
    rng = np.random.default_rng(2)
    x, _ = clustered(rng, 1, 1000, 1, 5)  # n_vars = 1: seven lanes of every group idle
    assert_is_the_reference(E, x, np.ones((1, 1000), bool), **GRID)


def test_sample_0_not_ok_and_no_sample_ok(E):
    rng = np.random.default_rng(3)
    x, _ = clustered(rng, 2, 600, 4, 3)
    ok = np.ones((2, 600), bool)
    ok[0, 0] = False
    x[1, 0, 2] = np.nan  # (not ok by its value; dist_inf of base 1 is then measured from a NaN: it never wins)
    want = assert_is_the_reference(E, x, ok, **GRID)
    assert want[3][:, 0].tolist() == [-1, -1] and want[1]["first"][:, 0].tolist() == [1, 1]
    want = assert_is_the_reference(E, x, np.zeros((2, 600), bool), **GRID)
    assert want[0]["n_branches"].tolist() == [0, 0] and not want[1]["count"].any() and np.all(want[3] == -1)


def test_a_leader_that_is_the_last_sample_of_a_round(E):
    rng = np.random.default_rng(4)
    x, _ = clustered(rng, 1, 700, 3, 3)
    x[0, 255] = 100.0  # rounds of 256: the last sample of round 0 and of round 1 each open a branch of their own ...
    x[0, 511] = 200.0
    x[0, 600] = 100.125  # ... which a later round's sample joins
    want = assert_is_the_reference(E, x, np.ones((1, 700), bool), chunks=(256, 0), **GRID)
    firsts = want[1]["first"][0, : want[0]["n_branches"][0]].tolist()
    assert 255 in firsts and 511 in firsts and want[3][0, 600] == firsts.index(255)


def test_overflow(E):
    rng = np.random.default_rng(5)
    x, _ = clustered(rng, 1, 600, 2, 6, spacing=10.0)
    x = np.round(x / 10.0) * 10.0  # six tight clusters
    want = assert_is_the_reference(E, x, np.ones((1, 600), bool), max_branches=3, **GRID)
    assert want[0]["n_branches"][0] == 3 and want[0]["n_overflow"][0] == np.count_nonzero(want[3] == -2) > 0
    # 300 distinct samples against a table of 256
    x = (np.arange(300.0) * 3.0).reshape(1, 300, 1) * np.ones((1, 1, 2))
    want = assert_is_the_reference(E, x, np.ones((1, 300), bool), max_branches=256, chunks=(0, 256), **GRID)
    assert tuple(want[0][0]) == (300, 300, 256, 44) and want[3][0].tolist() == list(range(256)) + [-2] * 44


@pytest.mark.parametrize("n_cmp", [12, 20, 40])
def test_every_width_of_a_lane_group(E, n_cmp):
    # 8 lanes serve the cases above; 16, 32 and 64 lanes per sample here (a mask leaves a few variables out)
    rng = np.random.default_rng(n_cmp)
    x, _ = clustered(rng, 2, 600, n_cmp + 3, 5)
    compare = np.ones(n_cmp + 3, np.uint8)
    compare[[1, 4, n_cmp]] = 0
    x[:, :, compare == 0] = rng.uniform(-9, 9, (2, 600, 3))
    assert_is_the_reference(E, x, rng.random((2, 600)) < 0.95, compare=compare, chunks=(256,), **GRID)


def test_300_variables(E):
    # more variables than a wavefront has lanes, and 20 leaders of 300 values: more than one LDS tile (13 of them fit one)
    rng = np.random.default_rng(6)
    x, _ = clustered(rng, 1, 600, 300, 20)  # (the verdict hangs on the first and on the last variable)
    x[0, 400] = 50.0  # (a branch that opens in the second round of 256, behind both tiles)
    want = assert_is_the_reference(E, x, np.ones((1, 600), bool), chunks=(256, 0), max_branches=128, **GRID)
    assert want[0]["n_branches"][0] > 20 and 400 in want[1]["first"][0].tolist()


def test_a_row_longer_than_an_lds_tile(E):
    # 4100 compared values: one leader's row does not fit the tile and is read from global memory
    rng = np.random.default_rng(7)
    centre = rng.integers(0, 3, (1, 520))
    x = centre[:, :, None] * 2.0 + np.zeros((1, 1, 4100))
    x[0, :, 4099] += rng.integers(-2, 3, 520) * 0.125
    assert_is_the_reference(E, x, np.ones((1, 520), bool), chunks=(256,), **GRID)


# ---- the run ----------------------------------------------------------------------------------------------------------------------
def fixture(E, name):
    if name not in _CACHE:
        f = getattr(R, name)(3)
        _CACHE[name] = (f, E.System(f.records, f.n_vars), [E.McDist(*t) for t in f.spread(3.0)])
    return _CACHE[name]


def chain_of_entries(E, name, x0, samples=SAMPLES, **rule):
    """ezpz_mc_sample for the starts, System.solve_batch, then the reference: per base of x0 [batch, n_vars]."""
    f, system, _ = fixture(E, name)
    x, st = zip(*[system.solve_batch(R.starts(E, f, SEED, samples, x0=row))[:2] for row in x0])
    x, st = np.stack(x), np.stack(st)
    return R.cluster_batch(x, R.ok_of(st["converged"], st["n_unsatisfied"]), origin=x0, status=st, **rule)


def run(E, name, x0, samples=SAMPLES, **kw):
    _, system, dists = fixture(E, name)
    return system.solve_branches(x0, dists, samples, seed=SEED, keep=True, **kw)


@pytest.mark.parametrize("name", ["chain", "blocks"])
def test_the_run_is_the_chain_of_entries_and_finds_the_oracles_branches(E, name):
    f, _, _ = fixture(E, name)
    got = run(E, name, f.x0)
    want = chain_of_entries(E, name, f.x0[None])
    for what, g, w in zip(("info", "branches", "x_branch", "labels"), device_bytes(got), R.result_bytes(*want)):
        assert g == w, (what, got.info, want[0])
    assert got.info["n_branches"][0] == 8 and got.labels[0, 0] == 0 and got.branches["first"][0, 0] == 0
    assert got.info["n_ok"][0] >= 0.9 * SAMPLES and got.info["n_ok"][0] == got.branches["count"].sum() + got.info["n_overflow"][0]
    assert got.nearest().tolist() == np.argsort(got.branches["dist_inf"][0, :8], kind="stable").tolist()
    # the oracle, from the same starts: 8 branches, and every device leader is the same branch as exactly one oracle leader
    rc, xo, _, conv, nun = O.solve_batch(f.records, R.starts(E, f, SEED, SAMPLES))
    assert rc == 0
    oracle = R.cluster(xo, R.ok_of(conv, nun), eps_abs=1e-4, eps_rel=1e-4, origin=f.x0)
    assert oracle[0]["n_branches"][0] == 8
    pairs = np.array([[R.same(got.x[0, i], oracle[2][j], 1e-4, 1e-4) for j in range(8)] for i in range(8)])
    assert np.all(pairs.sum(axis=0) == 1) and np.all(pairs.sum(axis=1) == 1)


def three_bases(E):
    f, system, _ = fixture(E, "chain")
    solved, st, _ = system.solve_batch(f.x0[None])
    assert st["converged"][0] and st["n_unsatisfied"][0] == 0
    other = f.x0.copy()
    other[4:] = [2.0, -1.0, 3.5, -2.0, 5.0, -1.0]  # below the base line
    return np.stack([solved[0], np.zeros(f.n_vars), other])


def test_three_bases_in_one_call_equal_their_own_calls(E):
    f, _, dists = fixture(E, "chain")
    x0 = three_bases(E)
    # base 0: a solved state, spread 1e-3 -- one branch, slot 0 = sample 0; base 1: the origin, whose sample 0 has every point on
    # one spot and does not assemble; base 2: an ordinary start below the base line
    tight = [E.McDist(*t) for t in f.spread(1e-3)]
    _, system, _ = fixture(E, "chain")
    near = system.solve_branches(x0[:1], tight, SAMPLES, seed=SEED, keep=True)
    assert tuple(near.info[0]) == (SAMPLES, SAMPLES, 1, 0) and near.branches["first"][0, 0] == 0 and not near.labels.any()
    together = run(E, "chain", x0)
    assert together.labels[1, 0] == -1 and together.labels[2, 0] == 0
    for b in range(3):
        alone = run(E, "chain", x0[b])
        for what, g, w in zip(("info", "branches", "x_branch", "labels"), device_bytes(alone),
                              R.result_bytes(together.info[b:b + 1], together.branches[b], together.x[b], together.labels[b])):
            assert g == w, (what, b)


def test_device_form_on_another_stream_equals_the_host_form_twice(E):
    import torch

    f, system, dists = fixture(E, "blocks")
    x0 = np.stack([f.x0, f.x0 + 0.25 * (1 - np.isin(np.arange(f.n_vars), f.fixed))])
    want = device_bytes(run(E, "blocks", x0, branch=E.BranchConfig(chunk=256)))
    assert device_bytes(run(E, "blocks", x0)) == want  # (one round of 512 or two of 256: a block system's answers are the same bits)
    x0_dev = torch.from_numpy(x0).cuda()
    stream = torch.cuda.Stream()
    for _ in range(2):
        out = [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (2 * 32, 2 * 32 * 56, 2 * 32 * f.n_vars * 8, 2 * SAMPLES * 4)]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            system.solve_branches_device(x0_dev.data_ptr(), dists, 2, SAMPLES, *(t.data_ptr() for t in out), seed=SEED,
                                         branch=E.BranchConfig(chunk=256), stream=stream.cuda_stream)
        stream.synchronize()
        assert [t.cpu().numpy().tobytes() for t in out] == want


# ---- argument errors: the return code, no output touched, nothing launched ------------------------------------------------------
def _raw_call(E, a, outputs):
    from ezpz_amd._lib import CBranchConfig

    ptr = lambda v: v.ctypes.data if v is not None else None  # noqa: E731
    bc = CBranchConfig(1, 0, a["max_branches"], a["eps_abs"], a["eps_rel"])
    info, branches, xb, labels = (o if a[k] else None for o, k in zip(outputs, ("info", "branches", "x_branch", "labels")))
    if a["run"]:
        d = E.api.mc_dists([E.McDist(*t) for t in a["dist"]]) if a["dist"] is not None else None
        cfg = E.Config()._c()
        return E.lib().ezpz_system_solve_branches(a["sys"]._h if a["sys"] is not None else None, ptr(a["x"]), ptr(d), ptr(a["compare"]),
                                                  a["batch"], a["samples"], C.byref(bc), C.byref(cfg), ptr(info), ptr(branches), ptr(xb),
                                                  ptr(labels))
    return E.lib().ezpz_branch_cluster(ptr(a["x"]), ptr(a["ok"]), ptr(a["compare"]), a["batch"], a["samples"], a["n_vars"], C.byref(bc),
                                       ptr(info), ptr(branches), ptr(xb), ptr(labels))


def _legal(E, run_entry):
    f, system, _ = fixture(E, "chain")
    a = dict(run=run_entry, max_branches=32, eps_abs=1e-5, eps_rel=1e-5, compare=None, batch=2, samples=300, info=True, branches=True,
             x_branch=True, labels=True)
    if run_entry:
        a.update(sys=system, x=np.stack([f.x0, f.x0]), dist=f.spread(3.0))
    else:
        a.update(x=np.zeros((2, 300, f.n_vars)), ok=np.ones((2, 300), np.uint8), n_vars=f.n_vars)
    return a


BAD_RULE = {
    "max_branches 0": dict(max_branches=0),
    "max_branches 257": dict(max_branches=257),
    "eps_abs negative": dict(eps_abs=-1e-9),
    "eps_rel negative": dict(eps_rel=-1.0),
    "eps_abs NaN": dict(eps_abs=np.nan),
    "eps_rel infinite": dict(eps_rel=np.inf),
    "compare selects nothing": dict(compare=np.zeros(10, np.uint8)),
    "x NULL": dict(x=None),
    "info NULL": dict(info=False),
    "branches NULL": dict(branches=False),
    "x_branch NULL": dict(x_branch=False),
}
BAD_RUN = {
    "sys NULL": dict(sys=None),
    "dist NULL": dict(dist=None),
    "unknown kind": dict(dist=[(7, 0.0, 0.0)] * 10),
    "uniform a > b": dict(dist=[(1, 1.0, -1.0)] * 10),
    "non-finite a": dict(dist=[(1, -np.inf, 1.0)] * 10),
    "sigma < 0": dict(dist=[(2, -1.0, 0.0)] * 10),
    "truncation in (0, 1)": dict(dist=[(2, 1.0, 0.5)] * 10),
    "21 corners": dict(),  # (a system of 22 variables: see below)
    "x0 not finite": dict(x=np.full((2, 10), np.nan)),
}


def _outputs(n_vars=10):
    return [np.full(n, 0xA5, np.uint8) for n in (2 * 32, 2 * 32 * 56, 2 * 32 * n_vars * 8, 2 * 300 * 4)]


@pytest.mark.parametrize("run_entry", [False, True])
@pytest.mark.parametrize("what", sorted(BAD_RULE))
def test_argument_errors_of_the_rule(E, what, run_entry):
    a, outputs = _legal(E, run_entry), _outputs()
    a.update(BAD_RULE[what])
    rc, stamps = _trace(E, lambda: _raw_call(E, a, outputs))
    assert rc == ERR_INVALID_ARGUMENT and not set(stamps) - COLD_STAMPS, (what, rc, stamps)
    assert all(np.all(o == 0xA5) for o in outputs), what


@pytest.mark.parametrize("what", sorted(BAD_RUN))
def test_argument_errors_of_the_run(E, what):
    a, outputs = _legal(E, True), _outputs()
    a.update(BAD_RUN[what])
    if what == "21 corners":
        if "s22" not in _CACHE:
            _CACHE["s22"] = E.System(O.stack([O.fixed(v, 1.0 + v) for v in range(22)]), 22)
        a.update(sys=_CACHE["s22"], x=np.ones((2, 22)), dist=[(3, 0.0, 0.1)] * 21 + [(0, 0.0, 0.0)])
        outputs = _outputs(22)
    rc, stamps = _trace(E, lambda: _raw_call(E, a, outputs))
    assert rc == ERR_INVALID_ARGUMENT and not set(stamps) - COLD_STAMPS, (what, rc, stamps)
    assert all(np.all(o == 0xA5) for o in outputs), what


@pytest.mark.parametrize("run_entry", [False, True])
def test_the_legal_call_of_the_error_cases_and_the_empty_ones(E, run_entry):
    # the same arguments with nothing wrong run (so each case above fails for its one reason), and leave their stamps
    a, outputs = _legal(E, run_entry), _outputs()
    rc, stamps = _trace(E, lambda: _raw_call(E, a, outputs))
    assert rc == 0 and 81 in stamps, (rc, stamps)
    info = outputs[0].view(R.INFO_DTYPE)
    assert info["samples"].tolist() == [300, 300] and (info["n_branches"] >= 1).all()
    # samples == 0 or batch == 0: EZPZ_OK, nothing written, nothing launched -- but still an error where the request is wrong
    for empty in (dict(samples=0), dict(batch=0)):
        outputs = _outputs()
        b = dict(a, **empty)
        rc, stamps = _trace(E, lambda: _raw_call(E, b, outputs))
        assert rc == 0 and not set(stamps) - COLD_STAMPS and all(np.all(o == 0xA5) for o in outputs), empty
        assert _raw_call(E, dict(b, max_branches=0), outputs) == ERR_INVALID_ARGUMENT
    # the labels are optional
    outputs = _outputs()
    assert _raw_call(E, dict(a, labels=False), outputs) == 0 and np.all(outputs[3] == 0xA5) and not np.all(outputs[0] == 0xA5)


def test_device_form_argument_error_touches_nothing(E):
    import torch

    f, system, dists = fixture(E, "chain")
    out = [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (32, 32 * 56, 32 * f.n_vars * 8)]
    x0 = torch.from_numpy(f.x0).cuda()
    torch.cuda.synchronize()

    def call():
        with pytest.raises(E.NonLinearSystemError):
            system.solve_branches_device(x0.data_ptr(), dists, 1, 300, *(t.data_ptr() for t in out), branch=E.BranchConfig(eps_abs=-1.0))

    _, stamps = _trace(E, call)
    torch.cuda.synchronize()
    assert not set(stamps) - COLD_STAMPS and all(bool((t == 0x5A).all()) for t in out)
