"""GPU tests (-m gpu) of the row stream of the kernel that does not wait for the LM control's verdicts, in its full-line form
(jit_kernel.hip.hpp: solve_kernel_fast<..., 4, true>, fast_wave IO 2): a wavefront's contiguous piece of a row is loaded and
stored as 16-byte accesses under the stream-once cache policy (piece_load / piece_store, kStreamOnce).  The policy must change
nothing but speed, so every comparison is bitwise: against the oracle, and -- the same cases run in a process of their own with
EZPZ_JIT_AHEAD=0 -- against the loop kernel, which keeps the default policy.

Sizes (gen_big_problem(lines), 4 * lines variables; four wavefronts for 385 ... 512 lines, 128 lines = 4096 bytes per wavefront,
the last one's piece 32 * (lines - 384) bytes):
  500  the 2000 x 2000 headline: last piece 3712 bytes = 3 KB + 40 lanes of the fourth, rows of 16 000 bytes start on a line
  497  rows of 15 904 bytes: not a multiple of 128, so all rows but every fourth start inside a line; last piece 3 KB + 34 lanes
  385  the last wavefront's piece is 32 bytes: two lanes of one access
A piece that is NOT A MULTIPLE OF 16 BYTES cannot be exercised: a line of gen_big_problem is four variables and a wavefront owns
whole lines, so every piece of every CONTIG size is a multiple of 32 bytes (the 8-byte tail of piece_load / piece_store is there
for topologies that the generator does not make).

Batch sizes: 1, 2, 3 (no next system; one), the launch's capacity + 1 and 2 x capacity + 5 (the draw is two systems ahead; the
last rounds have no next system).  The capacity is the device's compute units times the workgroups per compute unit that the
generated source asks for in ezpz_jit_solve_fast's __launch_bounds__ (wavefronts per SIMD = workgroups of four wavefronts per
compute unit); should the loader settle for fewer, both sizes are still beyond one and two rounds.

x_out is a view inside a larger tensor filled with a fixed bit pattern: every byte around the rows must keep it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gen
from conftest import ROOT
from oracle import oracle as O
from oracle import textual as T

pytestmark = pytest.mark.gpu

N_BASE = 64  # distinct systems; larger batches repeat them (system b of a batch is base system b % 61)
MASK_BATCH = 130  # (a host call of more than 1 MB, so that the host entry takes the kernel under test)

CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import ezpz_amd as E
from oracle import textual as T
lines, path, per_cu = int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
ref = T.load(T.gen_big_problem(lines))
n = ref.num_vars
s = E.System(ref.constraints, n)
assert s.info()["team_mode"] == 3, s.info()
assert s.specialize(wait=True) == 2
base, want = np.load(path + "/x0.npy"), np.load(path + "/xo.npy")
based, wantd = torch.from_numpy(base).cuda(), torch.from_numpy(want).cuda().view(torch.int64)
cap = int(torch.cuda.get_device_properties(0).multi_processor_count) * per_cu
PATTERN, GUARD = 0x5A5A5A5A5A5A5A5A, 272
out = {"capacity": cap}
def device_call(name, B):
    idx = torch.arange(B, device="cuda") % 61 if B > 64 else torch.arange(B, device="cuda")
    xin = based[idx].contiguous()
    buf = torch.full((2 * GUARD + B * n,), PATTERN, dtype=torch.int64, device="cuda")
    st = torch.zeros((B, 32), dtype=torch.uint8, device="cuda")
    s.solve_batch_device(xin.data_ptr(), B, buf.data_ptr() + 8 * GUARD, st.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rows = buf[GUARD:GUARD + B * n].view(B, n)
    out[name + "_rows_ok"] = bool(torch.equal(rows, wantd[idx]))
    out[name + "_wrong_rows"] = (rows != wantd[idx]).any(dim=1).nonzero().flatten()[:8].cpu().numpy()
    out[name + "_guard_ok"] = bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + B * n:] == PATTERN).all())
    out[name + "_st"] = st.cpu().numpy().view(E.STATUS_DTYPE).reshape(-1)
    out[name + "_idx"] = idx.cpu().numpy()
for B in (1, 2, 3, cap + 1, 2 * cap + 5):
    device_call("b%d" % (B if B <= 3 else (4 if B == cap + 1 else 5)), B)
for rep in range(2):  # (the second call finds the first one's redo list used: the `_list` launch is then as wide as the device)
    device_call("redo%d" % rep, 64)
idx = np.arange(int(sys.argv[5])) % 61
x, st, mask = s.solve_batch(base[idx], want_mask=True)
out["mask_rows_ok"] = bool(np.array_equal(x.view(np.uint64), want[idx].view(np.uint64)))
out["mask_st"], out["mask_mask"], out["mask_idx"] = st, mask, idx
np.savez(path + "/out.npz", **out)
print("ok")
'''


def fast_entry(lines):
    """(workgroups per compute unit, template arguments) of ezpz_jit_solve_fast in the generated source -- no device needed."""
    import ezpz_amd as E

    ref = T.load(T.gen_big_problem(lines))
    src = E.specialized_source(ref.constraints, ref.num_vars)
    m = re.search(r"__launch_bounds__\((\d+), (\d+)\) ezpz_jit_solve_fast\(const ezpz::jit::JitArgs a\) \{\s*ezpz::jit::solve_kernel_fast<(.*?)>\(a\);", src, re.S)
    assert m, src[-3000:]
    return int(m.group(1)), int(m.group(2)), m.group(3)


@pytest.fixture(scope="module", params=[500, 497, 385])
def outcome(request, tmp_path_factory):
    """The oracle's answers for N_BASE systems -- every other one starts at the solution: no iteration, so the fast kernel's verdict
    does not stand and the system goes through the redo list -- and what the two kernels made of every case (computed once)."""
    lines = request.param
    threads, per_simd, targs = fast_entry(lines)
    # the form under test, first: four wavefronts, every wavefront's variables one contiguous piece
    assert threads == 256 and targs.endswith(", 4, true"), (lines, threads, targs[-40:])
    ref = T.load(T.gen_big_problem(lines))
    n = ref.num_vars
    assert (8 * n) % 128 == (0 if lines % 4 == 0 else 32 * (lines % 4))
    exact = np.zeros(n)
    exact[0::4] = exact[2::4] = np.arange(lines)
    exact[3::4] = 4.0
    x0 = ref.guesses[None, :] + gen.keyed_uniform(4242 + lines, N_BASE, n, -0.25, 0.25)
    x0[1::2] = exact
    rc, xo, it, conv, nun = O.solve_batch(ref.constraints, x0, linsolve=O.LINSOLVE_SPARSE)
    assert rc == 0
    assert np.all(it[0::2] == 2) and np.all(conv == 1) and np.all(it[1::2] == 0), it
    d = tmp_path_factory.mktemp("stream%d" % lines)
    np.save(str(d / "x0.npy"), x0)
    np.save(str(d / "xo.npy"), xo)
    got = {}
    for ahead in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(lines), str(d), str(per_simd), str(MASK_BATCH)],
                           env=dict(os.environ, EZPZ_JIT_AHEAD=ahead), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
        got[ahead] = dict(np.load(str(d / "out.npz")))
    return {"lines": lines, "it": it, "conv": conv, "nun": nun, "fast": got["1"], "loop": got["0"]}


def check_case(o, name):
    """Rows bitwise the oracle's in both kernels, the bytes around them untouched, statuses the oracle's and the same in both."""
    fast, loop = o["fast"], o["loop"]
    for which, got in (("fast", fast), ("loop", loop)):
        assert got[name + "_rows_ok"], (o["lines"], name, which, got[name + "_wrong_rows"])
        assert got[name + "_guard_ok"], (o["lines"], name, which)
    idx = fast[name + "_idx"]
    assert np.array_equal(idx, loop[name + "_idx"])
    st = fast[name + "_st"]
    for f in st.dtype.names:
        assert np.array_equal(st[f], loop[name + "_st"][f], equal_nan=True), (name, f)
    assert np.array_equal(st["iterations"], o["it"][idx]) and np.array_equal(st["converged"], o["conv"][idx])
    assert np.array_equal(st["n_unsatisfied"], o["nun"][idx])


@pytest.mark.parametrize("name", ["b1", "b2", "b3"])
def test_batches_with_no_next_system_and_with_one(outcome, name):
    check_case(outcome, name)
    assert len(outcome["fast"][name + "_idx"]) == int(name[1])


def test_one_system_more_than_the_launch_holds(outcome):
    check_case(outcome, "b4")
    assert len(outcome["fast"]["b4_idx"]) == int(outcome["fast"]["capacity"]) + 1 > 1


def test_two_rounds_and_five_systems(outcome):
    """The row after next is drawn two systems ahead; in the last rounds there is no next system."""
    check_case(outcome, "b5")
    assert len(outcome["fast"]["b5_idx"]) == 2 * int(outcome["fast"]["capacity"]) + 5


@pytest.mark.parametrize("rep", [0, 1])
def test_redo_list_every_other_system(outcome, rep):
    """Every other system starts at the solution (0 iterations): the fast kernel stores its rows under the stream-once policy, lists
    the system, and the loop kernel's stores of the same rows must be what is read back."""
    check_case(outcome, "redo%d" % rep)
    assert np.array_equal(outcome["fast"]["redo%d_st" % rep]["iterations"][:4], [2, 0, 2, 0])


def test_with_the_unsatisfied_mask(outcome):
    fast, loop = outcome["fast"], outcome["loop"]
    assert fast["mask_rows_ok"] and loop["mask_rows_ok"]
    idx = fast["mask_idx"]
    assert len(idx) == MASK_BATCH
    assert np.array_equal(fast["mask_mask"], loop["mask_mask"])
    assert np.array_equal(fast["mask_mask"].sum(axis=1), outcome["nun"][idx])
    for f in fast["mask_st"].dtype.names:
        assert np.array_equal(fast["mask_st"][f], loop["mask_st"][f], equal_nan=True), f
    assert np.array_equal(fast["mask_st"]["iterations"], outcome["it"][idx]) and np.array_equal(fast["mask_st"]["converged"], outcome["conv"][idx])
