"""GPU tests (-m gpu) of the short division's range test in the kernel that does not wait for the LM control's verdicts
(jit_kernel.hip.hpp: fast_wave, DivRange).  That kernel divides through a refined reciprocal, which is the correctly rounded
quotient only while the numerator is zero or in a safe range; a lane whose numerator was outside it must put its system on the
redo list, where the loop kernel divides plainly.  The range is tested once per system on a folded maximum and a folded minimum
exponent, and lanes without an instance sit a slot out -- so here single lanes of full slots and of partial slots (the last
wavefront's last slot of each class) get guesses that make their numerators zero, denormal, about 2^-900, about 2^600,
infinite and NaN, among ordinary systems; every output must be bitwise the oracle's and the loop kernel's (EZPZ_JIT_AHEAD=0,
a process of its own)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gen
from conftest import ROOT
from oracle import oracle as O
from oracle import textual as T

pytestmark = pytest.mark.gpu

CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import ezpz_amd as E
from oracle import textual as T
lines, path = int(sys.argv[2]), sys.argv[3]
ref = T.load(T.gen_big_problem(lines))
x0 = np.load(path + "/x0.npy")
s = E.System(ref.constraints, ref.num_vars)
assert s.info()["team_mode"] == 3, s.info()
assert s.specialize(wait=True) == 2
for rep in range(2):
    x, st, mask = s.solve_batch(x0, want_mask=True)
    np.savez(path + "/out%d.npz" % rep, x=x, st=st, mask=mask)
print("ok")
'''

# what is added to the solution's value of one variable of one system: the residual of its Fixed constraint, and so the numerator of
# the lane's first division, is exactly that (where the solution's value is 0), or what is left of it beside the value
SPECIALS = [0.0, 1.5e-323, -5e-324, 2.0 ** -900, -(2.0 ** -901), 2.0 ** -899, 2.0 ** 600, -(2.0 ** 601), 2.0 ** 599, np.inf, -np.inf, np.nan]


def cases(lines, B):
    """Guesses for B systems of gen_big_problem(lines): ordinary ones, and between them systems with ONE special value each."""
    ref = T.load(T.gen_big_problem(lines))
    n = ref.num_vars
    exact = np.zeros(n)
    exact[0::4] = exact[2::4] = np.arange(lines)
    exact[3::4] = 4.0
    x0 = ref.guesses[None, :] + gen.keyed_uniform(1207, B, n, -0.25, 0.25)
    # line 0's variables (solution 0, 0, 0, 4: the first lane of a full slot) and the last line's (the last lane with an instance of the
    # last wavefront's partial slots)
    variables = [0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1]
    special = [(v, d) for v in variables for d in SPECIALS]
    assert 2 * len(special) + 3 <= B
    for k, (v, d) in enumerate(special):
        x0[3 + 2 * k, v] = exact[v] + d
    # ... one system with a special value in every one of those lanes at once, and one at the solution (every numerator zero)
    for k, v in enumerate(variables):
        x0[1, v] = exact[v] + SPECIALS[(5 * k + 1) % len(SPECIALS)]
    x0[B - 1] = exact
    return ref, x0, special


@pytest.mark.parametrize("lines,B", [(500, 256), (70, 2048), (600, 256)])
def test_numerators_outside_the_short_divisions_range_in_single_lanes(lines, B, tmp_path):
    """500 lines: the 2000 x 2000 headline (four wavefronts, 52 of 64 and 40 of 64 instances in the last one's last slots); 70 lines: one
    wavefront, whose values wait in LDS for their stores, 6 and 12 instances in its partial slots; 600 lines: the build with a wavefront
    per SIMD less.  Calls of more than 1 MB, so that the host entry takes the kernel under test."""
    ref, x0, special = cases(lines, B)
    assert x0.nbytes > (1 << 20)
    rc, xo, it, conv, nun = O.solve_batch(ref.constraints, x0, linsolve=O.LINSOLVE_SPARSE)
    assert rc == 0
    out = {}
    for ahead in ("1", "0"):
        d = tmp_path / ("ahead" + ahead)
        d.mkdir()
        np.save(str(d / "x0.npy"), x0)
        env = dict(os.environ, EZPZ_JIT_AHEAD=ahead, EZPZ_JIT_CACHE_DIR=str(d))
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(lines), str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
        out[ahead] = [np.load(str(d / ("out%d.npz" % rep))) for rep in range(2)]
    for rep in range(2):
        fast, loop = out["1"][rep], out["0"][rep]
        bad = np.nonzero(~(np.isnan(fast["x"]) & np.isnan(xo)) & (fast["x"] != xo))
        assert np.array_equal(fast["x"], xo, equal_nan=True), [(int(b), int(v), x0[b, v], fast["x"][b, v], xo[b, v]) for b, v in zip(*bad)][:8]
        assert np.array_equal(fast["x"].view(np.uint64)[~np.isnan(xo)], xo.view(np.uint64)[~np.isnan(xo)])  # (the sign of a zero too)
        assert np.array_equal(np.isnan(fast["x"]), np.isnan(loop["x"])) and np.array_equal(fast["mask"], loop["mask"])
        assert np.array_equal(fast["x"].view(np.uint64)[~np.isnan(xo)], loop["x"].view(np.uint64)[~np.isnan(xo)])
        for f in fast["st"].dtype.names:
            assert np.array_equal(fast["st"][f], loop["st"][f], equal_nan=True), f
        assert np.array_equal(fast["st"]["iterations"], it) and np.array_equal(fast["st"]["converged"], conv)
        assert np.array_equal(fast["st"]["n_unsatisfied"], nun) and np.array_equal(fast["mask"].sum(axis=1), nun)
    # the ordinary systems between the special ones took the expected path
    ordinary = np.ones(B, bool)
    ordinary[[1, B - 1] + [3 + 2 * k for k in range(len(special))]] = False
    assert np.all(it[ordinary] == 2) and np.all(conv[ordinary] == 1)
