"""Solution branches, what can be checked without a device: the symbols with their signatures and layouts, the defaults, hand-made
known answers of the rule's reference (tests/branch_ref.py), and the preconditions the GPU tests' fixtures rest on -- checked on the
CPU oracle with the very Philox starts (ezpz_mc_sample, the seeds of tests/test_gpu_branches.py) the device will draw.

The preconditions.  A run on chain(3) and on blocks(3) has 8 branches; the labels at eps 1e-6 and at eps 1e-4 are identical, so
answers of one branch lie within 1e-6 of their leader and distinct branches further apart than 1e-4: a comparison at 1e-4 between
the device's answers and the oracle's (equal to rounding, far below 1e-6) cannot fall on the wrong side; and at least 90 % of the
starts assemble."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import branch_ref as R
import ezpz_amd as E
from ezpz_amd._lib import EXPORTS, CBranchConfig
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SAMPLES = 11, 512  # (tests/test_gpu_branches.py takes them from here)

SIGNATURES = {
    "ezpz_branch_cluster": ["x", "ok", "compare", "batch", "samples", "n_vars", "cfg", "info", "branches", "x_branch", "keep_label"],
    "ezpz_branch_cluster_device": ["x_dev", "ok_dev", "compare", "batch", "samples", "n_vars", "cfg", "info_dev", "branches_dev",
                                   "x_branch_dev", "keep_label_dev", "stream"],
    "ezpz_system_solve_branches": ["sys", "x0", "dist", "compare", "batch", "samples", "bcfg", "cfg", "info", "branches", "x_branch",
                                   "keep_label"],
    "ezpz_system_solve_branches_device": ["sys", "x0_dev", "dist", "compare", "batch", "samples", "bcfg", "cfg", "info_dev", "branches_dev",
                                          "x_branch_dev", "keep_label_dev", "stream"],
}


def test_symbols_signatures_layouts_and_defaults():
    L = E.lib()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ezpz_amd.h")).read())
    for name, params in SIGNATURES.items():
        assert name in EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(params), name
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl, name
        assert [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")] == params, name
    assert "ezpz_default_branch_config" in EXPORTS and re.search(r"void ezpz_default_branch_config\(EzpzBranchConfig\* bcfg\);", header)
    assert E.BRANCH_INFO_DTYPE.itemsize == 32 and E.BRANCH_DTYPE.itemsize == 56 and C.sizeof(CBranchConfig) == 32
    assert E.BRANCH_INFO_DTYPE == R.INFO_DTYPE and E.BRANCH_DTYPE == R.BRANCH_DTYPE
    for text in ("typedef struct EzpzBranchConfig { /* 32 bytes */", "typedef struct EzpzBranchInfo { /* one per base; 32 bytes */",
                 "typedef struct EzpzBranch { /* one per slot; 56 bytes */", "#define EZPZ_BRANCH_MAX 256u",
                 "#define EZPZ_BRANCH_NOT_OK (-1)", "#define EZPZ_BRANCH_OVERFLOW (-2)"):
        assert text in header, text
    bc = CBranchConfig(7, 7, 7, 7.0, 7.0)
    L.ezpz_default_branch_config(C.byref(bc))
    assert (bc.seed, bc.chunk, bc.max_branches, bc.eps_abs, bc.eps_rel) == (0, 0, 32, 1e-5, 1e-5)
    py = E.BranchConfig()._c(5)
    assert (py.seed, py.chunk, py.max_branches, py.eps_abs, py.eps_rel) == (5, 0, 32, 1e-5, 1e-5)
    for method in ("solve_branches", "solve_branches_device"):
        assert callable(getattr(E.System, method))
    assert callable(E.cluster_branches) and callable(E.BranchResult.nearest)
    assert (R.NOT_OK, R.OVERFLOW) == (-1, -2)


# ---- the reference's known answers ---------------------------------------------------------------------------------------------------
def _labels(x, ok=None, **rule):
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    return R.cluster(x, np.ones(len(x), bool) if ok is None else np.asarray(ok), **rule)


def test_the_relation_is_not_transitive_and_the_leader_decides():
    # a ~ b ~ c, a not within eps of c: c fails the leader a although its neighbour b joined
    info, branches, xb, labels = _labels([0.0, 0.75, 1.5, 0.5, 2.25], eps_abs=1.0, eps_rel=0.0)
    assert labels.tolist() == [0, 0, 1, 0, 1] and info["n_branches"][0] == 2
    assert branches["first"][:2].tolist() == [0, 2] and branches["count"][:2].tolist() == [3, 2]
    assert branches["dist_inf"][:2].tolist() == [0.0, 1.5] and xb[:2, 0].tolist() == [0.0, 1.5] and not xb[2:].any()
    # the first leader that fits, not the nearest: 1.0 is nearer to the second leader
    assert _labels([0.0, 1.25, 1.0], eps_abs=1.0, eps_rel=0.0)[3].tolist() == [0, 1, 0]


def test_a_difference_equal_to_the_threshold_joins():
    # a grid of 0.125: every value, difference and threshold below is exact
    assert _labels([1.0, 1.25, 1.375], eps_abs=0.25, eps_rel=0.0)[3].tolist() == [0, 0, 1]
    # the relative part scales with the larger magnitude: |8 - 10| = 2 = 0.2 * 10 joins, |8 - 10.125| does not
    assert _labels([8.0, 10.0, 10.125, -8.0], eps_abs=0.0, eps_rel=0.2)[3].tolist() == [0, 0, 1, 2]
    # every compared variable has to fit; an uncompared one may differ
    x = [[0.0, 0.0, 5.0], [0.25, 0.0, -5.0], [0.0, 0.5, 5.0]]
    assert _labels(x, compare=[1, 1, 0], eps_abs=0.25, eps_rel=0.0)[3].tolist() == [0, 0, 1]
    assert _labels(x, eps_abs=0.25, eps_rel=0.0)[3].tolist() == [0, 1, 2]


def test_samples_that_are_not_ok_are_skipped():
    x = [[0.0, 1.0], [5.0, 1.0], [np.nan, 1.0], [5.0, np.inf], [0.125, 1.0]]
    info, branches, xb, labels = _labels(x, ok=[0, 1, 1, 1, 1], eps_abs=0.25, eps_rel=0.0)
    assert labels.tolist() == [-1, 0, -1, -1, 1] and tuple(info[0]) == (5, 2, 2, 0)
    assert branches["first"][:2].tolist() == [1, 4]
    assert branches["dist_inf"][:2].tolist() == [5.0, 0.125]  # (measured from sample 0 although it is not ok)
    # a non-finite value in a variable that is not compared does not matter
    assert _labels(x, ok=[0, 1, 1, 1, 1], compare=[1, 0], eps_abs=0.25, eps_rel=0.0)[3].tolist() == [-1, 0, -1, 0, 1]
    assert tuple(_labels(x, ok=[0] * 5)[0][0]) == (5, 0, 0, 0)


def test_overflow():
    info, branches, xb, labels = _labels([0.0, 10.0, 20.0, 10.0, 30.0, 0.0, 20.0], eps_abs=1.0, eps_rel=0.0, max_branches=2)
    assert labels.tolist() == [0, 1, -2, 1, -2, 0, -2] and tuple(info[0]) == (7, 7, 2, 3)
    assert branches["count"].tolist() == [2, 2] and info["n_ok"][0] == branches["count"].sum() + info["n_overflow"][0]


# ---- the fixtures' preconditions, on the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain", "blocks"])
def test_the_fixtures_have_8_well_separated_branches(name):
    f = getattr(R, name)(3)
    assert f.n_vars == {"chain": 10, "blocks": 18}[name]
    starts = R.starts(E, f, SEED, SAMPLES)
    assert starts[0].tobytes() == f.x0.tobytes() and np.all(np.abs(starts - f.x0) <= 3.0) and np.all(starts[:, f.fixed] == f.x0[f.fixed])
    rc, x, _, conv, nun = O.solve_batch(f.records, starts)
    ok = R.ok_of(conv, nun)
    assert rc == 0 and ok.mean() >= 0.9 and ok[0]
    tight = R.cluster(x, ok, eps_abs=1e-6, eps_rel=1e-6, origin=f.x0)
    loose = R.cluster(x, ok, eps_abs=1e-4, eps_rel=1e-4, origin=f.x0)
    assert tight[0]["n_branches"][0] == 8 and loose[0]["n_branches"][0] == 8
    assert tight[3].tobytes() == loose[3].tobytes() and tight[0]["n_overflow"][0] == 0
    assert tight[3][0] == 0  # slot 0 is what the plain solve finds


def test_requests_declined_before_any_device_is_touched():
    # the checks come first: a wrong rule and the bounds of the index arithmetic are answered on a machine without a device
    L = E.lib()
    x, out = np.zeros(8), [np.full(64, 0xA5, np.uint8) for _ in range(3)]
    call = lambda bc, batch, samples: L.ezpz_branch_cluster(x.ctypes.data, None, None, batch, samples, 2, C.byref(bc), *(o.ctypes.data for o in out), None)  # noqa: E731
    assert call(CBranchConfig(0, 0, 0, 1e-5, 1e-5), 1, 4) == -103 and call(CBranchConfig(0, 0, 32, -1.0, 1e-5), 1, 4) == -103
    assert call(CBranchConfig(0, 0, 32, 1e-5, 1e-5), 1 << 32, 4) == -102  # batch >= 2^32
    assert call(CBranchConfig(0, 0, 32, 1e-5, 1e-5), 1, 1 << 48) == -102  # samples >= 2^48
    assert call(CBranchConfig(0, 512, 32, 1e-5, 1e-5), (1 << 32) - 1, 1 << 20) == -102  # a round of 2^41 labels
    assert all(np.all(o == 0xA5) for o in out)
