"""Low-discrepancy draws (include/ezpz_amd.h: THE SEQUENCE), what can be checked without a device: the host sampler's points against
torch's and scipy's Sobol' engines, their stratification, the draws against the reference (tests/sequence_ref.py) byte for byte,
slices, the untouched plain draws, the inverse of the normal distribution, what the sequence buys on a tolerance-stack function,
the argument errors and the signatures.

Bars.  Points, shifts, u and flagged UNIFORM draws: bitwise (integer arithmetic, then one exact conversion and rounded + and *).
Flagged NORMAL on the central branch of the inverse: bitwise against the reference (+ - * / alone, in the published order).  Every
flagged NORMAL: 16 ulp of z against an independent inverse (scipy.special.ndtri, else statistics.NormalDist.inv_cdf) -- AS 241
claims about 1e-16 relative, the two independent inverses differ by 4.6 ulp on this grid.  Meaning: the issue's factor 4 at 4096
samples over 32 seeds (26 x and 19 x measured with numpy)."""
import ctypes as C
import inspect
import math
import os
import re
import statistics

import numpy as np
import pytest

import ezpz_amd as E
import mc_ref as R
import sequence_ref as Q
from ezpz_amd._lib import EXPORTS
from ezpz_amd.api import _with_sampling, mc_dists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARGUMENT = -103
SEED = 0x5EED0123456789AB

SIGNATURES = {
    "ezpz_mc_sample": ["seed", "dist", "nominal", "n_param", "first", "count", "params_out"],
}
PY_SIGNATURES = {
    "McDist.__init__": ["self", "kind", "a", "b", "sequence"],
    "McDist.uniform": ["lo", "hi", "sequence"],
    "McDist.normal": ["sigma", "trunc", "sequence"],
    "mc_sample": ["seed", "dists", "nominal", "first", "count"],
}


def _dists(tuples):
    return [E.McDist(*t) for t in tuples]


def _points(seed, dims, first, count):
    """x [count, dims] uint32 recovered from flagged UNIFORM(0, 1) draws at nominal 0: the draw is u itself."""
    u = E.mc_sample(seed, [E.McDist.uniform(0.0, 1.0, sequence=True)] * dims, np.zeros(dims), first, count)
    k = u * 2.0 ** 32 - 0.5
    assert np.all(k == np.floor(k)) and k.min() >= 0 and k.max() < 2.0 ** 32
    shifts = np.array([Q.shift(seed, j) for j in range(dims)], dtype=np.uint32)
    return k.astype(np.uint64).astype(np.uint32) ^ shifts[None, :]


@pytest.fixture(scope="module")
def points4096():
    return _points(SEED, 64, 0, 4096)


def test_points_equal_torch_in_30_bits(points4096):
    import torch
    want = torch.quasirandom.SobolEngine(64, scramble=False).draw(4096, dtype=torch.float64).numpy() * 2.0 ** 30
    assert np.all(want == np.floor(want))
    assert np.array_equal(points4096 >> np.uint32(2), want.astype(np.uint32))


def test_points_equal_scipy_in_32_bits(points4096):
    qmc = pytest.importorskip("scipy.stats.qmc")
    want = qmc.Sobol(d=64, scramble=False, bits=32).random(4096) * 2.0 ** 32
    assert np.all(want == np.floor(want))
    assert np.array_equal(points4096, want.astype(np.uint64).astype(np.uint32))


def test_every_dimension_is_stratified(points4096):
    for m in range(1, 13):
        cells = points4096[:1 << m] >> np.uint32(32 - m)
        assert np.array_equal(np.sort(cells, axis=0), np.repeat(np.arange(1 << m, dtype=np.uint32)[:, None], 64, axis=1)), m


def test_first_two_dimensions_fill_every_elementary_box(points4096):
    x, y = points4096[:1024, 0].astype(np.uint64), points4096[:1024, 1].astype(np.uint64)
    for a in range(11):
        box = ((x >> np.uint64(32 - a)) << np.uint64(10 - a)) | (y >> np.uint64(22 + a))  # (x and y are 64 bits wide: a shift by 32 is 0)
        assert np.array_equal(np.sort(box), np.arange(1024, dtype=np.uint64)), a


# (kind, a, b, flagged): flagged and plain of both kinds, truncations 0, 1 and 1.5, the kinds that ignore the flag
MIXED = [(R.UNIFORM, -0.25, 0.5, 1), (R.NORMAL, 0.125, 0.0, 1), (R.FIXED, 0.0, 0.0, 1), (R.NORMAL, 2.0, 1.0, 1), (R.CORNER, -0.5, 0.75, 1),
         (R.NORMAL, 0.01, 2.5, 0), (R.UNIFORM, 0.0, 0.0, 1), (R.CORNER, 1.0, 1.5, 0), (R.NORMAL, 0.5, 1.5, 1), (R.UNIFORM, -1.0, 1.0, 0)]
NOMINAL = np.array([1.0, -2.5, 3.25, 100.0, 0.0, -7.0, 1e-3, 12.0, 5.0, 0.5])
PLAIN = [(k, a, b, 0) for k, a, b, _ in MIXED]
FLAGGED = [j for j, d in enumerate(MIXED) if d[3] and d[0] in (R.UNIFORM, R.NORMAL)]


def assert_equal_reference(got, want, central, dists):
    """Bitwise wherever the reference says so; the sampler's bar 1e-13 sigma + 2^-52 |p| (tests/test_tolerance_mc_cpu.py) elsewhere."""
    assert got.shape == want.shape
    assert got[central].tobytes() == want[central].tobytes()
    sigma = np.array([d[1] if d[0] == R.NORMAL else 0.0 for d in dists])
    assert np.all(np.abs(got - want) <= 1e-13 * sigma + 2.0 ** -52 * np.abs(want))


def test_flagged_draws_equal_the_reference():
    got = E.mc_sample(SEED, _dists(MIXED), NOMINAL, 0, 700)
    want, central = Q.sample(SEED, MIXED, NOMINAL, 0, 700)
    assert_equal_reference(got, want, central, MIXED)
    assert got[:, 0].tobytes() == want[:, 0].tobytes() and got[:, 6].tobytes() == want[:, 6].tobytes()  # flagged UNIFORM: every bit
    for j in (1, 8):  # flagged NORMAL: most draws are on the central branch, some are not
        assert 0.7 * 700 <= central[:, j].sum() < 700, j
    assert central[:, 3].all()  # (T = 1: p stays inside [0.159, 0.841], the central branch)


def test_a_slice_equals_the_rows_of_a_longer_call():
    all2000 = E.mc_sample(SEED, _dists(MIXED), NOMINAL, 0, 2000)
    for first, count in ((0, 1), (255, 3), (1023, 2), (1024, 512), (1999, 1)):
        assert E.mc_sample(SEED, _dists(MIXED), NOMINAL, first, count).tobytes() == all2000[first:first + count].tobytes(), first
    # the last samples a flagged dimension has (only the host reaches them: a run that far would be 2^32 solves)
    top = 1 << 32
    last1000 = E.mc_sample(SEED, _dists(MIXED), NOMINAL, top - 1000, 1000)
    last300 = E.mc_sample(SEED, _dists(MIXED), NOMINAL, top - 300, 300)
    assert last300.tobytes() == last1000[700:].tobytes()
    if Q.direction_numbers()[1] == 32:
        want, central = Q.sample(SEED, MIXED, NOMINAL, top - 300, 300)
        assert_equal_reference(last300, want, central, MIXED)


def test_unflagged_dimensions_keep_their_bytes():
    plain = E.mc_sample(SEED, _dists(PLAIN), NOMINAL, 0, 300)
    want = R.sample(SEED, [d[:3] for d in PLAIN], NOMINAL, 0, 300)
    exact = np.array([d[0] != R.NORMAL for d in PLAIN])
    assert plain[:, exact].tobytes() == want[:, exact].tobytes()
    assert np.all(np.abs(plain - want) <= 1e-13 * np.array([d[1] if d[0] == R.NORMAL else 0.0 for d in PLAIN]) + 2.0 ** -52 * np.abs(want))
    mixed = E.mc_sample(SEED, _dists(MIXED), NOMINAL, 0, 300)
    for j in range(len(MIXED)):
        assert (mixed[:, j].tobytes() == plain[:, j].tobytes()) == (j not in FLAGGED or j == 6), j  # (6 is UNIFORM(0, 0): one value)
    # the other bits of `reserved` stay ignored, and so does bit 0 on FIXED and CORNER
    d = mc_dists(_dists(PLAIN))
    d["reserved"] = 0xFFFFFFFE
    d["reserved"][[2, 4, 7]] = 0xFFFFFFFF
    assert E.mc_sample(SEED, d, NOMINAL, 0, 300).tobytes() == plain.tobytes()


def test_another_seed_or_position_gives_another_shift():
    one = [E.McDist.uniform(0.0, 1.0, sequence=True)]
    a = E.mc_sample(SEED, one * 2, np.zeros(2), 0, 64)
    b = E.mc_sample(SEED + 1, one * 2, np.zeros(2), 0, 64)
    assert a[:, 0].tobytes() != b[:, 0].tobytes() and a[:, 1].tobytes() != b[:, 1].tobytes()
    shifts = {Q.shift(s, j) for s in (SEED, SEED + 1) for j in range(64)}
    assert len(shifts) == 128
    # the same point set under another shift: XOR of the two runs' grid indices is one constant per dimension
    ka, kb = (a * 2.0 ** 32 - 0.5).astype(np.uint64), (b * 2.0 ** 32 - 0.5).astype(np.uint64)
    for j in range(2):
        assert set(ka[:, j] ^ kb[:, j]) == {Q.shift(SEED, j) ^ Q.shift(SEED + 1, j)}


def _independent_inverse():
    try:
        from scipy.special import ndtri
        return lambda u: ndtri(u)
    except ImportError:
        inv = statistics.NormalDist().inv_cdf
        return lambda u: np.array([inv(float(v)) for v in u])


def _index_of_point(x):
    """b with x_0(b) == x: dimension 0 is the bit reversal of the Gray code."""
    g = int("{:032b}".format(x)[::-1], 2)
    b = 0
    while g:
        b ^= g
        g >>= 1
    return b


def test_normal_inverse_accuracy_truncation_and_grid_ends():
    n = 4096
    z = E.mc_sample(SEED, [E.McDist.normal(1.0, 0.0, sequence=True)], np.zeros(1), 0, n)[:, 0]
    u = Q.units(SEED, 0, 0, n)
    want = np.array([Q.ppnd16(float(v)) for v in u])
    central = want[:, 1].astype(bool)
    assert 0.8 * n <= central.sum() <= 0.9 * n  # (85 % of the grid)
    assert z[central].tobytes() == want[central, 0].tobytes()
    other = _independent_inverse()(u)
    assert np.all(np.abs(z - other) <= 16 * np.spacing(np.abs(other)))
    order = np.argsort(u)
    for trunc in (1.0, 3.0):
        zt = E.mc_sample(SEED, [E.McDist.normal(1.0, trunc, sequence=True)], np.zeros(1), 0, n)[:, 0]
        assert np.all(np.abs(zt) <= trunc) and np.all(np.diff(zt[order]) >= 0.0) and zt[order][0] < -0.9 * trunc and zt[order][-1] > 0.9 * trunc
        ref = np.array([Q.normal_z(float(v), trunc) for v in u])
        ok = ref[:, 1].astype(bool)
        assert zt[ok].tobytes() == ref[ok, 0].tobytes()
        assert np.all(np.abs(zt - ref[:, 0]) <= 1e-13)
    # both ends of the 32-bit grid: u = 2^-33 and 1 - 2^-33, about -+6.34 sigma, finite, with and without a truncation
    s = Q.shift(SEED, 0)
    for k, sign in ((0, -1.0), (0xFFFFFFFF, 1.0)):
        b = _index_of_point(k ^ s)
        assert int(Q.points(0, b, 1)[0]) ^ s == k
        got, end, cut = (E.mc_sample(SEED, [d], np.zeros(1), b, 1)[0, 0] for d in (  # (each at position 0: the same point)
            E.McDist.uniform(0.0, 1.0, sequence=True), E.McDist.normal(1.0, 0.0, sequence=True), E.McDist.normal(2.0, 1.0, sequence=True)))
        assert got == (k + 0.5) * 2.0 ** -32 and 0.0 < got < 1.0
        assert math.isfinite(end) and abs(end - sign * 6.34) < 0.01 and abs(cut - sign * 2.0) < 1e-6 and abs(cut) <= 2.0


def _stack(p):
    return np.sqrt((1.0 + p[:, 0]) ** 2 + (4.0 * p[:, 1]) ** 2) + p[:, 2] - 2.0 * p[:, 3] + 0.5 * p[:, 4] * p[:, 5] + p[:, 6] + np.sin(p[:, 7])


def test_mean_and_std_converge_four_times_closer_than_plain_draws():
    n, seeds = 4096, 32
    flagged, plain = [E.McDist.normal(0.05, 0.0, sequence=True)] * 8, [E.McDist.normal(0.05)] * 8
    truth = _stack(E.mc_sample(0xABCDEF, flagged, np.zeros(8), 0, 1 << 20))
    mean, std = truth.mean(), truth.std(ddof=1)
    err = {}
    for name, dists in (("flagged", flagged), ("plain", plain)):
        f = [_stack(E.mc_sample(1000 + s, dists, np.zeros(8), 0, n)) for s in range(seeds)]
        err[name] = (math.sqrt(np.mean([(v.mean() - mean) ** 2 for v in f])), math.sqrt(np.mean([(v.std(ddof=1) - std) ** 2 for v in f])))
    print("rms error of mean and std, plain / flagged: %.1f x, %.1f x" % (err["plain"][0] / err["flagged"][0], err["plain"][1] / err["flagged"][1]))
    assert err["flagged"][0] <= 0.25 * err["plain"][0]
    assert err["flagged"][1] <= 0.25 * err["plain"][1]


def _raw_sample(dists, first, count, n_out=None):
    d = mc_dists(dists)
    nominal = np.zeros(len(d))
    out = np.full((count if n_out is None else n_out, len(d)), 7.25)
    rc = E.lib().ezpz_mc_sample(SEED, d.ctypes.data, nominal.ctypes.data, len(d), first, count, out.ctypes.data)
    return rc, out


def test_argument_errors_leave_the_output_untouched():
    flagged_u, flagged_n, plain = E.McDist.uniform(0.0, 1.0, sequence=True), E.McDist.normal(1.0, 0.0, sequence=True), E.McDist.uniform(0.0, 1.0)
    top = 1 << 32
    # position 63 is the last one a flagged dimension can take; FIXED and CORNER ignore the flag anywhere
    rc, out = _raw_sample([plain] * 63 + [flagged_u], 0, 4)
    assert rc == 0 and np.all(out != 7.25)
    rc, out = _raw_sample([plain] * 64 + [E.McDist(R.FIXED, 0.0, 0.0, True), E.McDist(R.CORNER, 0.0, 1.0, True)], 0, 4)
    assert rc == 0 and np.all(out != 7.25)
    for bad in (flagged_u, flagged_n):
        rc, out = _raw_sample([plain] * 64 + [bad], 0, 4)
        assert rc == ERR_INVALID_ARGUMENT and np.all(out == 7.25)
    # first + count may reach 2^32 and no further
    rc, out = _raw_sample([flagged_n, plain], top - 4, 4)
    assert rc == 0 and np.all(out != 7.25)
    for first, count in ((top - 3, 4), (top, 1), (2 ** 64 - 2, 4)):
        rc, out = _raw_sample([flagged_n, plain], first, count, n_out=4)
        assert rc == ERR_INVALID_ARGUMENT and np.all(out == 7.25), (first, count)
    rc, out = _raw_sample([plain, plain], top - 2, 4)  # (plain draws go on past 2^32)
    assert rc == 0 and np.all(out != 7.25)
    # the plain list's errors stand with the flag set
    for bad in (E.McDist(R.UNIFORM, 1.0, 0.0, True), E.McDist(R.NORMAL, 1.0, 0.5, True), E.McDist(R.NORMAL, -1.0, 0.0, True), E.McDist(4, 0.0, 0.0, True),
                E.McDist(7, 0.0, 0.0, True)):
        rc, out = _raw_sample([bad], 0, 4)
        assert rc == ERR_INVALID_ARGUMENT and np.all(out == 7.25)
    with pytest.raises(E.NonLinearSystemError):
        E.mc_sample(SEED, [plain] * 64 + [flagged_u], np.zeros(65), 0, 1)


def test_symbols_signatures_and_python_options():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ezpz_amd.h")).read())
    L = E.lib()
    for name, params in SIGNATURES.items():
        assert name in EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(params), name
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")] == params, name
    assert not [name for name in EXPORTS if "sequence" in name]  # no new exported function
    assert "#define EZPZ_MC_SEQUENCE 1u" in header and "typedef struct EzpzMcDist { /* 24 bytes */ uint32_t kind, reserved;" in header
    assert E.MC_DIST_DTYPE.itemsize == 24 and E.MC_DIST_DTYPE.names == ("kind", "reserved", "a", "b") and Q.SEQUENCE == 1
    assert list(inspect.signature(E.McDist.__init__).parameters) == PY_SIGNATURES["McDist.__init__"]
    assert list(inspect.signature(E.McDist.uniform).parameters) == PY_SIGNATURES["McDist.uniform"]
    assert list(inspect.signature(E.McDist.normal).parameters) == PY_SIGNATURES["McDist.normal"]
    assert list(inspect.signature(E.mc_sample).parameters) == PY_SIGNATURES["mc_sample"]
    for fn in (E.McDist.__init__, E.McDist.uniform, E.McDist.normal):
        assert inspect.signature(fn).parameters["sequence"].default is False
    assert inspect.signature(E.System.tolerance_mc).parameters["sampling"].default == "philox"
    assert repr(E.McDist.uniform(-1.0, 1.0)) == "McDist.uniform(-1.0, 1.0)"
    assert repr(E.McDist.uniform(-1.0, 1.0, sequence=True)) == "McDist.uniform(-1.0, 1.0, sequence=True)"
    assert repr(E.McDist.normal(0.5, 3.0, sequence=True)) == "McDist.normal(0.5, 3.0, sequence=True)"
    d = mc_dists([E.McDist.uniform(0, 1, sequence=True), E.McDist.normal(1.0), E.McDist.normal(1.0, 2.0, True), E.McDist.fixed(), E.McDist.corner(0, 1)])
    assert d["reserved"].tolist() == [1, 0, 1, 0, 0] and d["kind"].tolist() == [1, 2, 2, 0, 3]
    assert _with_sampling(d, "philox")["reserved"].tolist() == [1, 0, 1, 0, 0]
    assert _with_sampling(d, "sequence")["reserved"].tolist() == [1, 1, 1, 0, 0] and d["reserved"].tolist() == [1, 0, 1, 0, 0]
    with pytest.raises(ValueError):
        _with_sampling(d, "sobol")
