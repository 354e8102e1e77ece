"""GPU tests (-m gpu) of the factorial effects (ezpz_mc_factorial_device, ezpz_system_tolerance_mc_factorial and its _device form;
csrc/mc_factorial.hip, csrc/tolerance_mc.hip): the device's transform gives the outputs tests/factorial_ref.py states and the host
form's, byte for byte; another stream changes no byte; the run is the plain Monte-Carlo run byte for byte and its factorial outputs
are the reduction alone on its kept rows; and the coefficients mean what the closed form says.  Every case is small: the shapes are
the edges of the kernels' tiles, not a workload.

The tile boundaries.  The gather kernel takes tiles of 2^7 rows and runs levels 0 .. 6 in LDS (ta = 7); a strided launch runs up to 7
more levels (g = 7).  So kc <= 7 is the gather alone (kc < 7: one partial tile), 8 <= kc <= 14 one strided launch of kc - 7 levels, 15
<= kc <= 20 two, the second of kc - 14 levels.  n_meas 3 runs every kc from 1 to 14; n_meas 1 and 32 run kc = 6, 7, 8 (around ta) and
13, 14, 15 (around ta + g); kc = 20 at n_meas 1 is the largest transform the interface allows: 7 + 7 + 6 levels.

Bars.  Everything but the meaning: bytes.  The meaning: every coefficient within max_b |m[b] - closed[b]| + 4 * 2^-53 of the closed
form's (a coefficient is a signed average of the m; the 4 ulp of 1 cover the closed form's own arithmetic in Python floats).  The
maximum itself is printed, not asserted: no existing GPU test of the family holds a solved distance to its closed form, so there is
no bar to take over (DESIGN.md 3r has the measured figure)."""
import math

import numpy as np
import pytest

import factorial_ref as R
import mc_ref
from oracle import oracle as O
from test_factorial_cpu import CAUSES, NAMES, PLACES, parts, reference, rows_of_f, same_bytes
from test_sobol_cpu import TRI_NOMINAL, TRI_POS, TRI_START, triangle

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -103
SEED = 0xC0FFEE1234
_CACHE = {}


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


def out_bytes(kc, n_meas):
    """the bytes of the eight outputs, in the library's order"""
    N = 1 << kc
    return [n_meas * 56, n_meas * kc * 8, n_meas * kc * kc * 8, n_meas * (kc + 1) * 8, n_meas * kc * 8, n_meas * kc * 8, n_meas * kc * 8, n_meas * N * 8]


def shaped(raws, kc, n_meas, with_coef=True):
    """the eight outputs as the arrays tests/factorial_ref.py returns, from their raw bytes"""
    N = 1 << kc
    shapes = [(n_meas, kc), (n_meas, kc, kc), (n_meas, kc + 1), (n_meas, kc), (n_meas, kc), (n_meas, kc), (n_meas, N)]
    out = [raws[0].view(R.DTYPE)] + [r.view(np.float64).reshape(s) for r, s in zip(raws[1:], shapes)]
    return out if with_coef else out[:7]


def device_factorial(E, m, flags, ok, nominal, stream=None, with_coef=True, kc=None, n_meas=None, missing=(), coef_shift=0):
    """ezpz_mc_factorial_device on copies of the arrays, every output prefilled with 7 and a guard of 64 bytes behind it: (rc, the
    eight outputs, or the raw bytes on an error).  missing: the places (0 .. 3: the inputs m, flags, ok, nominal; 4 .. 11: the outputs) passed as NULL;
    coef_shift: 8 puts coef at an address that is aligned as a double and no further."""
    import torch

    N0, M0 = m.shape
    kc0 = N0.bit_length() - 1
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (m, flags, ok, nominal)]
    sizes = out_bytes(kc0, M0)
    outs = [torch.full((s + 64,), 7, dtype=torch.uint8, device="cuda") for s in sizes]
    ptrs = [0 if t is None else t.data_ptr() for t in dev] + [o.data_ptr() for o in outs]
    ptrs[4 + 7] += coef_shift
    sizes[7] += coef_shift
    if not with_coef:
        ptrs[4 + 7] = 0
    for at in missing:
        ptrs[at] = 0
    args = [p or None for p in ptrs[:4]] + [kc0 if kc is None else kc, M0 if n_meas is None else n_meas] + [p or None for p in ptrs[4:]]
    torch.cuda.synchronize()
    if stream is None:
        rc = E.lib().ezpz_mc_factorial_device(*args, None)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_mc_factorial_device(*args, stream.cuda_stream)
        stream.synchronize()
    raws = [o.cpu().numpy() for o in outs]
    if rc != 0:
        return rc, raws
    for at, (r, s) in enumerate(zip(raws, sizes)):
        assert np.all(r[s:] == 7), NAMES[at]  # nothing past the end
    if not with_coef:
        assert np.all(raws[7] == 7)
    assert np.all(raws[7][:coef_shift] == 7)
    return rc, shaped([r[:s].copy() for r, s in zip(raws[:7], sizes)] + [raws[7][coef_shift:sizes[7]].copy()], kc0, M0, with_coef)


SHAPES = [(kc, 3) for kc in range(1, 15)] + [(kc, n_meas) for n_meas in (1, 32) for kc in (6, 7, 8, 13, 14, 15)]


@pytest.mark.parametrize("kc,n_meas", SHAPES)
def test_the_device_reduction_is_the_stated_rule(E, kc, n_meas):
    m, flags, ok, nominal = rows_of_f(kc, n_meas)
    want = reference(kc, n_meas)
    rc, got = device_factorial(E, m, flags, ok, nominal)
    assert rc == 0 and same_bytes(got, want), (kc, n_meas)
    assert same_bytes(got, parts(E.mc_factorial(m, flags, ok, nominal, keep_coef=True)))
    # without flags, ok and coef: the rows are all valid, so the other outputs are the same
    rc, lean = device_factorial(E, m, None, None, nominal, with_coef=False)
    assert rc == 0 and same_bytes(lean, want[:7])
    rc, half = device_factorial(E, m, flags, None, nominal)
    assert rc == 0 and same_bytes(half, want)
    # a record made incomplete by each cause in turn, at the first, a middle and the last row: the host form's bytes (which
    # tests/test_factorial_cpu.py holds to the restatement up to kc = 12), and the restatement's for one of the twelve
    for at, (cause, place) in enumerate((c, p) for c in CAUSES for p in PLACES):
        m2, flags2, ok2, _ = rows_of_f(kc, n_meas, cause, place)
        rc, got2 = device_factorial(E, m2, flags2, ok2, nominal)
        host2 = E.mc_factorial(m2, flags2, ok2, nominal, keep_coef=True)
        assert rc == 0 and same_bytes(got2, parts(host2)), (kc, n_meas, cause, place)
        i = min(2, n_meas - 1)
        assert got2[0]["complete"][i] == 0 and got2[0]["n_valid"][i] == (1 << kc) - 1 and np.isnan(got2[7][i]).all() and np.isnan(got2[1][i]).all()
        if at == (kc + n_meas) % 12:
            assert same_bytes(got2, reference(kc, n_meas, cause, place)), (kc, n_meas, cause, place)


def test_the_largest_transform(E):
    """kc = 20, n_meas = 1: 8 MiB of rows, the gather and two strided launches (7 + 7 + 6 levels), 4096 blocks of sums."""
    kc = 20
    m, flags, ok, nominal = rows_of_f(kc, 1)
    want = R.factorial(m, flags, ok, nominal)
    rc, got = device_factorial(E, m, flags, ok, nominal)
    assert rc == 0 and same_bytes(got, want)
    assert same_bytes(got, parts(E.mc_factorial(m, flags, ok, nominal, keep_coef=True)))
    y = m[:, 0] - nominal[0]
    bar = (4 * kc + (1 << kc) / 256 + 16) * 2.0 ** -53 * float(np.max(y * y))
    print("kc 20: var", got[0]["var"][0], "numpy", float(np.var(y)), "bar", bar)
    assert abs(float(got[0]["var"][0]) - float(np.var(y))) <= bar
    for cause, place in (("flag", "first"), ("nan", "last")):
        m2, flags2, ok2, _ = rows_of_f(kc, 1, cause, place)
        rc, got2 = device_factorial(E, m2, flags2, ok2, nominal, with_coef=False)
        assert rc == 0 and same_bytes(got2, parts(E.mc_factorial(m2, flags2, ok2, nominal))[:7]) and got2[0]["complete"][0] == 0


def test_another_stream_changes_no_byte(E):
    import torch

    stream = torch.cuda.Stream()
    for kc, n_meas in ((13, 32), (8, 3), (15, 1), (3, 3)):
        m, flags, ok, nominal = rows_of_f(kc, n_meas)
        want = reference(kc, n_meas)
        for _ in range(2):  # (the second call finds the workspace as the first left it)
            rc, got = device_factorial(E, m, flags, ok, nominal, stream=stream)
            assert rc == 0 and same_bytes(got, want), (kc, n_meas)
        rc, got = device_factorial(E, m, flags, ok, nominal, stream=stream, coef_shift=8)  # (coef aligned as a double, no further)
        assert rc == 0 and same_bytes(got, want), (kc, n_meas)


def test_argument_errors_of_the_device_reduction_leave_the_prefill(E):
    m, flags, ok, nominal = rows_of_f(3, 3)
    cases = [dict(kc=0), dict(kc=21), dict(n_meas=0), dict(n_meas=33), dict(missing=(0,)), dict(missing=(3,))] + [dict(missing=(4 + o,)) for o in range(7)]
    for case in cases:
        rc, raws = device_factorial(E, m, flags, ok, nominal, **case)
        assert rc == ERR_INVALID_ARGUMENT and all(np.all(r == 7) for r in raws), case


# ---- the run ------------------------------------------------------------------------------------------------------------------------
TRI_MEASURE = O.stack([O.vertical_distance((4, 5), (0, 1), 0.0), O.distance((2, 3), (4, 5), 0.0)])
# three CORNER side lengths; the third stays below 1.9 = 0.95 + 0.95, so all 8 corners assemble
TRI_CORNERS = [(mc_ref.CORNER, -0.05, 0.05), (mc_ref.CORNER, -0.05, 0.05), (mc_ref.CORNER, -0.3, -0.1)]
# ... and widened until the corners with the third side at 2.2 do not
TRI_WIDE = [(mc_ref.CORNER, -0.05, 0.05), (mc_ref.CORNER, -0.05, 0.05), (mc_ref.CORNER, -0.3, 0.3)]


def dists_of(E, tuples):
    return [E.McDist(*t) for t in tuples]


def tri(E):
    if "tri" not in _CACHE:
        rc, x0, _, conv, nun = O.solve_batch(triangle(TRI_NOMINAL), TRI_START)
        assert rc == 0 and conv[0] and nun[0] == 0
        _CACHE["tri"] = (E.System(triangle(TRI_NOMINAL), 6), x0[0].copy())
    return _CACHE["tri"]


def block(E):
    """(system, x0, positions, dists, records): the block system of 4 blocks (16 variables), its 12 parametrised constraints driven --
    10 CORNER dimensions with a FIXED one after the third and after the eighth -- and 5 reference dimensions across the blocks."""
    if "block" not in _CACHE:
        b = E.textual.Problem.from_str(E.textual.gen_big_problem(4)).to_constraint_system()
        s = E.System(b.records, b.num_vars)
        solved, st, _ = s.solve_batch(np.asarray(b.guesses, dtype=float)[None, :])
        assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0
        pos = [i for i in range(len(b.records)) if E.constraint_has_param(b.records[i])]
        assert len(pos) == 12
        dists = [(mc_ref.FIXED, 0.0, 0.0) if j in (3, 9) else (mc_ref.CORNER, -0.01 * (j + 1), 0.02 * (j + 2)) for j in range(12)]
        pt = lambda i: (2 * i, 2 * i + 1)  # noqa: E731
        records = O.stack([O.distance(pt(0), pt(7), 0.0), O.distance(pt(1), pt(4), 0.0), O.horizontal_distance(pt(0), pt(6), 0.0),
                           O.distance(pt(2), pt(5), 0.0), O.vertical_distance(pt(3), pt(0), 0.0)])
        _CACHE["block"] = (s, solved[0].copy(), pos, dists, records)
    return _CACHE["block"]


def case_of(E, name):
    if name == "triangle":
        s, x0 = tri(E)
        return s, x0, TRI_POS, TRI_CORNERS, TRI_MEASURE
    return block(E)


def ranges(E, name):
    if ("nom", name) not in _CACHE:
        s, x0, _, _, records = case_of(E, name)
        _CACHE[("nom", name)] = s.measure(x0[None, :], records)[0]
    nom = _CACHE[("nom", name)]
    return (nom - 0.05, nom + 0.08), (nom - 0.1, nom + 0.2, 16)


def run_f(E, name, chunk, factorial=True):
    key = ("run", name, chunk, factorial)
    if key not in _CACHE:
        s, x0, pos, dists, records = case_of(E, name)
        limits, hist = ranges(E, name)
        extra = dict(factorial=True, keep_coef=True) if factorial else {}
        _CACHE[key] = s.tolerance_mc(x0, pos, dists_of(E, dists), records, E.mc_corner_count(dists_of(E, dists)), seed=SEED, chunk=chunk, keep=True,
                                     limits=limits, hist=hist, **extra)
    return _CACHE[key]


def run_bytes(r):
    return [r.stats.tobytes(), r.totals.tobytes(), r.hist.tobytes(), r.params.tobytes(), r.m.tobytes(), r.flags.tobytes(), r.ok.tobytes()]


@pytest.mark.parametrize("chunk", [256, 0])
@pytest.mark.parametrize("name", ["triangle", "block"])
def test_the_run(E, name, chunk):
    res, p = run_f(E, name, chunk), run_f(E, name, 0, factorial=False)
    kc = {"triangle": 3, "block": 10}[name]
    N = 1 << kc
    # it is that run: stats, totals, hist and the kept arrays are tolerance_mc's bytes
    assert run_bytes(res) == run_bytes(p) and res.samples == N and res.n_ok == N and not hasattr(p, "factorial")
    # the factorial outputs are the reduction alone on the run's kept rows: the device form, the host form, the restatement
    f = res.factorial
    nominal = res.stats["nominal"].copy()
    rc, dev = device_factorial(E, res.m, res.flags, res.ok, nominal)
    host = E.mc_factorial(res.m, res.flags, res.ok, nominal, keep_coef=True)
    if ("ref", name) not in _CACHE:
        _CACHE[("ref", name)] = R.factorial(res.m, res.flags, res.ok, nominal)
    assert rc == 0 and same_bytes(parts(f), dev) and same_bytes(parts(f), parts(host)) and same_bytes(parts(f), _CACHE[("ref", name)])
    assert np.all(f.complete == 1) and np.all(f.n_valid == N) and f.kc == kc
    # what the numbers say against the statistics: the mean deviation, and the extremes against the predicted corners
    assert np.all(np.abs(f.mean_dev - (res.mean - nominal)) <= 1e-12 * np.maximum(1.0, np.abs(res.mean)))
    for i in range(len(nominal)):
        w = f.worst_case(i)
        assert w["m_hi"] <= w["max"] and w["m_lo"] >= w["min"] and w["m_hi"] == res.m[w["corner_hi"], i] and w["max"] == res.m[w["argmax"], i]
    if name == "block":  # the dimensions are places in the run's list: the FIXED ones are skipped
        assert f.dims == [0, 1, 2, 4, 5, 6, 7, 8, 10, 11] and all(d not in (3, 9) for _, t in f.largest(0, 5) for d in t)
    if chunk == 0:  # both round sizes give the same bytes
        assert same_bytes(parts(f), parts(run_f(E, name, 256).factorial)) and run_bytes(res) == run_bytes(run_f(E, name, 256))


def test_the_device_form_on_another_stream_equals_the_host_form(E):
    import torch

    s, x0_host, pos, dists, records = block(E)
    res = run_f(E, "block", 256)
    limits, hist = ranges(E, "block")
    kc, M, N = 10, 5, 1024
    x0 = torch.from_numpy(x0_host).cuda()
    out = lambda n: torch.full((max(n, 1),), 0x5A, dtype=torch.uint8, device="cuda")  # noqa: E731
    raw = lambda t: t.cpu().numpy().tobytes()  # noqa: E731
    stream = torch.cuda.Stream()
    names = ["factorial_%s_ptr" % n for n in NAMES]
    for kept in (True, False):  # the rows in the caller's keep buffers, then in the plan's workspace
        stats, totals, hist_d = out(M * 88), out(24), out(M * 18 * 8)
        outs = [out(n) for n in out_bytes(kc, M)]
        kp, km, kflags, kok = out(8 * N * 12), out(8 * N * M), out(N * M), out(N)
        keep = dict(keep_params_ptr=kp.data_ptr(), keep_m_ptr=km.data_ptr(), keep_flags_ptr=kflags.data_ptr(), keep_ok_ptr=kok.data_ptr()) if kept else {}
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s.tolerance_mc_device(x0.data_ptr(), pos, dists_of(E, dists), records, N, stats.data_ptr(), totals.data_ptr(), hist_d.data_ptr(),
                                  seed=SEED, chunk=256, limits=limits, hist=hist, stream=stream.cuda_stream, factorial=True,
                                  **dict(zip(names, (o.data_ptr() for o in outs))), **keep)
        stream.synchronize()
        assert [raw(t) for t in (stats, totals, hist_d)] == [res.stats.tobytes(), res.totals.tobytes(), res.hist.tobytes()], kept
        assert [raw(o) for o in outs] == [a.tobytes() for a in parts(res.factorial)], kept
        if kept:
            assert [raw(t) for t in (kp, km, kflags, kok)] == [res.params.tobytes(), res.m.tobytes(), res.flags.tobytes(), res.ok.tobytes()]
    # the run's argument errors touch nothing: a dimension that is neither CORNER nor FIXED, no CORNER dimension, samples other than
    # 2^kc, no reference dimension and more than 32, a required output NULL
    given = dict(zip(names, (o.data_ptr() for o in outs)))
    before = [raw(o) for o in outs] + [raw(stats)]
    uniform = [(mc_ref.UNIFORM, -0.1, 0.1) if j == 5 else d for j, d in enumerate(dists)]
    many = O.stack([O.fixed(0, 0.0)] * 33)
    bad = [dict(dists=uniform), dict(dists=[(mc_ref.FIXED, 0.0, 0.0)] * 12), dict(samples=N - 1), dict(samples=2 * N), dict(records=records[:0]),
           dict(records=many)] + [dict(drop=n) for n in names[:7]]
    for case in bad:
        a = dict(dists=dists, samples=N, records=records)
        drop = case.pop("drop", None)
        a.update(case)
        g = {k: (0 if k == drop else v) for k, v in given.items()}
        with pytest.raises(E.NonLinearSystemError):
            s.tolerance_mc_device(x0.data_ptr(), pos, dists_of(E, a["dists"]), a["records"], a["samples"], stats.data_ptr(), totals.data_ptr(), 0,
                                  seed=SEED, factorial=True, **g)
    s.tolerance_mc_device(x0.data_ptr(), pos, dists_of(E, dists), records, 0, stats.data_ptr(), totals.data_ptr(), 0, seed=SEED, factorial=True,
                          **given)  # samples == 0: EZPZ_OK after the checks, nothing written
    torch.cuda.synchronize()
    assert [raw(o) for o in outs] + [raw(stats)] == before
    with pytest.raises(ValueError):
        s.tolerance_mc(x0_host, pos, dists_of(E, dists), records, N, factorial=True, quantiles=[0.5])


def test_corners_that_do_not_assemble_leave_the_records_incomplete(E):
    s, x0 = tri(E)
    res = s.tolerance_mc(x0, TRI_POS, dists_of(E, TRI_WIDE), TRI_MEASURE, 8, seed=SEED, keep=True, factorial=True, keep_coef=True)
    p = s.tolerance_mc(x0, TRI_POS, dists_of(E, TRI_WIDE), TRI_MEASURE, 8, seed=SEED, keep=True)
    print("ok corners of the widened triangle:", res.n_ok, "of 8; ok", res.ok.tolist())
    assert run_bytes_no_hist(res) == run_bytes_no_hist(p) and 0 < res.n_ok < 8 and res.n_ok == p.n_ok
    f = res.factorial
    assert np.all(f.complete == 0) and np.all(f.n_valid == res.stats["n_valid"]) and np.all(f.n_valid < 8) and np.all(f.corner_hi == 0)
    for a in parts(f)[1:] + [f.mean_dev, f.var, f.m_hi, f.m_lo]:
        assert np.all(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == 0x7FF8000000000000)
    assert same_bytes(parts(f), R.factorial(res.m, res.flags, res.ok, res.stats["nominal"].copy()))


def run_bytes_no_hist(r):
    return [r.stats.tobytes(), r.totals.tobytes(), r.params.tobytes(), r.m.tobytes(), r.flags.tobytes(), r.ok.tobytes()]


# ---- the meaning --------------------------------------------------------------------------------------------------------------------
HU, HV = 0.1, 0.2  # chosen before any run
POINT = O.stack([O.fixed(0, 1.0), O.fixed(1, 0.5), O.fixed(2, 0.0), O.fixed(3, 0.0)])  # the point (0, 1) at (1, 0.5) and the origin (2, 3)
POINT_X0 = np.array([1.0, 0.5, 0.0, 0.0])


def test_the_coefficients_are_the_closed_form(E):
    s = E.System(POINT, 4)
    res = s.tolerance_mc(POINT_X0, [0, 1], dists_of(E, [(mc_ref.CORNER, -HU, HU), (mc_ref.CORNER, -HV, HV)]),
                         O.stack([O.distance((2, 3), (0, 1), 0.0)]), 4, seed=SEED, keep=True, factorial=True, keep_coef=True)
    f = res.factorial
    assert res.n_ok == 4 and f.complete[0] == 1
    closed = [math.sqrt((1.0 + (HU if b & 1 else -HU)) ** 2 + (0.5 + (HV if b & 2 else -HV)) ** 2) for b in range(4)]
    worst = max(abs(float(res.m[b, 0]) - closed[b]) for b in range(4))
    print("max_b |m[b] - closed[b]| =", worst, "; m", res.m[:, 0].tolist(), "closed", closed)
    nominal = float(res.stats["nominal"][0])
    for S in range(4):
        want = math.fsum((closed[b] - nominal) * (1.0 if bin(b & S).count("1") % 2 == bin(S).count("1") % 2 else -1.0) for b in range(4)) / 4.0
        print("coef", S, float(f.coef[0, S]), "closed", want, "diff", abs(float(f.coef[0, S]) - want))
        assert abs(float(f.coef[0, S]) - want) <= worst + 4 * 2.0 ** -53, S
    pair = math.fsum(closed[b] * (1.0 if b in (0, 3) else -1.0) for b in range(4)) / 4.0
    assert f.pair[0, 0, 1] != 0 and (f.pair[0, 0, 1] > 0) == (pair > 0)
    assert f.corner_hi[0] == res.stats["argmax"][0] == 0b11 and f.worst_case(0)["hi_is_linear"]
