"""GPU tests (-m gpu) of the sketch images (ezpz_sketch_image and its _device form, ezpz_system_tolerance_mc_image, the CLI's -o;
csrc/sketch_image.hip).  The counts are integers decided by one rule: the device, the host body and the numpy
restatement (tests/sketch_image_ref.py) agree exactly, whatever the batch, the rounds and the streams -- every comparison here is
array_equal, there is no tolerance.  The view is 200 x 136 throughout: four by three tiles of 64 pixels, the last of each kind partial.
The CLI's picture is compared with compose(sketch_image(...)) on the values of a Python solve of the same text: both go through
ezpz_solve with the same records and guesses."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import oracle as O

import sketch_image_cases as K
import sketch_image_ref as R

pytestmark = pytest.mark.gpu

CASES = K.cases()
_CACHE = {}


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host_body_equals_numpy(E, name):
    x, ok, items, view, n_layers = CASES[name]
    counts, info = R.image(x, ok, items, view, n_layers)
    host = E.sketch_image_host(x, items, view, n_layers, ok=ok)
    got = E.sketch_image(x, items, view, n_layers, ok=ok)
    assert got.counts.dtype == np.uint32 and got.counts.shape == (n_layers, K.H, K.W)
    assert np.array_equal(got.counts, counts) and np.array_equal(host.counts, counts)
    assert tuple(got.info) == info == tuple(host.info)


def test_layers_and_item_order(E):
    x, items, shuffled, view, n_layers = K.layered()
    a, b = E.sketch_image(x, items, view, n_layers), E.sketch_image(x, shuffled, view, n_layers)
    assert a.counts.shape[0] == 5 and np.array_equal(a.counts, b.counts) and a.info == b.info
    want, info = R.image(x, None, items, view, n_layers)
    assert np.array_equal(a.counts, want) and tuple(a.info) == info
    # accumulate through the host form: the caller's counts are uploaded first
    twice = E.sketch_image(x, shuffled, view, n_layers, accumulate=a)
    assert np.array_equal(twice.counts, 2 * want) and tuple(twice.info) == tuple(2 * v for v in info)
    # no variants, no items: the outputs are zeroed, the variants counted
    empty = E.sketch_image(np.zeros((0, x.shape[1])), items, view, n_layers)
    assert not empty.counts.any() and tuple(empty.info) == (0, 0, 0, 0)
    none = E.sketch_image(np.tile(x, (3, 1)), [], view, 2, ok=[1, 0, 1])
    assert none.counts.shape[0] == 2 and not none.counts.any() and tuple(none.info) == (3, 1, 0, 0)


# ---- 4099 jittered variants of a 10-item list ------------------------------------------------------------------------------------------
def cloud_reference():
    """The numpy sum, once: slices of variants side by side (integer counts add)."""
    if "cloud" not in _CACHE:
        x, items, view, n_layers = K.cloud()
        with ThreadPoolExecutor(8) as pool:
            parts = list(pool.map(lambda part: R.image(part, None, items, view, n_layers, block=32), np.array_split(x, 32)))
        counts = sum(c.astype(np.uint64) for c, _ in parts)
        assert counts.max() > 1000  # (a cloud: the variants land on the same pixels)
        _CACHE["cloud"] = (counts.astype(np.uint32), tuple(sum(i[k] for _, i in parts) for k in range(4)))
    return _CACHE["cloud"]


def test_cloud_in_one_call_equals_the_numpy_sum(E):
    x, items, view, n_layers = K.cloud()
    want, info = cloud_reference()
    got = E.sketch_image(x, items, view, n_layers)
    assert np.array_equal(got.counts, want) and tuple(got.info) == info and info[0] == 4099


def test_cloud_in_two_accumulating_calls(E):
    x, items, view, n_layers = K.cloud()
    want, info = cloud_reference()
    first = E.sketch_image(x[:2000], items, view, n_layers)
    both = E.sketch_image(x[2000:], items, view, n_layers, accumulate=first)
    assert tuple(first.info)[0] == 2000 and 0 < first.counts.sum() < want.sum()
    assert np.array_equal(both.counts, want) and tuple(both.info) == info


def test_cloud_on_two_streams_joined_by_an_event(E):
    import torch

    x, items, view, n_layers = K.cloud()
    want, info = cloud_reference()
    xa, xb = torch.from_numpy(x[:2000].copy()).cuda(), torch.from_numpy(x[2000:].copy()).cuda()
    counts = torch.full((n_layers, K.H, K.W), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # (the first call zeroes)
    inf = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        E.sketch_image_device(xa.data_ptr(), 0, 2000, x.shape[1], items, view, n_layers, counts.data_ptr(), inf.data_ptr(), accumulate=False,
                              stream=s1.cuda_stream)
        joined = torch.cuda.Event()
        joined.record(s1)
    s2.wait_event(joined)
    with torch.cuda.stream(s2):
        E.sketch_image_device(xb.data_ptr(), 0, 2099, x.shape[1], items, view, n_layers, counts.data_ptr(), inf.data_ptr(), accumulate=True,
                              stream=s2.cuda_stream)
    s2.synchronize()
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want)
    assert tuple(int(v) for v in inf.cpu().numpy()) == info


# ---- tolerance_mc(..., image=...): the triangle of tests/test_gpu_tolerance_mc.py, whose third side can outgrow the other two ----------
A, B, Cc = (0, 1), (2, 3), (4, 5)
TRIANGLE = O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(3, 0.0), O.distance(A, B, 1.0), O.distance(B, Cc, 1.0), O.distance(Cc, A, 1.9)])
TRI_POS, TRI_NOMINAL = [3, 4, 5], np.array([1.0, 1.0, 1.9])
TRI_DISTS = [(1, -0.05, 0.05), (1, -0.05, 0.05), (1, -0.3, 0.3)]  # UNIFORM: the host sampler's draws are the device's, bit for bit
TRI_MEASURE = O.stack([O.vertical_distance(Cc, A, 0.0), O.distance(B, Cc, 0.0)])
TRI_VIEW = (-0.6, -0.45, 80.0, K.W, K.H)
TRI_ITEMS = [(K.POINT, 0, 0, A, 4.0), (K.POINT, 0, 0, B, 4.0), (K.POINT, 0, 0, Cc, 4.0), (K.SEGMENT, 1, 0, A + B, 1.5), (K.SEGMENT, 1, 0, B + Cc, 1.5),
             (K.SEGMENT, 1, 0, Cc + A, 1.5), (K.CIRCLE, 2, 0, (4, 5, 2), 1.0)]  # (the circle: about C, with B's x as its radius)
SEED, SAMPLES = 0xC0FFEE1234, 1000
TRI_LIMITS, TRI_HIST = ((0.0, 0.9), (0.6, 1.05)), ((0.0, 0.9), (0.7, 1.1), 8)


def triangle(E):
    if "tri" not in _CACHE:
        s = E.System(TRIANGLE, 6)
        x0, st, _ = s.solve_batch(np.array([[0.0, 0.0, 1.0, 0.0, 0.9, 0.4]]))
        assert st["converged"][0] and st["n_unsatisfied"][0] == 0
        _CACHE["tri"] = (s, x0[0])
    return _CACHE["tri"]


def tri_run(E, chunk, image):
    s, x0 = triangle(E)
    dists = [E.McDist(*d) for d in TRI_DISTS]
    return s.tolerance_mc(x0, TRI_POS, dists, TRI_MEASURE, SAMPLES, seed=SEED, limits=TRI_LIMITS, hist=TRI_HIST, chunk=chunk,
                          image=E.ImageConfig(TRI_ITEMS, TRI_VIEW, 3) if image else None)


def tri_chain(E):
    """The picture from the entries that existed before: the host sampler, solve_batch_params, sketch_image with the solves' verdicts."""
    if "chain" not in _CACHE:
        s, x0 = triangle(E)
        p = E.mc_sample(SEED, [E.McDist(*d) for d in TRI_DISTS], TRI_NOMINAL, 0, SAMPLES)
        x, st, _ = s.solve_batch_params(np.tile(x0, (SAMPLES, 1)), TRI_POS, p)
        ok = ((st["converged"] != 0) & (st["n_unsatisfied"] == 0)).astype(np.uint8)
        _CACHE["chain"] = (E.sketch_image(x, TRI_ITEMS, TRI_VIEW, 3, ok=ok), ok)
    return _CACHE["chain"]


@pytest.mark.parametrize("chunk", [256, 1024])  # four rounds, the last partial; one round
def test_tolerance_mc_with_an_image(E, chunk):
    plain, res = tri_run(E, chunk, False), tri_run(E, chunk, True)
    assert not hasattr(plain, "image")
    for name in ("stats", "totals", "hist"):
        assert getattr(res, name).tobytes() == getattr(plain, name).tobytes(), name
    assert 300 <= res.n_ok <= 900  # (variants that do not assemble, and they are not drawn)
    want, ok = tri_chain(E)
    assert int(ok.sum()) == res.n_ok
    assert res.image.dtype == np.uint32 and res.image.shape == (3, K.H, K.W) and np.array_equal(res.image, want.counts)
    assert res.image_info == want.info and res.image_info.variants == SAMPLES and res.image_info.masked == SAMPLES - res.n_ok
    assert res.image[0].max() == res.n_ok  # (A is fixed: every drawn variant covers its disc's centre)


def test_tolerance_mc_image_device_form_on_another_stream(E):
    import torch

    s, x0 = triangle(E)
    want = tri_run(E, 256, True)
    x0_dev = torch.from_numpy(x0).cuda()
    out = lambda n: torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")  # noqa: E731
    stats, totals, hist, counts, info = out(2 * 88), out(24), out(2 * 10 * 8), out(3 * K.H * K.W * 4), out(32)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s.tolerance_mc_device(x0_dev.data_ptr(), TRI_POS, [E.McDist(*d) for d in TRI_DISTS], TRI_MEASURE, SAMPLES, stats.data_ptr(), totals.data_ptr(),
                              hist.data_ptr(), seed=SEED, limits=TRI_LIMITS, hist=TRI_HIST, chunk=256, stream=stream.cuda_stream,
                              image=E.ImageConfig(TRI_ITEMS, TRI_VIEW, 3), image_counts_ptr=counts.data_ptr(), image_info_ptr=info.data_ptr())
    stream.synchronize()
    got = [t.cpu().numpy().tobytes() for t in (stats, totals, hist, counts, info)]
    assert got == [want.stats.tobytes(), want.totals.tobytes(), want.hist.tobytes(), want.image.tobytes(),
                   np.array(tuple(want.image_info), np.uint64).tobytes()]


def test_tolerance_mc_image_argument_errors_and_kinds(E):
    s, x0 = triangle(E)
    dists = [E.McDist(*d) for d in TRI_DISTS]
    run = lambda **kw: s.tolerance_mc(x0, TRI_POS, dists, TRI_MEASURE, 300, seed=SEED, **kw)  # noqa: E731
    bad = [E.ImageConfig([(K.POINT, 0, 0, (0, 6), 1.0)], TRI_VIEW, 1),          # an id past the system's variables
           E.ImageConfig([(K.POINT, 3, 0, (0, 1), 1.0)], TRI_VIEW, 3),          # a layer past n_layers
           E.ImageConfig(TRI_ITEMS, (0.0, 0.0, 0.0, K.W, K.H), 3),              # a view without a scale
           E.ImageConfig(TRI_ITEMS, TRI_VIEW, 9)]
    for image in bad:
        with pytest.raises(E.NonLinearSystemError) as e:
            run(image=image)
        assert e.value.code == -103
    for kind in (dict(contributors=True), dict(quantiles=[0.5]), dict(factorial=True)):
        with pytest.raises(ValueError):
            run(image=E.ImageConfig(TRI_ITEMS, TRI_VIEW, 3), **kind)
    # the run's own argument errors come first, and no samples is no picture
    with pytest.raises(E.NonLinearSystemError):
        s.tolerance_mc(x0, [99], dists[:1], TRI_MEASURE, 300, image=E.ImageConfig(TRI_ITEMS, TRI_VIEW, 3))
    none = s.tolerance_mc(x0, TRI_POS, dists, TRI_MEASURE, 0, image=E.ImageConfig(TRI_ITEMS, TRI_VIEW, 3))
    assert none.samples == 0 and not none.image.any() and tuple(none.image_info) == (0, 0, 0, 0)


def test_a_plain_run_enqueues_no_picture(E):
    """csrc/call_trace.hpp: the stamps 140 and 141 are the rasteriser's.  A run with an image leaves them once per round; a plain run
    on the same system, before and after it, leaves none."""
    def stamps(image):
        trace = np.zeros(1024, dtype=np.uint64)
        E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
        try:
            tri_run(E, 256, image)
        finally:
            k = E.lib().ezpz_debug_call_trace(None, 0)
        return [int(v) for v in trace[:k:2]]

    before, with_image, after = stamps(False), stamps(True), stamps(False)
    assert with_image.count(141) == 4 and not {140, 141} & set(before) and not {140, 141} & set(after)
    assert [v for v in with_image if v not in (140, 141)] == after


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_solved_sketch(E, tmp_path):
    path = os.path.join(GOLDEN, "test_cases", "two_rectangles", "problem.md")
    png = str(tmp_path / "sketch.png")
    cli = os.path.join(ROOT, "ezpz_amd", "ezpz-amd")
    r = subprocess.run(["timeout", "-k", "10", "120", cli, "-f", path, "--show-points", "-o", png], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert ("Plot saved to %s" % png) in r.stdout.splitlines() and "PNG output is not part" not in r.stderr
    problem = E.textual.Problem.from_str(open(path).read())
    x = problem.to_constraint_system().solve_no_metadata().final_values()
    # (the printed points are those values, to the two digits the CLI prints)
    shown = [line.split(": ")[1] for line in r.stdout.splitlines() if line.startswith("\tp")]
    assert shown == ["(%.2f, %.2f)" % (x[2 * i], x[2 * i + 1]) for i in range(8)]
    items = E.items_from_problem(problem)
    view = E.fit_view(x, items, 1600, 1600)
    image = E.sketch_image(x, items, view, n_layers=5)
    want = E.compose(image.counts, E.REFERENCE_LAYERS)[::-1]
    got = E.residual_viz.load_png(png)
    assert got.shape == (1600, 1600, 3) and np.array_equal(got, want)
    # the picture holds what it should: white paper, the points' and the lines' colours, nothing of the circles' or arcs'
    colours = {tuple(c) for c in np.unique(got.reshape(-1, 3), axis=0)}
    assert colours == {(255, 255, 255), (0x58, 0x50, 0x8d), (0xff, 0xa6, 0x00)}
    assert image.info.increments == int(image.counts.sum()) > 8 * 300 and image.info.items_skipped == 0
    # the numpy rule on the same values, at the CLI's own size
    assert np.array_equal(image.counts, R.image(x[None, :], None, [tuple(it) for it in items], tuple(view), 5)[0])
    # ... and the Python writer's file reads back the same
    mine = str(tmp_path / "mine.png")
    E.save_sketch_png(mine, x, items, view)
    assert np.array_equal(E.residual_viz.load_png(mine), want)
