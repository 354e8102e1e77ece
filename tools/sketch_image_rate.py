"""The rate of the sketch images (ezpz_sketch_image_device, ezpz_system_tolerance_mc_image_device), printed as the text
of profiles/sketch_image_rate.txt.

Per system (a block system; one connected sketch of tests/gen.py), at 1600 x 1600 pixels with ten items (five discs of radius 10,
five strokes 3 wide) over the view `fit_view` gives the solved sketch:
  1. the rasteriser alone on variants that are on the device already: 1 (the CLI's case), 4096 and 1 048 576 -- the solves of a
     tolerance run's own draws with the zones of profiles/tolerance_mc_rate.txt -- in variants/s and in LDS adds/s (the info
     record's increments over the time: every add goes through LDS)
  2. ezpz_system_tolerance_mc_image_device against ezpz_system_tolerance_mc_device on the same samples, in rounds of 65536: what the
     tail adds in total and per round
  3. the route that existed before, at 4096 variants: x to the host and the numpy rule (tests/sketch_image_ref.py), restricted to
     each item's box over all variants, as a caller would write it -- timed on HOST_VARIANTS of them, the rule's time scaled to 4096

Device events on the stream around the enqueued work; WARMUP untimed runs of each form, then REPEATS timed runs, the forms of one
section alternating; median (min .. max).

    python tools/sketch_image_rate.py > profiles/sketch_image_rate.txt
"""
import os
import sys
import time

import numpy as np
import torch  # (before the library: torch brings its own HIP runtime and must be the first to load one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ezpz_amd as E  # noqa: E402
import sketch_image_ref as R  # noqa: E402
from ezpz_amd._lib import MC_STATS_DTYPE, MC_TOTALS_DTYPE, STATUS_DTYPE  # noqa: E402
from oracle import oracle as O  # noqa: E402

WARMUP, REPEATS = 2, 7
SIDE, LAYERS = 1600, 2
BATCHES = (1, 4096, 1048576)
SAMPLES, CHUNK = 1048576, 65536
MAX_DRIVEN, SIGMA, TRUNC = 8, 1e-3, 3.0
HOST_VARIANTS = 256


def systems():
    from gen import connected_sketch

    block = E.textual.Problem.from_str(E.textual.gen_big_problem(16)).to_constraint_system()
    recs, g = connected_sketch(40, 11)
    return [("block system, 16 blocks, %d variables" % block.num_vars, E.System(block.records, block.num_vars), block.records,
             np.asarray(block.guesses, dtype=float)),
            ("connected sketch, %d variables" % len(g), E.System(recs, len(g)), recs, np.asarray(g, dtype=float))]


def driven(recs):
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    return np.ascontiguousarray(pos[np.linspace(0, len(pos) - 1, min(MAX_DRIVEN, len(pos))).astype(int)])


def measurements(n):
    pts = n // 2
    pt = lambda i: (2 * i, 2 * i + 1)  # noqa: E731
    pairs = [(0, pts - 1), (1, pts // 2), (pts // 3, pts - 2), (2, pts - 3)]
    return O.stack([O.distance(pt(a), pt(b), 0.0) for a, b in pairs] + [O.horizontal_distance(pt(a), pt(b), 0.0) for a, b in pairs])


def drawing(n):
    pts = n // 2
    chosen = [int(v) for v in np.linspace(0, pts - 1, 6).astype(int)]
    items = [E.DrawItem.point(2 * p, 2 * p + 1, 10.0, 0) for p in chosen[:5]]
    items += [E.DrawItem.segment(2 * a, 2 * a + 1, 2 * b, 2 * b + 1, 1.5, 1) for a, b in zip(chosen[:5], chosen[1:])]
    return items


def timed(stream, f):
    """milliseconds between two events on the stream around what f enqueues there"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    start.record(stream)
    f()
    end.record(stream)
    end.synchronize()
    return start.elapsed_time(end)


def measure(stream, forms):
    for _ in range(WARMUP):
        for f in forms:
            timed(stream, f)
    ts = [[] for _ in forms]
    for _ in range(REPEATS):
        for i, f in enumerate(forms):
            ts[i].append(timed(stream, f))
    return [np.asarray(t) for t in ts]


def spread(t):
    return "%10.3f ms (%.3f .. %.3f)" % (np.median(t), t.min(), t.max())


def case(name, system, recs, g, stream):
    n, pos, records = len(g), driven(recs), measurements(len(g))
    k, n_meas = len(pos), len(records)
    solved, st, _ = system.solve_batch(g[None, :])
    assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
    items = drawing(n)
    view = E.fit_view(solved[0], items, SIDE, SIDE)
    own = recs["param"][pos].astype(np.float64)
    sigma = SIGMA * np.maximum(1.0, np.abs(own))
    dists = [E.McDist.normal(float(s), TRUNC) for s in sigma]
    h = stream.cuda_stream
    print("-- %s; %d driven (normal, sigma %g x max(1, |value|), cut at %g sigma); %d items on %d layers, %d x %d pixels, scale %.4g pixels a unit"
          % (name, k, SIGMA, TRUNC, len(items), LAYERS, SIDE, SIDE, view.scale))
    with torch.cuda.stream(stream):
        x0 = torch.from_numpy(solved[0]).cuda()
        counts = torch.zeros((LAYERS, SIDE, SIDE), dtype=torch.int32, device="cuda")
        info = torch.zeros(4, dtype=torch.int64, device="cuda")
        # the variants: the solves of the run's own draws, in the run's rounds
        params = torch.from_numpy(E.mc_sample(1, dists, own, 0, SAMPLES)).cuda()
        x_all = torch.zeros((SAMPLES, n), dtype=torch.float64, device="cuda")
        status = torch.zeros((SAMPLES, STATUS_DTYPE.itemsize // 4), dtype=torch.int32, device="cuda")
        x_in = x0.repeat(CHUNK, 1)
        for first in range(0, SAMPLES, CHUNK):
            system.solve_batch_params_device(x_in.data_ptr(), pos, params[first:].data_ptr(), CHUNK, x_all[first:].data_ptr(), status[first:].data_ptr(), stream=h)
        ok = ((status[:, 1] != 0) & (status[:, 2] == 0)).to(torch.uint8).contiguous()
    stream.synchronize()
    print("   variants solved: %d of %d" % (int(ok.sum()), SAMPLES))

    # 1. the rasteriser alone
    for batch in BATCHES:
        def draw():
            E.sketch_image_device(x_all.data_ptr(), ok.data_ptr(), batch, n, items, view, LAYERS, counts.data_ptr(), info.data_ptr(), stream=h)
        (t,) = measure(stream, [draw])
        adds = int(info.cpu().numpy()[3])
        print("   rasteriser, %7d variants  %s  %12.0f variants/s  %.3g LDS adds/s (%d adds, %d pixels touched)"
              % (batch, spread(t), batch / (np.median(t) * 1e-3), adds / (np.median(t) * 1e-3), adds, int((counts != 0).sum())))
        sys.stdout.flush()
    cloud = counts.cpu().numpy().view(np.uint32).copy()

    # 2. the run with and without the picture
    with torch.cuda.stream(stream):
        stats = torch.zeros(n_meas * MC_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        totals = torch.zeros(MC_TOTALS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

    def run(image):
        kw = dict(image=E.ImageConfig(items, view, LAYERS), image_counts_ptr=counts.data_ptr(), image_info_ptr=info.data_ptr()) if image else {}
        system.tolerance_mc_device(x0.data_ptr(), pos, dists, records, SAMPLES, stats.data_ptr(), totals.data_ptr(), seed=1, chunk=CHUNK, stream=h, **kw)

    plain, with_image = measure(stream, [lambda: run(False), lambda: run(True)])
    differ = int((counts.cpu().numpy().view(np.uint32) != cloud).sum())
    rounds = SAMPLES // CHUNK
    added = np.median(with_image) - np.median(plain)
    print("   tolerance_mc, %d samples in %d rounds: plain %s" % (SAMPLES, rounds, spread(plain)))
    print("                                         with image %s   the tail adds %.3f ms, %.3f ms a round (%.1f%% of the plain run)"
          % (spread(with_image), added, added / rounds, 100.0 * added / np.median(plain)))
    print("   pixels of the run's picture that differ from the rasteriser's on the host sampler's draws: %d (normal draws agree to 1e-13 sigma)" % differ)
    sys.stdout.flush()

    # 3. the route that existed before, at 4096 variants
    t0 = time.perf_counter()
    x_host = x_all[:4096].cpu().numpy()
    ok_host = ok[:4096].cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    part = host_route(x_host[:HOST_VARIANTS], ok_host[:HOST_VARIANTS], items, view)
    t_rule = time.perf_counter() - t0
    with torch.cuda.stream(stream):
        E.sketch_image_device(x_all.data_ptr(), ok.data_ptr(), HOST_VARIANTS, n, items, view, LAYERS, counts.data_ptr(), info.data_ptr(), stream=h)
    stream.synchronize()
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), part), "the host route draws another picture"
    print("   host route, 4096 variants: x to the host %.3f ms; the numpy rule on %d of them %.1f ms, x %d = %.0f ms for 4096 (scaled, not measured)"
          % (t_copy * 1e3, HOST_VARIANTS, t_rule * 1e3, 4096 // HOST_VARIANTS, t_rule * 1e3 * (4096 // HOST_VARIANTS)))
    sys.stdout.flush()


def host_route(x, ok, items, view):
    """The numpy rule on each item's box over all variants (grown by a pixel), not on the whole view."""
    counts = np.zeros((LAYERS, SIDE, SIDE), np.uint32)
    x = x[ok != 0]
    for it in items:
        ids, pairs = it.ids, len(it.ids) // 2
        u = np.concatenate([(x[:, ids[2 * j]] - view.x_min) * view.scale for j in range(pairs)])
        v = np.concatenate([(x[:, ids[2 * j + 1]] - view.y_min) * view.scale for j in range(pairs)])
        x0, x1 = max(int(u.min() - it.half_width) - 2, 0), min(int(u.max() + it.half_width) + 2, SIDE - 1)
        y0, y1 = max(int(v.min() - it.half_width) - 2, 0), min(int(v.max() + it.half_width) + 2, SIDE - 1)
        if x0 > x1 or y0 > y1:
            continue
        # (the rule at the view's own pixel centres: a crop with an origin of its own would round otherwise)
        X = (np.arange(x0, x1 + 1, dtype=np.float64) + 0.5)[None, None, :]
        Y = (np.arange(y0, y1 + 1, dtype=np.float64) + 0.5)[None, :, None]
        p = []
        for j in range(pairs):
            p.append(((x[:, ids[2 * j]] - view.x_min) * view.scale)[:, None, None])
            p.append(((x[:, ids[2 * j + 1]] - view.y_min) * view.scale)[:, None, None])
        for at in range(0, len(x), 16):
            part = [q[at:at + 16] for q in p]
            counts[it.layer, y0:y1 + 1, x0:x1 + 1] += R.covered(it.kind, it.flags, part, it.half_width, X, Y).sum(axis=0, dtype=np.uint32)
    return counts


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/sketch_image_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("Sketch images (ezpz_sketch_image_device, ezpz_system_tolerance_mc_image_device) on", torch.cuda.get_device_name(0))
    print("device events on the stream around the enqueued work; %d warm-up runs of each form, then %d timed runs, the forms of one section"
          % (WARMUP, REPEATS))
    print("alternating; median (min .. max).  The host route: host clock.")
    for name, system, recs, g in systems():
        case(name, system, recs, g, stream)


if __name__ == "__main__":
    main()
