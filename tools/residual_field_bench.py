"""Timing of the residual field (ezpz_system_residual_field*), printed as the text of profiles/residual_field.txt.

(a) host to host, one Distance constraint at 1024x1024: the new entry against the only earlier route, ezpz_system_eval_batch
    with one value vector per pixel -- taken from ANOTHER BUILD of the library (--old-lib: a build of the parent commit, which
    this process loads beside its own), interleaved, RUNS runs each.
(b) device resident at 4096x4096, rgb only and rgb + mag, for one Vertical constraint (a linear kind), one Distance
    constraint and every constraint of a connected sketch with one point swept: time per launch from events, interleaved,
    and bytes stored per second.
--launch-only SCENE: a few launches of one scene and nothing else (for rocprofv3 --kernel-trace / --pmc).

    python tools/residual_field_bench.py --old-lib /path/to/parent/libezpz_amd.so
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch  # (before the library: torch brings its own HIP runtime and must be the first to load one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ezpz_amd as E  # noqa: E402
from ezpz_amd._lib import CONSTRAINT_DTYPE, CViewport  # noqa: E402
from oracle import oracle as O  # noqa: E402

RUNS = 5


def scenes():
    from gen import connected_sketch

    recs, guess = connected_sketch(120, 11)
    k = 57
    return {
        "vertical": (O.stack([O.vertical((0, 1), (2, 3))]), np.zeros(4), 0, 1, 0, (-5.0, 5.0, -5.0, 5.0)),
        "distance": (O.stack([O.distance((0, 1), (2, 3), 3.0)]), np.zeros(4), 0, 1, 0, (-5.0, 5.0, -5.0, 5.0)),
        "sketch": (recs, guess, 2 * k, 2 * k + 1, -1, (guess[2 * k] - 1.0, guess[2 * k] + 1.0, guess[2 * k + 1] - 1.0, guess[2 * k + 1] + 1.0)),
    }


def device_launches(name, size, with_mag, repeats):
    """(times in ms per launch from events, bytes stored per launch)"""
    recs, base, vx, vy, sel, box = scenes()[name]
    system = E.System(recs, len(base))
    dev = torch.device("cuda:0")
    xb = torch.tensor(base, dtype=torch.float64, device=dev)
    rgb = torch.empty((size, size, 3), dtype=torch.uint8, device=dev)
    mag = torch.empty((size, size), dtype=torch.float64, device=dev) if with_mag else None
    vp = CViewport(*[float(v) for v in box], size, size)
    stream = torch.cuda.current_stream()

    def launch():
        rc = E.lib().ezpz_system_residual_field_device(system._h, xb.data_ptr(), vx, vy, sel, C.byref(vp), mag.data_ptr() if with_mag else None,
                                                       rgb.data_ptr(), None, stream.cuda_stream)
        assert rc == 0, rc

    launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        launch()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return times, size * size * (3 + (8 if with_mag else 0)), system


def old_route(lib_path, size):
    """The parent build's only way to such a field: one value vector per pixel through ezpz_system_eval_batch."""
    L = C.CDLL(lib_path)
    vp_ = C.c_void_p
    L.ezpz_system_create.argtypes = [vp_, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(vp_), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.ezpz_system_eval_batch.argtypes = [vp_, vp_, C.c_size_t, vp_, vp_, vp_]
    recs = O.stack([O.distance((0, 1), (2, 3), 3.0)]).astype(CONSTRAINT_DTYPE)
    h = vp_()
    ec, ev = C.c_int32(-1), C.c_int64(-1)
    assert L.ezpz_system_create(recs.ctypes.data, 1, 4, 0, 0, C.byref(h), C.byref(ec), C.byref(ev)) == 0
    xs = -5.0 + 10.0 * (np.arange(size) + 0.5) / size

    def run():
        t0 = time.perf_counter()
        x = np.zeros((size * size, 4))
        x[:, 0] = np.tile(xs, size)
        x[:, 1] = np.repeat(xs, size)
        r = np.empty((size * size, 1))
        jv = np.empty((size * size, 4))
        deg = np.empty(size * size, np.uint32)
        assert L.ezpz_system_eval_batch(h, x.ctypes.data, size * size, r.ctypes.data, jv.ctypes.data, deg.ctypes.data) == 0
        mag = np.abs(r).reshape(size, size)
        return time.perf_counter() - t0, mag

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old-lib", default=None)
    ap.add_argument("--old-commit", default="?")
    ap.add_argument("--new-commit", default="?")
    ap.add_argument("--launch-only", default=None)
    ap.add_argument("--mag", type=int, default=0)
    a = ap.parse_args()
    if a.launch_only:
        device_launches(a.launch_only, 4096, bool(a.mag), 5)
        return
    print("# tools/residual_field_bench.py: new build %s, old route from a build of %s" % (a.new_commit, a.old_commit))
    if a.old_lib:
        size = 1024
        old = old_route(a.old_lib, size)
        recs, base, vx, vy, sel, box = scenes()["distance"]
        system = E.System(recs, 4)

        def new():
            t0 = time.perf_counter()
            f = system.residual_field(base, vx, vy, (*box, size, size), constraint=0, want=("mag",))
            return time.perf_counter() - t0, f.mag

        old()
        new()
        t_old, t_new = [], []
        for _ in range(RUNS):
            dt, m_old = old()
            t_old.append(dt)
            dt, m_new = new()
            t_new.append(dt)
        print("(a) host to host, one Distance constraint, %dx%d magnitudes, seconds per call, interleaved" % (size, size))
        print("    old route (eval_batch, one value vector per pixel): " + " ".join("%.4f" % t for t in t_old))
        print("    new entry (ezpz_system_residual_field):             " + " ".join("%.4f" % t for t in t_new))
        print("    fastest old / slowest new = %.1f; fields agree to %.3g" % (min(t_old) / max(t_new), float(np.max(np.abs(m_old - m_new)))))
        assert max(t_new) < min(t_old), "the new entry must win outright"
    print("(b) device resident, 4096x4096, milliseconds per call (first launch + field kernel) from events, interleaved; stored GB/s of the median")
    cases = [(n, m) for n in ("vertical", "distance", "sketch") for m in (False, True)]
    results = {c: [] for c in cases}
    for _ in range(3):
        for c in cases:
            t, nbytes, _ = device_launches(c[0], 4096, c[1], RUNS)
            results[c] += t
    for (n, m), t in results.items():
        nbytes = 4096 * 4096 * (3 + (8 if m else 0))
        med = float(np.median(t))
        print("    %-9s %-9s min %.4f median %.4f max %.4f ms  -> %.0f GB/s stored (%d MB)" % (
            n, "rgb+mag" if m else "rgb", min(t), med, max(t), nbytes / med / 1e6, nbytes >> 20))


if __name__ == "__main__":
    main()
