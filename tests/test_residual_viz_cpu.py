"""Residual-field rendering without a device: the colour map and the overlay of ezpz_amd.residual_viz (host functions of
the C ABI) against the five baseline images of the reference's own residual_viz tests, the PNG reader / writer, and what
the device entries answer before they need a system."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from residual_viz_common import BASELINES, KIND_VIEW, SCENES, VIEWPORT, kind_scene, moves_under_one_ulp, oracle_field

import ezpz_amd as E
from ezpz_amd import residual_viz as V
from ezpz_amd._lib import CViewport
from oracle import oracle as O


@pytest.mark.parametrize("name", sorted(SCENES))
def test_colormap_and_overlay_reproduce_the_reference_image(name):
    """Oracle residual per pixel -> ezpz_residual_colormap -> ezpz_residual_overlay: every one of the 65 536 pixels of the
    reference's baseline (ezpz/tests/residual_viz_baselines, rendered by its Rust code)."""
    rec, x_base, example, solution = SCENES[name]
    mag, _ = oracle_field(rec, x_base, 0, 1, VIEWPORT)
    rgb = V.colormap(mag)
    V.draw_overlay(rgb, VIEWPORT, example[0], example[1], solution[0], solution[1])
    want = V.load_png(os.path.join(BASELINES, name + ".png"))
    assert want.shape == (256, 256, 3)
    differing = int(np.any(rgb != want, axis=2).sum())
    assert differing == 0, differing


def test_colormap_edges():
    """mag_to_pixel (residual_viz.rs:72-81): threshold, rounding of the grey value (halves away from zero), integers,
    huge and non-finite magnitudes (Rust's saturating `as u8`: NaN -> 0)."""
    t = [64, 224, 208]
    g = lambda v: [v, v, v]
    cases = [
        (0.0, t), (0.0799999, t), (0.08, g(235)),  # 255 - 0.08 * 255 = 234.6
        (1.0, g(255)), (2.0, g(255)), (7.0, g(255)),
        (1.5, g(128)),            # 127.5 rounds away from zero
        (1.0 + 0.49 / 255, g(255)), (1.0 + 0.51 / 255, g(254)),  # either side of k + 0.5 / 255: 254.51 | 254.49
        (3.0 + 1.49 / 255, g(254)), (3.0 + 1.51 / 255, g(253)),
        (0.999999, g(0)),         # 255 - 254.9997 = 0.0003 -> 0
        (1e300, g(255)), (float("nan"), g(0)), (float("inf"), g(0)),
    ]
    got = V.colormap(np.array([c[0] for c in cases]))
    for (m, want), have in zip(cases, got.tolist()):
        assert have == want, (m, have, want)


def test_png_round_trip_and_fixtures(tmp_path):
    rng = np.random.default_rng(5)
    for h, w in ((17, 31), (4, 1), (5, 3), (2, 255)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        path = tmp_path / ("t_%d_%d.png" % (h, w))
        V.save_png(path, img)
        back = V.load_png(path)
        assert back.dtype == np.uint8 and np.array_equal(back, img)
    for name in SCENES:
        assert V.load_png(os.path.join(BASELINES, name + ".png")).shape == (256, 256, 3)


def test_png_reader_row_filters(tmp_path):
    """All five row filters, each applied by hand to a random image."""
    import struct
    import zlib

    rng = np.random.default_rng(6)
    h, w = 10, 7
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    flat = img.reshape(h, 3 * w).astype(np.int32)
    rows = bytearray()
    for y in range(h):
        kind = y % 5
        rows.append(kind)
        for i in range(3 * w):
            left = flat[y, i - 3] if i >= 3 else 0
            up = flat[y - 1, i] if y else 0
            ul = flat[y - 1, i - 3] if (y and i >= 3) else 0
            p = left + up - ul
            pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
            paeth = left if (pa <= pb and pa <= pc) else (up if pb <= pc else ul)
            pred = [0, left, up, (left + up) // 2, paeth][kind]
            rows.append((flat[y, i] - pred) & 255)
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))
    data = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(bytes(rows))) + chunk(b"IEND", b"")
    path = tmp_path / "filters.png"
    path.write_bytes(data)
    assert np.array_equal(V.load_png(path), img)


def test_entries_without_a_system():
    """No system can be created without a device; what can be asked: null system / viewport -> EZPZ_ERR_INVALID_ARGUMENT from
    both entries, and EzpzViewport's layout as the header declares it."""
    L = E.lib()
    vp = CViewport(-1.0, 1.0, -1.0, 1.0, 4, 4)
    x = np.zeros(4)
    mag = np.zeros(16)
    deg = C.c_uint64(0)
    assert L.ezpz_system_residual_field(None, x.ctypes.data, 0, 1, -1, C.byref(vp), mag.ctypes.data, None, C.byref(deg)) == -103
    assert L.ezpz_system_residual_field_device(None, x.ctypes.data, 0, 1, -1, C.byref(vp), mag.ctypes.data, None, None, None) == -103
    # (a viewport is looked at only behind the system, so a null viewport is asked of a null system too)
    assert L.ezpz_system_residual_field(None, x.ctypes.data, 0, 1, -1, None, mag.ctypes.data, None, None) == -103
    assert L.ezpz_system_residual_field_device(None, x.ctypes.data, 0, 1, -1, None, mag.ctypes.data, None, None, None) == -103
    rgb = np.zeros((4, 4, 3), np.uint8)
    assert L.ezpz_residual_overlay(rgb.ctypes.data, None, 0.0, 0.0, 0.0, 0.0) == -103
    assert L.ezpz_residual_overlay(None, C.byref(vp), 0.0, 0.0, 0.0, 0.0) == -103
    header = open(os.path.join(ROOT, "include", "ezpz_amd.h")).read()
    body = re.search(r"typedef struct EzpzViewport \{(.*?)\} EzpzViewport;", header, re.S).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in CViewport._fields_]
    assert C.sizeof(CViewport) == 40 and CViewport.width.offset == 32 and CViewport.height.offset == 36


def test_overlay_clips_and_draws_in_order():
    """The green disc is drawn last (it wins over the red one and the arrow); points outside the image are clipped."""
    vp = (0.0, 16.0, 0.0, 16.0, 16, 16)
    rgb = np.zeros((16, 16, 3), np.uint8)
    V.draw_overlay(rgb, vp, 8.0, 8.0, 8.0, 8.0)  # same pixel: no arrow (shorter than a pixel), green over red
    assert rgb[8, 8].tolist() == [0, 180, 0] and rgb[8, 13].tolist() == [0, 180, 0] and rgb[8, 14].tolist() == [0, 0, 0]
    rgb[:] = 0
    V.draw_overlay(rgb, vp, -100.0, 8.0, 3.0, 8.0)
    assert rgb[8, 3].tolist() == [0, 180, 0] and not (rgb[..., 0] == 255).any()


def test_kind_scenes_are_almost_everywhere_continuous():
    """The seeded scenes of tests/test_gpu_residual_viz.py (all 25 kinds): at no more than 0.1 % of a scene's pixels does the
    oracle's own magnitude move by more than the comparison's bar under one ulp of a swept coordinate -- the only pixels the
    device comparison may leave out."""
    from residual_viz_common import pixel_centres

    w, h = KIND_VIEW
    for kind in range(25):
        rec, x_base, vx, vy, viewport = kind_scene(kind)
        mag, _ = oracle_field(rec, x_base, vx, vy, viewport)
        xs, ys = pixel_centres(viewport)
        jumps = sum(moves_under_one_ulp(rec, x_base, vx, vy, xs[c], ys[r], mag[r, c]) for r in range(h) for c in range(w))
        print("kind %2d %-28s discontinuous pixels %d" % (kind, E.api.KIND_NAMES[kind], jumps))
        assert jumps <= (w * h) // 1000, (kind, jumps)
