"""Residual-field rendering: the reference's `residual_viz` module (ezpz/src/residual_viz.rs) on the device.

The residual magnitude of a constraint -- or of a whole system -- is drawn as a 2-D scalar field while one point sweeps a
viewport: turquoise where it is near zero, rings of its fractional part elsewhere, "a sanity check when changing residual
math: the image should change".  The field and its colours come from the HIP kernel behind `ezpz_system_residual_field`;
the overlay (example point, solution point, arrow) is drawn by `ezpz_residual_overlay` on the host.  PNG files are read
and written with the standard library alone.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import struct
import zlib
from collections import namedtuple
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import CViewport, lib
from . import api as _api

# the example points of the reference's pictures (residual_viz.rs:19-32)
EXAMPLE_POINT = (3.0, 2.0)
DISTANCE_EXAMPLE_POINT = (4.5, 3.0)
PERP_DISTANCE_EXAMPLE_POINT = (-2.0, 5.0)
VERTICAL_HORIZONTAL_EXAMPLE_POINT = (3.0, 2.0)

Viewport = namedtuple("Viewport", "x_min x_max y_min y_max width height")
Field = namedtuple("Field", "mag rgb degenerate_pixels")


def _viewport(viewport) -> CViewport:
    v = Viewport(*viewport)
    return CViewport(float(v.x_min), float(v.x_max), float(v.y_min), float(v.y_max), int(v.width), int(v.height))


def residual_field(system_or_records, x_base, var_x: int, var_y: int, viewport, constraint: Optional[int] = None,
                   want: Sequence[str] = ("mag", "rgb"), overlay: Optional[Tuple[float, float]] = None) -> Field:
    """The field of `constraint` (a position in the constraint list; None: all constraints) while variables var_x / var_y
    of `x_base` sweep `viewport` = (x_min, x_max, y_min, y_max, width, height).  Returns Field(mag (H, W) float64,
    rgb (H, W, 3) uint8, degenerate pixels); an output not named in `want` is None.  `overlay` = (example_x, example_y)
    draws the red point there and the green one where an ordinary solve from x_base, with the swept point started at the
    example, lands."""
    x_base = np.ascontiguousarray(x_base, dtype=np.float64).reshape(-1)
    system = system_or_records if isinstance(system_or_records, _api.System) else _api.System(system_or_records, len(x_base))
    if len(x_base) != system.n_vars:
        raise ValueError("x_base must hold one value per variable")
    unknown = set(want) - {"mag", "rgb"}
    if unknown:
        raise ValueError("unknown outputs: %s" % sorted(unknown))
    vp = _viewport(viewport)
    mag = np.empty((vp.height, vp.width), np.float64) if "mag" in want else None
    rgb = np.empty((vp.height, vp.width, 3), np.uint8) if ("rgb" in want or overlay is not None) else None
    deg = C.c_uint64(0)
    rc = lib().ezpz_system_residual_field(system._h, x_base.ctypes.data, var_x, var_y, -1 if constraint is None else int(constraint),
                                          C.byref(vp), mag.ctypes.data if mag is not None else None,
                                          rgb.ctypes.data if rgb is not None else None, C.byref(deg))
    if rc != 0:
        raise _api.NonLinearSystemError(rc)
    if overlay is not None:
        start = x_base.copy()
        start[var_x], start[var_y] = overlay
        solved, _, _ = system.solve_batch(start[None, :])
        draw_overlay(rgb, viewport, overlay[0], overlay[1], float(solved[0, var_x]), float(solved[0, var_y]))
    return Field(mag, rgb, int(deg.value))


def colormap(mag) -> np.ndarray:
    """`mag_to_pixel` (residual_viz.rs:72-81) of every magnitude: an array of mag's shape + (3,), uint8.  Host only."""
    mag = np.ascontiguousarray(mag, dtype=np.float64)
    rgb = np.empty(mag.shape + (3,), np.uint8)
    lib().ezpz_residual_colormap(mag.ctypes.data, mag.size, rgb.ctypes.data)
    return rgb


def draw_overlay(rgb: np.ndarray, viewport, example_x: float, example_y: float, solution_x: float, solution_y: float) -> np.ndarray:
    """`draw_solver_overlay` (residual_viz.rs:186-200) into an (H, W, 3) uint8 image, in place.  Host only."""
    vp = _viewport(viewport)
    if rgb.dtype != np.uint8 or rgb.shape != (vp.height, vp.width, 3) or not rgb.flags["C_CONTIGUOUS"]:
        raise ValueError("rgb must be a contiguous (height, width, 3) uint8 array of the viewport's size")
    rc = lib().ezpz_residual_overlay(rgb.ctypes.data, C.byref(vp), example_x, example_y, solution_x, solution_y)
    if rc != 0:
        raise _api.NonLinearSystemError(rc)
    return rgb


def _render(records, x_base, viewport, example, solution) -> np.ndarray:
    rgb = residual_field(records, x_base, 0, 1, viewport, constraint=0, want=("rgb",)).rgb
    return draw_overlay(rgb, viewport, example[0], example[1], solution[0], solution[1])


def render_points_coincident_residual_to_image(fixed_x, fixed_y, x_min, x_max, y_min, y_max, width, height) -> np.ndarray:
    """residual_viz.rs:206-252: point (ids 0, 1) swept, PointsCoincident with the fixed point (ids 2, 3)."""
    rec = _api._rec(_api.POINTS_COINCIDENT, [0, 1, 2, 3])
    return _render([rec], [0.0, 0.0, fixed_x, fixed_y], (x_min, x_max, y_min, y_max, width, height), EXAMPLE_POINT, (fixed_x, fixed_y))


def render_distance_residual_to_image(fixed_x, fixed_y, target_distance, x_min, x_max, y_min, y_max, width, height) -> np.ndarray:
    """residual_viz.rs:259-316; the green point is the point of the circle in the example's radial direction (:297-313)."""
    rec = _api._rec(_api.DISTANCE, [0, 1, 2, 3], target_distance)
    ex, ey = DISTANCE_EXAMPLE_POINT
    dx, dy = ex - fixed_x, ey - fixed_y
    dist = math.hypot(dx, dy)
    if dist > 1e-10:
        sol = (fixed_x + dx / dist * target_distance, fixed_y + dy / dist * target_distance)
    else:
        sol = (fixed_x + target_distance, fixed_y)
    return _render([rec], [0.0, 0.0, fixed_x, fixed_y], (x_min, x_max, y_min, y_max, width, height), (ex, ey), sol)


def render_point_line_distance_residual_to_image(line_p0_x, line_p0_y, line_p1_x, line_p1_y, target_distance, x_min, x_max,
                                                 y_min, y_max, width, height) -> np.ndarray:
    """residual_viz.rs:329-383; the green point lies at the target distance on the example's side of the line (:353-381)."""
    rec = _api._rec(_api.POINT_LINE_DISTANCE, [0, 1, 2, 3, 4, 5], target_distance)
    a, b = line_p0_y - line_p1_y, line_p1_x - line_p0_x
    c = line_p0_x * line_p1_y - line_p1_x * line_p0_y
    denom = math.hypot(a, b)
    denom = denom if denom > 1e-10 else 1.0
    ex, ey = PERP_DISTANCE_EXAMPLE_POINT
    actual = (a * ex + b * ey + c) / denom
    sol = (ex + a / denom * (target_distance - actual), ey + b / denom * (target_distance - actual))
    return _render([rec], [0.0, 0.0, line_p0_x, line_p0_y, line_p1_x, line_p1_y], (x_min, x_max, y_min, y_max, width, height),
                   (ex, ey), sol)


def render_vertical_residual_to_image(fixed_x, fixed_y, x_min, x_max, y_min, y_max, width, height) -> np.ndarray:
    """residual_viz.rs:388-430: the green point keeps the example's y (:424-428)."""
    rec = _api._rec(_api.VERTICAL, [0, 1, 2, 3])
    ex, ey = VERTICAL_HORIZONTAL_EXAMPLE_POINT
    return _render([rec], [0.0, 0.0, fixed_x, fixed_y], (x_min, x_max, y_min, y_max, width, height), (ex, ey), (fixed_x, ey))


def render_horizontal_residual_to_image(fixed_x, fixed_y, x_min, x_max, y_min, y_max, width, height) -> np.ndarray:
    """residual_viz.rs:435-477: the green point keeps the example's x (:471-475)."""
    rec = _api._rec(_api.HORIZONTAL, [0, 1, 2, 3])
    ex, ey = VERTICAL_HORIZONTAL_EXAMPLE_POINT
    return _render([rec], [0.0, 0.0, fixed_x, fixed_y], (x_min, x_max, y_min, y_max, width, height), (ex, ey), (ex, fixed_y))


def render_points_coincident_residual(path, fixed_x, fixed_y, x_min, x_max, y_min, y_max, width, height) -> None:
    """residual_viz.rs:484-503: the picture as a PNG file at `path` (its directory is created)."""
    parent = os.path.dirname(os.fspath(path))
    if parent:
        os.makedirs(parent, exist_ok=True)
    save_png(path, render_points_coincident_residual_to_image(fixed_x, fixed_y, x_min, x_max, y_min, y_max, width, height))


# ---- PNG: 8-bit RGB, non-interlaced ------------------------------------------------------------------------------------
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def save_png(path, rgb: np.ndarray) -> None:
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError("save_png takes an (H, W, 3) uint8 array")
    h, w = rgb.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), np.uint8)  # filter 0 (none) in front of every row
    rows[:, 1:] = rgb.reshape(h, 3 * w)
    data = _PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + \
        _chunk(b"IDAT", zlib.compress(rows.tobytes(), 9)) + _chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(data)


def load_png(path) -> np.ndarray:
    """An 8-bit RGB, non-interlaced PNG file as an (H, W, 3) uint8 array (all five row filters)."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError("not a PNG file")
    at, header, idat = 8, None, []
    while at + 8 <= len(data):
        size, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + size]
        if tag == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        at += 12 + size
    if header is None:
        raise ValueError("PNG without a header")
    w, h, depth, colour, _, _, interlace = header
    if (depth, colour, interlace) != (8, 2, 0):
        raise ValueError("only 8-bit RGB, non-interlaced PNG files are read")
    stride = 3 * w
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    if raw.size != h * (stride + 1):
        raise ValueError("PNG data of the wrong size")
    raw = raw.reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        kind, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        if kind == 0:
            cur = line
        elif kind == 2:  # up
            cur = (line + prev) & 255
        elif kind == 1:  # sub: a running sum per channel
            cur = (np.cumsum(line.reshape(w, 3), axis=0) & 255).reshape(-1)
        elif kind in (3, 4):  # average, Paeth: depend on the pixel to the left as it comes out
            cur = np.zeros(stride, np.int32)
            for i in range(stride):
                left = int(cur[i - 3]) if i >= 3 else 0
                up = int(prev[i])
                if kind == 3:
                    pred = (left + up) >> 1
                else:
                    upleft = int(prev[i - 3]) if i >= 3 else 0
                    p = left + up - upleft
                    pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
                    pred = left if (pa <= pb and pa <= pc) else (up if pb <= pc else upleft)
                cur[i] = (int(line[i]) + pred) & 255
        else:
            raise ValueError("unknown PNG row filter %d" % kind)
        out[y] = cur
        prev = cur
    return out.reshape(h, w, 3)
