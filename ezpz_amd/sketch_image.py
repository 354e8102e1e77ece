"""Sketch images: the reference's `visualize` module (ezpz-cli/src/visualize.rs) on the device, for one sketch and for many.

A drawing list -- points, segments, circles, arcs over variable ids -- is rasterised for every variant of a batch of value
vectors into integer counts per layer and pixel (`ezpz_sketch_image`, a HIP kernel; `ezpz_sketch_image_host`, the same rule
in plain loops without a device), and `compose` turns the counts into colours on the host.  One variant is the picture of a
solved sketch; the steps of a sweep trace a coupler curve; a million samples of a tolerance run give the cloud the geometry
fills inside its tolerance zone (`System.tolerance_mc(..., image=ImageConfig(...))` never brings a value to the host).  Axes,
mesh, caption and labels of the reference's chart are not drawn.  Row 0 of every array is y_min; `save_sketch_png` puts it at
the bottom of the picture.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np

from . import api as _api
from ._lib import (COMPOSE_LAYER_DTYPE, DRAW_ARC, DRAW_CIRCLE, DRAW_FILL, DRAW_ITEM_DTYPE, DRAW_POINT, DRAW_SEGMENT, IMAGE_INFO_DTYPE,
                   CImageView, lib)

ImageView = namedtuple("ImageView", "x_min y_min scale width height")
ImageInfo = namedtuple("ImageInfo", "variants masked items_skipped increments")
SketchImage = namedtuple("SketchImage", "counts info")  # counts [n_layers, height, width] uint32
ComposeLayer = namedtuple("ComposeLayer", "rgb opacity a_min full_at", defaults=(255, 0, 0))
ImageConfig = namedtuple("ImageConfig", "items view n_layers", defaults=(None,))


class DrawItem(namedtuple("DrawItem", "kind layer flags ids half_width")):
    """An EzpzDrawItem: `ids` are variable ids in the caller's numbering, `half_width` is in pixels."""
    __slots__ = ()

    @staticmethod
    def point(x: int, y: int, radius: float, layer: int = 0) -> "DrawItem":
        return DrawItem(DRAW_POINT, layer, 0, (x, y), float(radius))

    @staticmethod
    def segment(ax: int, ay: int, bx: int, by: int, half_width: float, layer: int = 0) -> "DrawItem":
        return DrawItem(DRAW_SEGMENT, layer, 0, (ax, ay, bx, by), float(half_width))

    @staticmethod
    def circle(cx: int, cy: int, r: int, half_width: float, layer: int = 0, fill: bool = False) -> "DrawItem":
        return DrawItem(DRAW_CIRCLE, layer, DRAW_FILL if fill else 0, (cx, cy, r), float(half_width))

    @staticmethod
    def arc(cx: int, cy: int, ax: int, ay: int, bx: int, by: int, half_width: float, layer: int = 0) -> "DrawItem":
        """The minor arc from a to b about c, with the radius |a - c|."""
        return DrawItem(DRAW_ARC, layer, 0, (cx, cy, ax, ay, bx, by), float(half_width))


def _hex(colour: str):
    return tuple(int(colour[i:i + 2], 16) for i in (1, 3, 5))


# the reference's palette (visualize.rs:7-10), one layer per colour and opacity; a count of 1 is already the full colour
LAYER_POINTS, LAYER_DISCS, LAYER_CENTRES, LAYER_ARCS, LAYER_LINES = range(5)
REFERENCE_LAYERS = (
    ComposeLayer(_hex("#58508d"), 255, 0, 1),  # points
    ComposeLayer(_hex("#bc5090"), 77, 0, 1),   # circle discs: the reference's mix(0.3)
    ComposeLayer(_hex("#bc5090"), 255, 0, 1),  # circle centres
    ComposeLayer(_hex("#ff6361"), 255, 0, 1),  # arcs and their three points
    ComposeLayer(_hex("#ffa600"), 255, 0, 1),  # lines
)


def pack_items(items) -> np.ndarray:
    """A list of `DrawItem` (or an array of DRAW_ITEM_DTYPE already) as the library's records."""
    if isinstance(items, np.ndarray) and items.dtype == DRAW_ITEM_DTYPE:
        return np.ascontiguousarray(items)
    out = np.zeros(len(items), dtype=DRAW_ITEM_DTYPE)
    for i, it in enumerate(items):
        it = DrawItem(*it)
        if len(it.ids) > 6:
            raise ValueError("a drawing item has at most six ids")
        out[i]["kind"], out[i]["layer"], out[i]["flags"], out[i]["half_width"] = it.kind, it.layer, it.flags, it.half_width
        out[i]["ids"][:len(it.ids)] = it.ids
    return out


def _view(view) -> CImageView:
    v = ImageView(*view)
    return CImageView(float(v.x_min), float(v.y_min), float(v.scale), int(v.width), int(v.height))


def _layers_of(items: np.ndarray, n_layers: Optional[int]) -> int:
    return int(n_layers) if n_layers is not None else (int(items["layer"].max()) + 1 if len(items) else 1)


def fit_view(x, items, width: int, height: int, padding: float = 1.0) -> ImageView:
    """The reference's `Bounds` (visualize.rs:139-171) as a view: one span min .. max over both axes -- of every point, of the
    circles by their radius, of the arcs by their three points, `padding` added on either side -- mapped onto the shorter side of
    width x height.  x: [n_vars] or [batch, n_vars]; values that are NaN are left out."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    xs, ys = [], []
    for it in pack_items(items):
        ids = it["ids"]
        if it["kind"] == DRAW_CIRCLE:
            for sign in (1.0, -1.0):
                xs.append(x[:, ids[0]] + sign * x[:, ids[2]])
                ys.append(x[:, ids[1]] + sign * x[:, ids[2]])
        else:
            for k in range({DRAW_POINT: 1, DRAW_SEGMENT: 2, DRAW_ARC: 3}[int(it["kind"])]):
                xs.append(x[:, ids[2 * k]])
                ys.append(x[:, ids[2 * k + 1]])

    def span(values):
        both = np.concatenate(values) if values else np.zeros(1)
        both = both[~np.isnan(both)]
        return (float(both.min()), float(both.max())) if both.size else (0.0, 0.0)

    (min_x, max_x), (min_y, max_y) = span(xs), span(ys)
    lo, hi = min(min_x - padding, min_y - padding), max(max_x + padding, max_y + padding)
    if not hi > lo:
        raise ValueError("fit_view: an empty span (no padding and a single point)")
    return ImageView(lo, lo, min(int(width), int(height)) / (hi - lo), int(width), int(height))


def _request(x, items, view, n_layers, ok, accumulate):
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2:
        raise ValueError("x: [n_vars] or [batch, n_vars]")
    recs = pack_items(items)
    vw = _view(view)
    if accumulate is not None:
        counts = np.ascontiguousarray(accumulate.counts, dtype=np.uint32).copy()
        if counts.ndim != 3 or counts.shape[1:] != (vw.height, vw.width) or (n_layers is not None and counts.shape[0] != n_layers):
            raise ValueError("accumulate: counts of another shape")
        layers = counts.shape[0]
        info = np.array([tuple(accumulate.info)], dtype=IMAGE_INFO_DTYPE)
    else:
        layers = _layers_of(recs, n_layers)
        if not (1 <= vw.width <= 16384 and 1 <= vw.height <= 16384 and 1 <= layers <= 8):
            raise _api.NonLinearSystemError(-103)
        counts = np.zeros((layers, vw.height, vw.width), np.uint32)
        info = np.zeros(1, dtype=IMAGE_INFO_DTYPE)
    if ok is not None:
        ok = np.ascontiguousarray(ok, dtype=np.uint8).reshape(-1)
        if ok.size != x.shape[0]:
            raise ValueError("ok: one byte per variant")
    return x, recs, vw, layers, ok, counts, info


def _draw(entry, x, items, view, n_layers, ok, accumulate) -> SketchImage:
    x, recs, vw, layers, ok, counts, info = _request(x, items, view, n_layers, ok, accumulate)
    rc = entry(_api._ptr(x), _api._ptr(ok), x.shape[0], x.shape[1], _api._ptr(recs), len(recs), C.byref(vw), layers,
               int(accumulate is not None), counts.ctypes.data, info.ctypes.data)
    if rc != 0:
        raise _api.NonLinearSystemError(rc)
    return SketchImage(counts, ImageInfo(*(int(v) for v in info[0])))


def sketch_image(x, items, view, n_layers: Optional[int] = None, ok=None, accumulate: Optional[SketchImage] = None) -> SketchImage:
    """`ezpz_sketch_image`: every variant x[b] of the drawing list rasterised on the device.  Returns SketchImage(counts
    [n_layers, height, width] uint32, info); n_layers None: one more than the largest layer used; ok [batch]: a variant whose
    byte is 0 draws nothing; accumulate: an earlier result this call adds to (it is not modified)."""
    return _draw(lib().ezpz_sketch_image, x, items, view, n_layers, ok, accumulate)


def sketch_image_host(x, items, view, n_layers: Optional[int] = None, ok=None, accumulate: Optional[SketchImage] = None) -> SketchImage:
    """`ezpz_sketch_image_host`: the same rule in plain loops over every pixel, on the host; it needs no device."""
    return _draw(lib().ezpz_sketch_image_host, x, items, view, n_layers, ok, accumulate)


def sketch_image_device(x_ptr: int, ok_ptr: int, batch: int, n_vars: int, items, view, n_layers: int, counts_ptr: int, info_ptr: int,
                        accumulate: bool = False, stream: int = 0) -> None:
    """`ezpz_sketch_image_device`: device pointers for x [batch, n_vars], ok [batch] (0: none), counts (uint32 [n_layers, height,
    width]) and info (IMAGE_INFO_DTYPE [1]) and a hipStream_t handle; items and view stay host values.  Enqueues only once the
    item list is the last call's."""
    recs = pack_items(items)
    vw = _view(view)
    rc = lib().ezpz_sketch_image_device(x_ptr or None, ok_ptr or None, int(batch), int(n_vars), _api._ptr(recs), len(recs), C.byref(vw),
                                        int(n_layers), int(bool(accumulate)), counts_ptr or None, info_ptr or None, stream or None)
    if rc != 0:
        raise _api.NonLinearSystemError(rc)


def pack_layers(layers) -> np.ndarray:
    out = np.zeros(len(layers), dtype=COMPOSE_LAYER_DTYPE)
    for i, layer in enumerate(layers):
        layer = ComposeLayer(*layer)
        out[i]["rgb"], out[i]["opacity"], out[i]["a_min"], out[i]["full_at"] = layer.rgb, layer.opacity, layer.a_min, layer.full_at
    return out


def compose(counts, layers: Sequence[ComposeLayer] = REFERENCE_LAYERS, background=(255, 255, 255)) -> np.ndarray:
    """`ezpz_sketch_compose`: counts [n_layers, height, width] to an (height, width, 3) uint8 image, the layers in order over
    `background`; a layer is ComposeLayer(rgb, opacity, a_min, full_at) -- full_at 0: the layer's largest count.  Integers only;
    host only.  `layers` may be longer than the counts have layers."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if counts.ndim != 3:
        raise ValueError("counts: [n_layers, height, width]")
    if len(layers) < counts.shape[0]:
        raise ValueError("compose: a ComposeLayer per layer of the counts")
    recs = pack_layers(list(layers)[:counts.shape[0]])
    vw = CImageView(0.0, 0.0, 1.0, counts.shape[2], counts.shape[1])
    rgb = np.empty((counts.shape[1], counts.shape[2], 3), np.uint8)
    bg = np.array(background, dtype=np.uint8)
    rc = lib().ezpz_sketch_compose(counts.ctypes.data, C.byref(vw), counts.shape[0], _api._ptr(recs), bg.ctypes.data, rgb.ctypes.data)
    if rc != 0:
        raise _api.NonLinearSystemError(rc)
    return rgb


def items_from_problem(problem, point_radius: float = 10.0, stroke: float = 3.0):
    """The drawing list of a `textual.Problem` in the reference's order (visualize.rs:44-62, :76-107): the points, the circles'
    centres, the arcs' a, b and centres as discs of `point_radius`; the circles as filled discs; the arcs and the `line`
    instructions as strokes `stroke` pixels wide.  The variable ids are those of the solution's value vector."""
    cs = problem.to_constraint_system() if hasattr(problem, "to_constraint_system") else problem
    n_p, n_c, n_a = len(cs.inner_points), len(cs.inner_circles), len(cs.inner_arcs)
    circle = lambda i: 2 * n_p + 3 * i
    arc = lambda i: 2 * n_p + 3 * n_c + 6 * i  # a (s, s + 1), b (s + 2, s + 3), centre (s + 4, s + 5)
    items = [DrawItem.point(2 * i, 2 * i + 1, point_radius, LAYER_POINTS) for i in range(n_p)]
    items += [DrawItem.point(circle(i), circle(i) + 1, point_radius, LAYER_CENTRES) for i in range(n_c)]
    for offset in (0, 2, 4):
        items += [DrawItem.point(arc(i) + offset, arc(i) + offset + 1, point_radius, LAYER_ARCS) for i in range(n_a)]
    items += [DrawItem.circle(circle(i), circle(i) + 1, circle(i) + 2, 0.0, LAYER_DISCS, fill=True) for i in range(n_c)]
    items += [DrawItem.arc(arc(i) + 4, arc(i) + 5, arc(i), arc(i) + 1, arc(i) + 2, arc(i) + 3, stroke / 2.0, LAYER_ARCS) for i in range(n_a)]
    items += [DrawItem.segment(2 * a, 2 * a + 1, 2 * b, 2 * b + 1, stroke / 2.0, LAYER_LINES) for a, b in cs.inner_lines]
    return items


def save_sketch_png(path, x, items, view, layers: Sequence[ComposeLayer] = REFERENCE_LAYERS, background=(255, 255, 255)) -> None:
    """The picture of x (one variant or many) as a PNG file: `sketch_image`, `compose`, row 0 at the bottom."""
    from . import residual_viz

    image = sketch_image(x, items, view, n_layers=len(layers))
    residual_viz.save_png(path, compose(image.counts, layers, background)[::-1])
