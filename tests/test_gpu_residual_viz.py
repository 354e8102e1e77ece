"""Residual-field rendering on the device (ezpz_system_residual_field*, ezpz_amd.residual_viz) against the reference's five
baseline images -- every pixel, zero tolerance: in those scenes no magnitude is closer than 2.7e-7 to a place where the
colour changes, and device residuals are held to 1e-11 -- and against the oracle's residuals per pixel."""
import ctypes as C
import os

import numpy as np
import pytest

from gen import connected_sketch
from residual_viz_common import (BAR, BASELINES, KIND_VIEW, SCENES, VIEWPORT, kind_scene, moves_under_one_ulp, oracle_field,
                                 pixel_centres)

import ezpz_amd as E
from ezpz_amd import residual_viz as V
from ezpz_amd._lib import CViewport
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RENDER = {
    "points_coincident": lambda: V.render_points_coincident_residual_to_image(0.0, 0.0, -5.0, 5.0, -5.0, 5.0, 256, 256),
    "distance": lambda: V.render_distance_residual_to_image(0.0, 0.0, 3.0, -5.0, 5.0, -5.0, 5.0, 256, 256),
    "point_line_distance": lambda: V.render_point_line_distance_residual_to_image(-4.0, -2.0, 4.0, 2.0, 2.0, -5.0, 5.0, -5.0, 5.0, 256, 256),
    "vertical": lambda: V.render_vertical_residual_to_image(0.0, 0.0, -5.0, 5.0, -5.0, 5.0, 256, 256),
    "horizontal": lambda: V.render_horizontal_residual_to_image(0.0, 0.0, -5.0, 5.0, -5.0, 5.0, 256, 256),
}


def eval_residuals(system, values):
    """System.eval_batch without its dense Jacobian: (r [batch, rows], degenerate counts)."""
    info = system.info()
    values = np.ascontiguousarray(values, dtype=np.float64)
    batch = values.shape[0]
    r = np.zeros((batch, info["n_rows"]))
    jv = np.zeros((batch, max(info["nnz_j"], 1)))
    deg = np.zeros(batch, np.uint32)
    assert E.lib().ezpz_system_eval_batch(system._h, values.ctypes.data, batch, r.ctypes.data, jv.ctypes.data, deg.ctypes.data) == 0
    return r, deg


def within_bar(got, want):
    return np.abs(got - want) <= BAR * np.maximum(1.0, np.abs(want))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_render_equals_the_reference_image(name):
    """The reference test's arguments (residual_viz.rs:536-580): all 65 536 pixels of its baseline."""
    got = RENDER[name]()
    want = V.load_png(os.path.join(BASELINES, name + ".png"))
    assert got.shape == want.shape == (256, 256, 3) and got.dtype == np.uint8
    differing = int(np.any(got != want, axis=2).sum())
    print(name, "differing pixels", differing)
    assert differing == 0, differing


@pytest.mark.parametrize("name", sorted(SCENES))
def test_magnitude_equals_the_oracle(name):
    """Bitwise for Vertical / Horizontal (a subtraction and fabs), 1e-11 * max(1, |want|) for the others."""
    rec, x_base, _, _ = SCENES[name]
    want, want_deg = oracle_field(rec, x_base, 0, 1, VIEWPORT)
    f = V.residual_field([rec], x_base, 0, 1, VIEWPORT, constraint=0)
    print(name, "max abs difference", float(np.max(np.abs(f.mag - want))), "degenerate", f.degenerate_pixels, int(want_deg.sum()))
    if name in ("vertical", "horizontal"):
        assert np.array_equal(f.mag, want)
    else:
        assert within_bar(f.mag, want).all()
    assert f.degenerate_pixels == int(want_deg.sum())
    assert np.array_equal(f.rgb, V.colormap(f.mag))
    # the one constraint of the system, selected or as "all": the same field (C = 0.0)
    g = V.residual_field([rec], x_base, 0, 1, VIEWPORT)
    assert within_bar(g.mag, want).all() and g.degenerate_pixels == f.degenerate_pixels


def test_every_kind_against_the_oracle():
    """All 25 kinds, one constraint selected, 64x48 pixels around two of its own variables.  A pixel may be left out only where
    the oracle's own value moves by more than the bar under one ulp of a swept coordinate, at most 0.1 % of a scene."""
    w, h = KIND_VIEW
    for kind in range(25):
        rec, x_base, vx, vy, viewport = kind_scene(kind)
        want, want_deg = oracle_field(rec, x_base, vx, vy, viewport)
        f = V.residual_field([rec], x_base, vx, vy, viewport, constraint=0)
        xs, ys = pixel_centres(viewport)
        off = np.argwhere(~within_bar(f.mag, want))
        left_out = 0
        for r, c in off:
            assert moves_under_one_ulp(rec, x_base, vx, vy, xs[c], ys[r], want[r, c]), (kind, int(r), int(c), f.mag[r, c], want[r, c])
            left_out += 1
        print("kind %2d %-28s left out %d, degenerate %d / %d, max abs difference %.3g" % (
            kind, E.api.KIND_NAMES[kind], left_out, f.degenerate_pixels, int(want_deg.sum()),
            float(np.max(np.abs(f.mag - want)))))
        assert left_out <= (w * h) // 1000, (kind, left_out)
        assert f.degenerate_pixels == int(want_deg.sum()), kind
        assert np.array_equal(f.rgb, V.colormap(f.mag))


def test_guard_leaves_zero_and_counts_the_pixel():
    """Distance from a point to a line of no length (PointLineDistance's guard, constraints.rs:712-740): every pixel degenerate."""
    rec = O.point_line_distance((0, 1), (2, 3), (4, 5), 2.0)
    x_base = [0.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    f = V.residual_field([rec], x_base, 0, 1, (-1.0, 1.0, -1.0, 1.0, 8, 4), constraint=0)
    assert f.degenerate_pixels == 32 and np.array_equal(f.mag, np.zeros((4, 8)))


def test_whole_sketch_against_eval_batch():
    """All constraints of a connected sketch (240 variables, weights 1) with one point swept: sqrt of the summed squares of
    System.eval_batch's residuals at the same values; then the part no pixel changes alone (C), by sweeping two variables
    that no constraint other than one Fixed uses."""
    recs, guess = connected_sketch(120, 11)
    n = len(guess)
    assert (recs["weight"] == 1.0).all()
    system = E.System(recs, n)
    k = 57
    vx, vy = 2 * k, 2 * k + 1
    viewport = (float(guess[vx] - 1.0), float(guess[vx] + 1.0), float(guess[vy] - 0.75), float(guess[vy] + 0.75), 64, 48)
    xs, ys = pixel_centres(viewport)
    values = np.tile(guess, (48 * 64, 1))
    values[:, vx] = np.tile(xs, 48)
    values[:, vy] = np.repeat(ys, 64)
    r, deg = eval_residuals(system, values)
    want = np.sqrt((r * r).sum(axis=1)).reshape(48, 64)
    f = system.residual_field(guess, vx, vy, viewport)
    print("sketch: max relative difference", float(np.max(np.abs(f.mag - want) / np.maximum(1.0, want))))
    assert within_bar(f.mag, want).all()
    assert np.array_equal(f.rgb, V.colormap(f.mag)) and f.degenerate_pixels == 0 and not deg.any()
    # each listed constraint alone, and a constraint that no swept variable touches (a constant field)
    touching = [i for i in range(len(recs)) if vx in recs["ids"][i][:O.KIND_NUM_IDS[int(recs["kind"][i])]]
                or vy in recs["ids"][i][:O.KIND_NUM_IDS[int(recs["kind"][i])]]]
    assert len(touching) >= 2
    s = np.zeros((48, 64))
    for i in touching:
        m = system.residual_field(guess, vx, vy, viewport, constraint=i, want=("mag",)).mag
        s += m * m
    far = next(i for i in range(len(recs)) if i not in touching)
    const = system.residual_field(guess, vx, vy, viewport, constraint=far, want=("mag",)).mag
    assert (const == const[0, 0]).all()
    rest = np.array([guess])
    r0, _ = eval_residuals(system, rest)
    rows_of = np.cumsum([0] + [O.residual_dim(c) for c in recs])
    c_want = sum(float(r0[0, j]) ** 2 for i in range(len(recs)) if i not in touching for j in range(rows_of[i], rows_of[i + 1]))
    assert within_bar(f.mag, np.sqrt(c_want + s)).all()
    # C alone: two more variables, one of them held by a Fixed, the other used by nothing
    a, b = n, n + 1
    recs2 = O.stack(list(recs) + [O.fixed(a, 0.25)])
    base2 = np.concatenate([guess, [0.0, 0.0]])
    system2 = E.System(recs2, n + 2)
    viewport2 = (-1.0, 1.0, -1.0, 1.0, 64, 48)
    xs2, ys2 = pixel_centres(viewport2)
    values2 = np.tile(base2, (48 * 64, 1))
    values2[:, a] = np.tile(xs2, 48)
    values2[:, b] = np.repeat(ys2, 64)
    r2, _ = eval_residuals(system2, values2)
    want2 = np.sqrt((r2 * r2).sum(axis=1)).reshape(48, 64)
    f2 = system2.residual_field(base2, a, b, viewport2, want=("mag",))
    assert f2.rgb is None and within_bar(f2.mag, want2).all()
    assert (f2.mag == f2.mag[0:1, :]).all()  # (b changes nothing)


def test_shapes_outputs_and_the_device_entry():
    """Widths 1, 3, 5, 1023 and height 1 (the pixel-by-pixel stores), a multiple of 4 (the vector stores); rgb only, mag only;
    the device entry on a stream of its own with torch tensors: the host entry's bits."""
    import torch

    rec_v = O.vertical((0, 1), (2, 3))
    rec_d = O.distance((0, 1), (2, 3), 1.5)
    x_base = np.array([0.0, 0.0, 0.25, -0.5])
    system = E.System(O.stack([rec_v, rec_d]), 4)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    xb = torch.tensor(x_base, dtype=torch.float64, device=dev)
    for w, h in ((1, 1), (3, 2), (5, 3), (1023, 2), (64, 1), (7, 1), (128, 5)):
        viewport = (-2.0, 2.0, -1.0, 3.0, w, h)
        xs, ys = pixel_centres(viewport)
        f = system.residual_field(x_base, 0, 1, viewport, constraint=0)
        assert f.mag.shape == (h, w) and f.rgb.shape == (h, w, 3)
        assert np.array_equal(f.mag, np.tile(np.abs(xs - 0.25), (h, 1)))  # Vertical: bitwise
        assert np.array_equal(f.rgb, V.colormap(f.mag))
        both = system.residual_field(x_base, 0, 1, viewport)
        want = np.sqrt(f.mag ** 2 + (np.hypot(xs[None, :] - 0.25, ys[:, None] + 0.5) - 1.5) ** 2)
        assert within_bar(both.mag, want).all()
        only_rgb = system.residual_field(x_base, 0, 1, viewport, want=("rgb",))
        only_mag = system.residual_field(x_base, 0, 1, viewport, want=("mag",))
        assert only_rgb.mag is None and only_mag.rgb is None
        assert np.array_equal(only_rgb.rgb, both.rgb) and np.array_equal(only_mag.mag, both.mag)
        # device entry
        mag_t = torch.full((h, w), -1.0, dtype=torch.float64, device=dev)
        rgb_t = torch.full((h, w, 3), 7, dtype=torch.uint8, device=dev)
        deg_t = torch.full((1,), 99, dtype=torch.int64, device=dev)
        vp = CViewport(*[float(v) for v in viewport[:4]], w, h)
        with torch.cuda.stream(stream):
            rc = E.lib().ezpz_system_residual_field_device(system._h, xb.data_ptr(), 0, 1, -1, C.byref(vp), mag_t.data_ptr(),
                                                           rgb_t.data_ptr(), deg_t.data_ptr(), stream.cuda_stream)
        assert rc == 0
        stream.synchronize()
        assert np.array_equal(mag_t.cpu().numpy(), both.mag) and np.array_equal(rgb_t.cpu().numpy(), both.rgb)
        assert int(deg_t.item()) == both.degenerate_pixels == 0
    # outputs the caller did not align: the same values through the pixel-by-pixel stores
    w, h = 64, 3
    viewport = (-2.0, 2.0, -1.0, 3.0, w, h)
    both = system.residual_field(x_base, 0, 1, viewport)
    mag_t = torch.zeros(h * w + 1, dtype=torch.float64, device=dev)
    rgb_t = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device=dev)
    vp = CViewport(-2.0, 2.0, -1.0, 3.0, w, h)
    rc = E.lib().ezpz_system_residual_field_device(system._h, xb.data_ptr(), 0, 1, -1, C.byref(vp), mag_t.data_ptr() + 8,
                                                   rgb_t.data_ptr() + 1, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(mag_t.cpu().numpy()[1:].reshape(h, w), both.mag) and mag_t[0].item() == 0.0
    assert np.array_equal(rgb_t.cpu().numpy()[1:].reshape(h, w, 3), both.rgb) and rgb_t[0].item() == 0


def test_argument_errors():
    rec = O.distance((0, 1), (2, 3), 1.0)
    system = E.System(O.stack([rec]), 4)
    L = E.lib()
    x = np.zeros(4)
    mag = np.zeros(16)
    rgb = np.zeros(48, np.uint8)

    def call(var_x=0, var_y=1, constraint=0, width=4, height=4, mag_p=mag.ctypes.data, rgb_p=rgb.ctypes.data, vp_null=False):
        vp = CViewport(-1.0, 1.0, -1.0, 1.0, width, height)
        return L.ezpz_system_residual_field(system._h, x.ctypes.data, var_x, var_y, constraint, None if vp_null else C.byref(vp),
                                            mag_p, rgb_p, None)

    assert call() == 0
    assert call(constraint=-1) == 0
    assert call(vp_null=True) == -103
    assert call(width=0) == -103 and call(height=0) == -103
    assert call(var_x=1, var_y=1) == -103
    assert call(var_x=4) == -103 and call(var_y=4) == -103
    assert call(constraint=1) == -103 and call(constraint=-2) == -103
    assert call(mag_p=None, rgb_p=None) == -103
    assert call(mag_p=None) == 0 and call(rgb_p=None) == 0
    vp = CViewport(-1.0, 1.0, -1.0, 1.0, 4, 4)
    assert L.ezpz_system_residual_field_device(system._h, None, 0, 1, 0, C.byref(vp), None, None, None, None) == -103
    assert L.ezpz_system_residual_field_device(system._h, 8, 0, 0, 0, C.byref(vp), 8, None, None, None) == -103
    with pytest.raises(E.NonLinearSystemError):
        system.residual_field(x, 0, 0, (-1.0, 1.0, -1.0, 1.0, 4, 4))


def test_overlay_of_a_general_system_and_the_png_entry(tmp_path):
    """overlay=(example): the green point is where an ordinary solve from the example lands -- for the Distance scene the
    reference's closed form, so the picture is the baseline again; and the reference's file entry point."""
    rec, x_base, example, _ = SCENES["distance"]
    f = V.residual_field([rec, O.fixed(2, 0.0), O.fixed(3, 0.0)], x_base, 0, 1, VIEWPORT, constraint=0, overlay=example)
    want = V.load_png(os.path.join(BASELINES, "distance.png"))
    assert int(np.any(f.rgb != want, axis=2).sum()) == 0
    path = tmp_path / "sub" / "points_coincident.png"
    V.render_points_coincident_residual(path, 0.0, 0.0, -5.0, 5.0, -5.0, 5.0, 256, 256)
    assert np.array_equal(V.load_png(path), V.load_png(os.path.join(BASELINES, "points_coincident.png")))
