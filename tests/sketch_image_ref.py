"""The sketch-image rule and the compositor as explicit numpy: the yardstick of tests/test_sketch_image_cpu.py and
tests/test_gpu_sketch_image.py.  Written from the statement of the rule (include/ezpz_amd.h), not from the C body: every
operation is one numpy float64 operation, in the order the rule writes it, over all pixels of the view at once -- and, for a batch,
over a block of variants at once, which changes no operation.

    counts, info = image(x, ok, items, view, n_layers)
    rgb = compose(counts, layers, background)

items: tuples (kind, layer, flags, ids, half_width); view: (x_min, y_min, scale, width, height); info: (variants, masked,
items_skipped, increments)."""
import numpy as np

POINT, SEGMENT, CIRCLE, ARC = 0, 1, 2, 3
FILL = 1
LIMIT = 2.0 ** 30


def _ring(d2, R2, h):
    q = (d2 + R2) - h * h
    return (q <= 0.0) | (q * q <= (4.0 * d2) * R2)


def covered(kind, flags, p, h, X, Y):
    """p: the item's pixel-space numbers, each an array that broadcasts against X and Y (the pixel centres)."""
    h = np.float64(h)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == POINT:
            u, v = p
            dx = X - u
            dy = Y - v
            d2 = dx * dx + dy * dy
            return d2 <= h * h
        if kind == SEGMENT:
            au, av, bu, bv = p
            ex = bu - au
            ey = bv - av
            L2 = ex * ex + ey * ey
            wx = X - au
            wy = Y - av
            t = wx * ex + wy * ey
            near_a = (L2 == 0.0) | (t <= 0.0)
            zx = X - bu
            zy = Y - bv
            cr = wx * ey - wy * ex
            return np.where(near_a, wx * wx + wy * wy <= h * h, np.where(t >= L2, zx * zx + zy * zy <= h * h, cr * cr <= (h * h) * L2))
        if kind == CIRCLE:
            u, v, R = p
            wx = X - u
            wy = Y - v
            d2 = wx * wx + wy * wy
            R2 = R * R
            if flags & FILL:
                hi = R + h
                return d2 <= hi * hi
            return _ring(d2, R2, h)
        cu, cv, au, av, bu, bv = p
        px = au - cu
        py = av - cv
        qx = bu - cu
        qy = bv - cv
        R2 = px * px + py * py
        wx = X - cu
        wy = Y - cv
        d2 = wx * wx + wy * wy
        ring = _ring(d2, R2, h)
        s = px * qy - py * qx
        c1 = px * wy - py * wx
        c2 = wx * qy - wy * qx
        sector = np.where(s > 0.0, (c1 >= 0.0) & (c2 >= 0.0),
                          np.where(s < 0.0, (c1 <= 0.0) & (c2 <= 0.0), np.where(px * qx + py * qy > 0.0, False, c1 >= 0.0)))
        return ring & sector


def image(x, ok, items, view, n_layers, block=128):
    x_min, y_min, scale, width, height = view
    x = np.asarray(x, dtype=np.float64).reshape(-1, np.asarray(x).shape[-1])
    batch = x.shape[0]
    alive = np.ones(batch, bool) if ok is None else np.asarray(ok).reshape(-1) != 0
    counts = np.zeros((n_layers, height, width), np.uint64)
    X = (np.arange(width, dtype=np.float64) + 0.5)[None, None, :]
    Y = (np.arange(height, dtype=np.float64) + 0.5)[None, :, None]
    skipped = 0
    xs = x[alive]
    for kind, layer, flags, ids, h in items:
        pairs = {POINT: 1, SEGMENT: 2, CIRCLE: 1, ARC: 3}[kind]
        with np.errstate(over="ignore", invalid="ignore"):
            p = []
            for k in range(pairs):
                p.append((xs[:, ids[2 * k]] - x_min) * scale)
                p.append((xs[:, ids[2 * k + 1]] - y_min) * scale)
            if kind == CIRCLE:
                p.append(np.fabs(xs[:, ids[2]]) * scale)
            good = np.ones(len(xs), bool)
            for v in p:
                good &= np.isfinite(v) & (np.fabs(v) <= LIMIT)
        skipped += int((~good).sum())
        p = [v[good] for v in p]
        for at in range(0, int(good.sum()), block):
            part = [v[at:at + block, None, None] for v in p]
            counts[layer] += covered(kind, flags, part, h, X, Y).sum(axis=0, dtype=np.uint64)
    info = (batch, int((~alive).sum()), skipped, int(counts.sum()))
    return (counts & 0xFFFFFFFF).astype(np.uint32), info


def compose(counts, layers, background=(255, 255, 255)):
    """layers: tuples (rgb, opacity, a_min, full_at), one per layer of the counts.  Python integers per pixel, vectorised as int64."""
    counts = np.asarray(counts).astype(np.int64)
    out = np.empty(counts.shape[1:] + (3,), np.int64)
    out[...] = np.asarray(background, dtype=np.int64)
    for cnt, (rgb, opacity, a_min, full_at) in zip(counts, layers):
        F = int(full_at) if full_at else int(cnt.max())
        F = F if F else 1
        a = np.where(cnt == 0, 0, np.maximum(a_min, np.minimum(cnt, F) * 255 // F))
        a = a * opacity // 255
        for c in range(3):
            out[..., c] = (out[..., c] * (255 - a) + rgb[c] * a + 127) // 255
    return out.astype(np.uint8)
