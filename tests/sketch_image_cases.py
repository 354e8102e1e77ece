"""The case list of the sketch-image tests (tests/test_sketch_image_cpu.py: host body against numpy; tests/test_gpu_sketch_image.py:
device against both): name -> (x [batch, n_vars], ok or None, items, view, n_layers).  Every case is drawn on a 200 x 136 view: no
multiple of the kernel's 64-pixel tile, so tile edges lie inside the image.  items: (kind, layer, flags, ids, half_width)."""
import numpy as np

POINT, SEGMENT, CIRCLE, ARC = 0, 1, 2, 3
FILL = 1
W, H = 200, 136
UNIT = (0.0, 0.0, 1.0, W, H)      # pixel space is value space: the ties below are exact
WORLD = (-2.0, -1.5, 7.3, W, H)   # a scale that rounds


class Values:
    """Collects values and hands out their ids."""

    def __init__(self):
        self.v = []

    def __call__(self, *values):
        first = len(self.v)
        self.v += [float(a) for a in values]
        return tuple(range(first, len(self.v)))

    def x(self):
        return np.array([self.v])


def _kinds():
    """Every kind alone: inside, across the tile boundaries at 64 and 128, partly and wholly outside the view, larger than it."""
    out = {}
    v = Values()
    out["point"] = (v, [(POINT, 0, 0, v(3.1, 2.2), 6.5), (POINT, 0, 0, v(6.77, 7.2), 9.0),  # the second lies over the corner of four tiles
                        (POINT, 0, 0, v(-2.5, 5.0), 7.0), (POINT, 0, 0, v(26.0, 17.5), 12.0), (POINT, 0, 0, v(60.0, 5.0), 20.0),
                        (POINT, 0, 0, v(12.0, 9.0), 400.0)], WORLD)
    v = Values()
    out["segment"] = (v, [(SEGMENT, 0, 0, v(4.0, 1.0, 9.0, 8.5), 1.5), (SEGMENT, 0, 0, v(-5.0, 3.0, 4.0, 4.0), 2.5),
                          (SEGMENT, 0, 0, v(-30.0, -20.0, 60.0, 40.0), 1.0), (SEGMENT, 0, 0, v(40.0, 0.0, 50.0, 30.0), 3.0),
                          (SEGMENT, 0, 0, v(20.0, 2.0, 20.0, 16.0), 0.75)], WORLD)
    v = Values()
    out["circle"] = (v, [(CIRCLE, 0, 0, v(6.77, 7.27, 4.0), 1.5), (CIRCLE, 0, FILL, v(17.0, 5.0, 2.5), 0.0), (CIRCLE, 0, FILL, v(24.0, 16.0, 3.0), 2.0),
                         (CIRCLE, 0, 0, v(10.0, -30.0, 40.0), 2.0), (CIRCLE, 0, 0, v(11.0, 8.0, 60.0), 3.0), (CIRCLE, 0, 0, v(-40.0, 8.0, 5.0), 3.0),
                         (CIRCLE, 0, 0, v(3.0, 12.0, -2.0), 1.0)], WORLD)
    v = Values()
    out["arc"] = (v, [(ARC, 0, 0, v(6.77, 7.27, 10.77, 7.27, 6.77, 11.27), 1.5), (ARC, 0, 0, v(17.0, 5.0, 17.0, 8.0, 14.5, 3.0), 2.0),
                      (ARC, 0, 0, v(10.0, -30.0, 10.0, 10.0, 30.0, 4.6), 2.0), (ARC, 0, 0, v(22.0, 12.0, 26.0, 12.0, 22.5, 15.9), 1.0),
                      (ARC, 0, 0, v(-50.0, -50.0, -45.0, -50.0, -50.0, -45.0), 2.0)], WORLD)
    return out


def cases():
    out = {}
    kinds = _kinds()
    for name, (v, items, view) in kinds.items():
        out[name] = (v.x(), None, items, view, 1)
    # all together: every list on a layer of its own, the ids shifted behind one another
    x, items = [], []
    for layer, (name, (v, its, view)) in enumerate(kinds.items()):
        items += [(k, layer, f, tuple(i + len(x) for i in ids), h) for k, _, f, ids, h in its]
        x += v.v
    out["all"] = (np.array([x]), None, items, WORLD, 4)

    # ties: <= written as < loses pixels here
    v = Values()
    items = ([(POINT, 0, 0, v(10.5, 10.5), 3.0), (POINT, 0, 0, v(63.5, 64.5), 5.0),
                       (SEGMENT, 1, 0, v(5.0, 20.0, 30.0, 20.0), 1.5), (SEGMENT, 1, 0, v(40.0, 30.0, 40.0, 70.0), 1.5),
                       (SEGMENT, 1, 0, v(5.5, 90.5, 30.5, 90.5), 2.0), (SEGMENT, 1, 0, v(100.5, 5.5, 100.5, 5.5), 4.0),
                       (CIRCLE, 2, 0, v(50.5, 50.5, 10.0), 2.0), (CIRCLE, 2, FILL, v(120.5, 60.5, 5.0), 0.0), (CIRCLE, 2, FILL, v(150.5, 60.5, 3.0), 2.0),
                       (ARC, 3, 0, v(150.5, 100.5, 160.5, 100.5, 150.5, 110.5), 2.0)])
    out["ties"] = (v.x(), None, items, UNIT, 4)

    # degenerate items
    v = Values()
    items = [(SEGMENT, 0, 0, v(20.5, 20.5, 20.5, 20.5), 3.0),                      # zero length: a disc
             (CIRCLE, 0, 0, v(50.5, 20.5, 0.0), 2.0), (CIRCLE, 0, FILL, v(70.5, 20.5, 0.0), 2.0),  # r = 0
             (CIRCLE, 1, 0, v(100.5, 30.5, -12.0), 1.5), (CIRCLE, 1, FILL, v(140.5, 30.5, -6.0), 0.0),  # r < 0
             (ARC, 2, 0, v(30.5, 70.5, 40.5, 70.5, 40.5, 70.5), 1.5),                # a == b: nothing
             (ARC, 2, 0, v(30.5, 70.5, 36.5, 78.5, 42.5, 86.5), 1.5),                # b beyond a on one ray: nothing
             (ARC, 2, 0, v(70.5, 70.5, 82.5, 70.5, 58.5, 70.5), 1.5),                # a opposite b: the half-turn from a
             (ARC, 2, 0, v(110.5, 70.5, 110.5, 58.5, 110.5, 82.5), 1.5),             # ... along the other axis
             (ARC, 2, 0, v(150.5, 70.5, 150.5, 70.5, 160.5, 70.5), 2.5),             # a == c: radius 0
             (POINT, 3, 0, v(20.5, 110.5), 0.0), (POINT, 3, 0, v(30.0, 110.5), 0.0),  # half_width 0: on a centre, between two
             (SEGMENT, 3, 0, v(40.5, 110.5, 60.5, 110.5), 0.0), (SEGMENT, 3, 0, v(70.5, 100.5, 90.5, 120.5), 0.0),
             (CIRCLE, 3, 0, v(120.5, 110.5, 5.0), 0.0), (ARC, 3, 0, v(150.5, 110.5, 155.5, 110.5, 150.5, 115.5), 0.0),
             (POINT, 0, 0, v(180.0, 100.0), 1e300)]                                  # a reach that overflows its square
    out["degenerate"] = (v.x(), None, items, UNIT, 4)

    # values that cannot be drawn: the items that read them are skipped and counted, the others are drawn
    v = Values()
    items = [(POINT, 0, 0, v(3.0, 2.0), 5.0), (SEGMENT, 0, 0, v(4.0, 4.0, 12.0, 9.0), 1.5), (CIRCLE, 0, 0, v(15.0, 8.0, 3.0), 1.5),
             (ARC, 0, 0, v(8.0, 12.0, 11.0, 12.0, 8.0, 15.0), 1.5), (CIRCLE, 0, FILL, v(20.0, 4.0, 1.0), 1.0)]
    x = np.repeat(v.x(), 9, axis=0)
    scale = WORLD[2]
    x[1, 0] = np.nan            # the point's u
    x[2, 3] = np.inf            # the segment's av
    x[3, 4] = -np.inf           # its bu
    x[4, 8] = 3e9 / scale       # the circle's R: above 2^30 pixels
    x[5, 8] = -3e9 / scale      # ... by its magnitude
    x[6, 11] = 3e9 / scale      # the arc's au
    x[7, 7] = -3e9 / scale      # the circle's v
    x[8, :] = np.nan            # every item of a variant
    out["not_drawable"] = (x, None, items, WORLD, 1)

    # ok with zeros: a masked variant draws nothing and its values are not looked at
    ok = np.array([1, 0, 1, 0, 0, 1, 1, 0, 255], np.uint8)
    out["masked"] = (x, ok, items, WORLD, 1)
    return out


def layered():
    """n_layers = 5 and one list in two orders: the same counts."""
    v = Values()
    items = [(POINT, 4, 0, v(3.0, 2.0), 5.0), (SEGMENT, 2, 0, v(4.0, 4.0, 12.0, 9.0), 1.5), (CIRCLE, 0, 0, v(15.0, 8.0, 3.0), 1.5),
             (ARC, 3, 0, v(8.0, 12.0, 11.0, 12.0, 8.0, 15.0), 1.5), (CIRCLE, 4, FILL, v(4.0, 3.0, 1.0), 1.0), (POINT, 2, 0, v(8.0, 6.5), 4.0)]
    return v.x(), items, [items[i] for i in (3, 5, 0, 4, 2, 1)], WORLD, 5


def cloud(batch=4099, seed=11):
    """`batch` jittered variants of a 10-item list, all landing on the same few thousand pixels."""
    v = Values()
    items = [(POINT, 0, 0, v(3.0, 2.0), 4.0), (POINT, 0, 0, v(12.0, 3.0), 4.0), (POINT, 0, 0, v(12.0, 9.0), 4.0), (POINT, 0, 0, v(3.0, 9.0), 4.0),
             (SEGMENT, 1, 0, (0, 1, 2, 3), 1.5), (SEGMENT, 1, 0, (2, 3, 4, 5), 1.5), (SEGMENT, 1, 0, (4, 5, 6, 7), 1.5), (SEGMENT, 1, 0, (6, 7, 0, 1), 1.5),
             (CIRCLE, 2, 0, v(18.0, 6.0, 3.0), 1.5), (ARC, 3, 0, v(7.5, 12.0, 10.5, 12.0, 7.5, 15.0), 1.5)]
    rng = np.random.default_rng(seed)
    x = v.x() + rng.normal(0.0, 0.08, (batch, len(v.v)))
    return x, items, WORLD, 4
