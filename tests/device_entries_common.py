"""What tests/test_gpu_device_entries.py is built from: the FreedomAnalysis systems of each placement, one `Call` per `_device`
entry (its device buffers, its enqueue on a stream of the caller's, its outputs refilled with a pattern before every run), and
the cases of the two-stream tests with their batch sizes.  Inputs and references are the existing ones (redundancy_ref,
sensitivity_ref, sweep_common, gen)."""
import numpy as np

import gen
import redundancy_ref as RR
import sensitivity_ref as SR
import sweep_common as SC
from oracle import oracle as O
from oracle import textual as T

PATTERN = 0xA5  # every byte of every output before a run


# ---- FreedomAnalysis: the smallest system of each placement (csrc/freedom.hip: build_freedom) ------------------------------------
def _blocks_without_every_28th(lines):
    ref = T.load(T.gen_big_problem(lines))
    keep = [c for i, c in enumerate(ref.constraints) if not (i % 28 == 3)]
    return O.stack(keep), ref.num_vars, ref.guesses


FREEDOM_PLACEMENTS = ("lane", "lane_groups", "lds", "global", "wide")
_FREEDOM = {}


def freedom_system(E, name):
    """(system, records, n_vars, values(batch) -> [batch, n]) of a placement; the sketches' values are polished by a solve, as the
    host tests of such systems do, the block systems' are drawn (linear: every system sees the same dependencies)."""
    if name in _FREEDOM:
        return _FREEDOM[name]
    polish, spread, key = True, 0.02, 43
    if name in ("lane", "lane_groups"):  # 180 components (a lane per component, one system per workgroup) / 30 (four systems)
        recs, n, g = _blocks_without_every_28th(60 if name == "lane" else 10)
        polish, spread, key = False, 0.2, 31
    elif name == "lds":  # one component of 46 variables: a workgroup per system, workspace in LDS
        recs, g = gen.connected_sketch(24, 5)
        recs, n = recs[:-3], len(g)
    elif name == "global":  # one component of 88 variables: workspace in global memory, no workgroup waits for another
        recs, g = gen.connected_sketch(44, 13)
        recs, n = recs[:-1], len(g)
    elif name == "wide":  # 240 variables in one component: the QR over many workgroups
        recs, g = SC.chain(120)
        recs, n, spread, key = recs[:-1], len(g), 0.05, 41
    else:
        raise KeyError(name)
    s = E.System(recs, n)
    cache = {}

    def values(batch):
        if batch not in cache:
            x = g[None, :] + gen.keyed_uniform(key, batch, n, -spread, spread)
            if polish:
                x, st, _ = s.solve_batch(x, E.Config(max_iterations=60))
                assert np.all(st["n_unsatisfied"] == 0)
            cache[batch] = np.ascontiguousarray(x)
        return cache[batch]

    _FREEDOM[name] = (s, recs, n, values)
    return _FREEDOM[name]


def freedom_rule(E, s):
    """(components, ws, largest n) by build_freedom's rule, from the system's own Jacobian pattern: components of the row /
    variable graph that hold a variable with an entry, ws = max over them of m n + 2 n^2 + 2 n doubles."""
    info = s.info()
    zj, m, n = info["nnz_j"], info["n_rows"], s.n_vars
    rows, cols = np.zeros(max(zj, 1), np.uint32), np.zeros(max(zj, 1), np.uint32)
    E.lib().ezpz_system_jacobian_pattern(s._h, rows.ctypes.data, cols.ctypes.data)
    parent = list(range(n + m))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for r, c in zip(rows[:zj].tolist(), cols[:zj].tolist()):
        a, b = find(c), find(n + r)
        if a != b:
            parent[max(a, b)] = min(a, b)
    size = {}
    for v in set(cols[:zj].tolist()):
        size.setdefault(find(v), [0, 0])[0] += 1
    for r in range(m):
        root = find(n + r)
        if root in size:
            size[root][1] += 1
    ws = max(mc * nc + 2 * nc * nc + 2 * nc for nc, mc in size.values())
    return len(size), ws, max(nc for nc, _ in size.values())


# ---- one call of a `_device` entry --------------------------------------------------------------------------------------------------
class Call:
    """Inputs on the device (kept alive here), outputs, and `enqueue(stream handle)`."""

    def __init__(self, enqueue, outputs, inputs, batch):
        self.enqueue, self.outputs, self.inputs, self.batch = enqueue, outputs, inputs, batch

    def refill(self):
        for t in self.outputs:
            t.view(-1).view(_torch().uint8).fill_(PATTERN)

    def run(self, stream):
        self.enqueue(stream.cuda_stream)

    def snapshot(self):
        """Copies of the outputs as bytes, on the device (compared there: some are hundreds of megabytes)."""
        return [t.view(-1).view(_torch().uint8).clone() for t in self.outputs]

    def equals(self, snapshot):
        torch = _torch()
        return [bool(torch.equal(t.view(-1).view(torch.uint8), ref)) for t, ref in zip(self.outputs, snapshot)]

    def written(self):
        """Whether every output holds something other than the pattern (a call that did nothing would pass an equality of patterns)."""
        return [bool((t.view(-1).view(_torch().uint8) != PATTERN).any()) for t in self.outputs]


def _torch():
    import torch

    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _out(shape, dtype):
    return _torch().empty(shape, dtype=dtype, device="cuda")


def _status_bytes(count):
    from ezpz_amd._lib import STATUS_DTYPE

    return _out((max(count, 1) * STATUS_DTYPE.itemsize,), _torch().uint8)


def _tiled(x, batch, key, spread):
    """`batch` value vectors: the rows of x over and over, every one moved a little (keyed: `key` gives other values)."""
    x = np.atleast_2d(x)
    reps = (batch + len(x) - 1) // len(x)
    return np.ascontiguousarray(np.tile(x, (reps, 1))[:batch] + gen.keyed_uniform(key, batch, x.shape[1], -spread, spread))


def redundancy_call(s, c, batch, key, focus):
    torch = _torch()
    x = _dev(_tiled(c["x"], batch, key, 1e-3))
    n_cs, m = len(c["recs"]), s.info()["n_rows"]
    focus = list(focus)
    con, rows = _out((batch, n_cs), torch.uint8), _out((batch, m), torch.uint8)
    rank, group = _out((batch,), torch.int32), _out((batch, max(len(focus), 1), n_cs), torch.uint8)

    def enqueue(stream):
        s.redundancy_device(x.data_ptr(), batch, con.data_ptr(), rows.data_ptr(), rank.data_ptr(), focus or None,
                            group.data_ptr() if focus else 0, stream=stream)

    return Call(enqueue, [con, rows, rank] + ([group] if focus else []), [x], batch)


def sensitivity_call(s, ref, batch, key, pos=None, columns=None):
    """`ref`: a system of sensitivity_ref; pos / columns: another list (a subset of ref's, with its columns of the parameters)."""
    torch = _torch()
    pos = ref["pos"] if pos is None else pos
    params = ref["params"] if columns is None else ref["params"][:, columns]
    x = _dev(_tiled(ref["x"], batch, key, 1e-4))
    p = _dev(_tiled(params, batch, key + 1, 1e-4))
    S = _out((batch, len(pos), ref["n_vars"]), torch.float64)
    st, deg = _out((batch,), torch.int32), _out((batch,), torch.int32)

    def enqueue(stream):
        s.param_sensitivity_device(x.data_ptr(), pos, p.data_ptr(), batch, S.data_ptr(), st.data_ptr(), lam=ref["lam"],
                                   degenerate_ptr=deg.data_ptr(), stream=stream)

    return Call(enqueue, [S, st, deg], [x, p], batch)


def driven_call(E, s, recs, g, batch, seed, steps=0, config=None, pos=None):
    """steps == 0: solve_batch_params_device; else sweep_params_device of that many steps.  pos: a subset of the driven list."""
    torch = _torch()
    all_pos, params, x0 = SC.driven_walk(E, recs, g, batch, max(steps, 1), seed)
    if pos is not None:
        params = np.ascontiguousarray(params[:, :, np.searchsorted(all_pos, pos)])
    else:
        pos = all_pos
    n, n_cs, rows = len(g), len(recs), max(steps, 1) * batch
    xd, pd = _dev(x0), _dev(params if steps else params[0])
    xo, st, mask = _out((rows, n), torch.float64), _status_bytes(rows), _out((rows, n_cs), torch.uint8)

    def enqueue(stream):
        if steps:
            s.sweep_params_device(xd.data_ptr(), pos, pd.data_ptr(), steps, batch, xo.data_ptr(), st.data_ptr(), mask.data_ptr(),
                                  stream=stream, config=config)
        else:
            s.solve_batch_params_device(xd.data_ptr(), pos, pd.data_ptr(), batch, xo.data_ptr(), st.data_ptr(), mask.data_ptr(),
                                        stream=stream, config=config)

    return Call(enqueue, [xo, st, mask], [xd, pd], batch)


def solve_call(s, g, n_cs, batch, key, config=None):
    torch = _torch()
    xd = _dev(g[None, :] + gen.keyed_uniform(key, batch, len(g), -0.03, 0.03))
    xo, st, mask = _out((batch, len(g)), torch.float64), _status_bytes(batch), _out((batch, n_cs), torch.uint8)

    def enqueue(stream):
        s.solve_batch_device(xd.data_ptr(), batch, xo.data_ptr(), st.data_ptr(), mask.data_ptr(), stream=stream, config=config)

    return Call(enqueue, [xo, st, mask], [xd], batch)


def freedom_call(s, n, values, batch, key):
    torch = _torch()
    x = _dev(_tiled(values(3), batch, key, 1e-3))
    mask, part, count = _out((batch, n), torch.uint8), _out((batch, n), torch.float64), _out((batch,), torch.int32)

    def enqueue(stream):
        s.freedom_batch_device(x.data_ptr(), batch, mask.data_ptr(), part.data_ptr(), count.data_ptr(), stream=stream)

    return Call(enqueue, [mask, part, count], [x], batch)


# ---- the cases of "long call, then short call": (entry, placement) -> (systems of A, systems of B) -----------------------------
# Sized on an MI355X so that A alone takes at least ten times the host's gap between the two enqueues plus B alone, with room, and
# stays under about 50 ms (the measured times: the docstring of test_long_call_then_short_call).
BATCHES = {
    ("redundancy", "blocks"): (131072, 3),
    ("redundancy", "sketch24"): (16384, 3),
    ("redundancy", "sketch150"): (2560, 1),
    ("sensitivity", "massive40"): (65536, 3),
    ("sensitivity", "sketch150"): (8192, 2),
    ("sensitivity", "hub512"): (3584, 1),
    ("params", "sub-wavefront teams"): (4194304, 4),
    ("params", "barrier workgroup"): (32768, 2),
    ("params", "record walk"): (16384, 2),
    ("params", "global workspace"): (8192, 1),
    ("params", "fronts"): (32768, 2),
    ("sweep", "sub-wavefront teams"): (2097152, 4),
    ("sweep", "barrier workgroup"): (16384, 2),
    ("sweep", "record walk"): (8192, 2),
    ("sweep", "global workspace"): (5120, 1),
    ("sweep", "fronts"): (16384, 2),
    ("freedom", "lane"): (131072, 3),
    ("freedom", "lds"): (32768, 3),
    ("freedom", "global"): (8192, 2),
}
SWEEP_STEPS = 3


def driven_shape(E, placement, setenv):
    """(records, guesses, team_size, config, finish(system)) of a one-workgroup shape of the driven entries.  setenv(name, value):
    the test's monkeypatch (the fronts on ONE workgroup are asked for through the environment when the system is created)."""
    config, fronts = None, False
    if placement == "global workspace":  # the system of test_gpu_params.test_workspace_in_global_memory
        (recs, g), team, mode = SC.chain(2000), 256, 2
        config = E.Config().with_max_iterations(3)
    elif placement == "fronts":
        (recs, g), team, mode, fronts = SC.chain(40), E.TEAM_FRONTS, 5, True
        setenv("EZPZ_FRONT_WGS", "1")
    else:
        recs, g, team, mode = {name: (r, gg, t, m) for name, r, gg, t, m in SC.shapes(E)}[placement]

    def make():
        s = E.System(recs, len(g), team_size=team)
        info = s.info()
        assert info["team_mode"] == mode and info["grid_workgroups"] == 1, (placement, info)
        if placement == "global workspace":
            assert info["workspace_in_lds"] == 0, info
        if fronts:
            assert info["front_workgroups"] == 1, info
            s.set_params_route("fronts")
        return s

    return recs, g, config, make


def two_calls(E, entry, placement, setenv, sizes=None):
    """(system, call A, call B) of a case of BATCHES (sizes: other batch sizes, for the script that chose them)."""
    batch_a, batch_b = sizes or BATCHES[(entry, placement)]
    if entry == "redundancy":
        c = RR.case(placement)
        s = E.System(c["recs"], c["n_vars"])
        return s, redundancy_call(s, c, batch_a, 101, c["focus"]), redundancy_call(s, c, batch_b, 202, c["focus"])
    if entry == "sensitivity":
        ref = SR.system(placement)
        s = E.System(ref["recs"], ref["n_vars"])
        return s, sensitivity_call(s, ref, batch_a, 101), sensitivity_call(s, ref, batch_b, 202)
    if entry in ("params", "sweep"):
        recs, g, config, make = driven_shape(E, placement, setenv)
        s, steps = make(), SWEEP_STEPS if entry == "sweep" else 0
        return s, driven_call(E, s, recs, g, batch_a, 101, steps, config), driven_call(E, s, recs, g, batch_b, 202, steps, config)
    if entry == "freedom":
        s, _, n, values = freedom_system(E, placement)
        return s, freedom_call(s, n, values, batch_a, 101), freedom_call(s, n, values, batch_b, 202)
    raise KeyError(entry)
