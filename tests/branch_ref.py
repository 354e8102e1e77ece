"""The rule of the solution branches (include/ezpz_amd.h: THE RULE) restated in numpy, and the fixtures of its tests.

`cluster` is the sequential leader pass, to be checked by eye against the header; everything the device returns is held to it byte
for byte.  `chain(k)` and `blocks(k)` are the sketches: k triangles, every apex at distance 3 from both its parents, either chained
on one fixed base (connected, 4 + 2 k variables, 2^k assemblies) or each on a fixed base of its own (k blocks, 6 k variables, 2^k
assemblies)."""
import numpy as np

from oracle import oracle as O

NOT_OK, OVERFLOW = -1, -2
STATUS_DTYPE = np.dtype([("iterations", "<u4"), ("converged", "<u4"), ("n_unsatisfied", "<u4"), ("n_warnings", "<u4"),
                         ("final_residual_inf", "<f8"), ("final_lambda", "<f8")])
INFO_DTYPE = np.dtype([("samples", "<u8"), ("n_ok", "<u8"), ("n_branches", "<u8"), ("n_overflow", "<u8")])
BRANCH_DTYPE = np.dtype([("first", "<u8"), ("count", "<u8"), ("dist_inf", "<f8"), ("status", STATUS_DTYPE)])


def same(a, c, eps_abs, eps_rel):
    """Rows a and c (compared variables only) lie in one branch."""
    return np.all(np.abs(a - c) <= eps_abs + eps_rel * np.maximum(np.abs(a), np.abs(c)), axis=-1)


def cluster(x, ok, compare=None, eps_abs=1e-5, eps_rel=1e-5, max_branches=32, origin=None, status=None):
    """One base: x [samples, n_vars], ok [samples] -> (info [1], branches [max_branches], x_branch [max_branches, n_vars], labels)."""
    samples, n_vars = x.shape
    v = np.arange(n_vars) if compare is None else np.flatnonzero(compare)
    origin = x[0] if origin is None else origin
    labels = np.full(samples, NOT_OK, np.int32)
    leaders = []
    for i in range(samples):
        if not ok[i] or not np.all(np.isfinite(x[i, v])):
            continue
        hits = np.flatnonzero(same(x[i, v], x[leaders][:, v], eps_abs, eps_rel)) if leaders else []
        if len(hits):
            labels[i] = hits[0]  # the first, never the nearest
        elif len(leaders) < max_branches:
            labels[i] = len(leaders)
            leaders.append(i)
        else:
            labels[i] = OVERFLOW
    info = np.zeros(1, INFO_DTYPE)
    info[0] = (samples, np.count_nonzero(labels != NOT_OK), len(leaders), np.count_nonzero(labels == OVERFLOW))
    branches, x_branch = np.zeros(max_branches, BRANCH_DTYPE), np.zeros((max_branches, n_vars))
    for slot, i in enumerate(leaders):
        branches["first"][slot], branches["count"][slot] = i, np.count_nonzero(labels == slot)
        branches["dist_inf"][slot] = np.fmax.reduce(np.abs(x[i, v] - origin[v]), initial=0.0)  # (from +0.0; a NaN never wins)
        if status is not None:
            branches["status"][slot] = status[i]
        x_branch[slot] = x[i]
    return info, branches, x_branch, labels


def cluster_batch(x, ok, origin=None, status=None, **rule):
    """x [batch, samples, n_vars]: `cluster` per base, stacked as the library lays its outputs out."""
    parts = [cluster(x[b], ok[b], origin=None if origin is None else origin[b], status=None if status is None else status[b], **rule)
             for b in range(len(x))]
    return tuple(np.concatenate(p) if k == 0 else np.stack(p) for k, p in enumerate(zip(*parts)))


def result_bytes(info, branches, x_branch, labels):
    return [np.ascontiguousarray(a).tobytes() for a in (info, branches, x_branch, labels)]


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
BASE = 4.0  # the fixed base's length: an apex lies sqrt(9 - 4) = 2.24 above or below it
SIDE = 3.0


class Fixture:
    """records, n_vars, the fixed variables, and x0: the base of the runs -- the fixed variables at their values, the free points
    spread out above the base line (no two on one spot, none on the line: both are degenerate starts)."""

    def __init__(self, cons, n_vars, fixed, x0):
        self.records, self.n_vars, self.fixed, self.x0 = O.stack(cons), n_vars, fixed, np.array(x0, dtype=np.float64)

    def spread(self, half_width):
        """(kind, a, b) per variable: FIXED for the fixed variables, UNIFORM +- half_width for the others."""
        return [(0, 0.0, 0.0) if v in self.fixed else (1, -half_width, half_width) for v in range(self.n_vars)]


def _point(i):
    return (2 * i, 2 * i + 1)


def chain(k):
    """Points 0 and 1 fixed at (0, 0) and (BASE, 0); point i + 2 at SIDE from points i and i + 1: connected, 4 + 2 k variables."""
    cons, x0 = [O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(2, BASE), O.fixed(3, 0.0)], [0.0, 0.0, BASE, 0.0]
    for i in range(k):
        cons += [O.distance(_point(i + 2), _point(i), SIDE), O.distance(_point(i + 2), _point(i + 1), SIDE)]
        x0 += [BASE / 2 + 1.5 * i, 1.0 + (i % 2)]
    return Fixture(cons, 4 + 2 * k, [0, 1, 2, 3], x0)


def blocks(k):
    """k triangles of their own, block j on the fixed base (10 j, 0) .. (10 j + BASE, 0): k components, 6 k variables."""
    cons, fixed, x0 = [], [], []
    for j in range(k):
        p, q, apex = _point(3 * j), _point(3 * j + 1), _point(3 * j + 2)
        cons += [O.fixed(p[0], 10.0 * j), O.fixed(p[1], 0.0), O.fixed(q[0], 10.0 * j + BASE), O.fixed(q[1], 0.0),
                 O.distance(apex, p, SIDE), O.distance(apex, q, SIDE)]
        fixed += [*p, *q]
        x0 += [10.0 * j, 0.0, 10.0 * j + BASE, 0.0, 10.0 * j + BASE / 2, 1.0]
    return Fixture(cons, 6 * k, fixed, x0)


def starts(E, fixture, seed, samples, half_width=3.0, x0=None):
    """The starts of a run on the host: ezpz_mc_sample around x0, sample 0 the base itself."""
    x0 = fixture.x0 if x0 is None else np.asarray(x0, dtype=np.float64)
    s = E.mc_sample(seed, [E.McDist(*t) for t in fixture.spread(half_width)], x0, 0, samples)
    s[0] = x0
    return s


def ok_of(converged, n_unsatisfied):
    return (np.asarray(converged) != 0) & (np.asarray(n_unsatisfied) == 0)
