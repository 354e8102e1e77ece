"""The reference of the Monte-Carlo main effects (include/ezpz_amd.h: ezpz_mc_effects, ezpz_mc_effect_indices), restated from the
header's text alone: the bin of a drawn value (a count of comparisons), the validity rule of the Monte-Carlo section, the cells'
sums as the adjacent-pair tree over the 256 leaves of a block -- the tree of mc_ref.pair_tree, written with numpy's element-wise
IEEE additions over all cells at once -- with the blocks added left to right, and the closing step in Python floats and explicit
loops in the header's operation order.  tests/test_effects_cpu.py holds the host entries to it bit for bit,
tests/test_gpu_effects.py the device."""
import math

import numpy as np

from mc_ref import BLOCK

MAX_DIM, MAX_BINS, MAX_CELLS = 32, 64, 4096


def bins_of(params, edges):
    """[samples, k] int: the number of edges of dimension j that are <= p[b][j] (a NaN p: 0)."""
    params, edges = np.asarray(params, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (edges[None, :, :] <= params[:, :, None]).sum(axis=2)


def valid(m, flags, ok):
    """[samples, n_meas] bool: ok, flag bit 0 clear, m finite."""
    m = np.asarray(m, dtype=np.float64)
    v = np.isfinite(m)
    if flags is not None:
        v &= (np.asarray(flags).reshape(m.shape) & 1) == 0
    if ok is not None:
        v &= (np.asarray(ok).reshape(-1) != 0)[:, None]
    return v


def pair_tree(leaves):
    """the adjacent-pair tree along axis 0 (BLOCK leaves): for h = 1, 2, .. 128, v[t] += v[t + h] for every t a multiple of 2 h."""
    v = np.array(leaves, dtype=np.float64)
    assert v.shape[0] == BLOCK
    h = 1
    while h < BLOCK:
        v[0::2 * h] = v[0::2 * h] + v[h::2 * h]
        h *= 2
    return v[0]


def effects(params, m, flags, ok, nominal_m, edges):
    """(sums [k, B, m, 2] float64, counts [k, B, m] uint64)."""
    params, m = np.asarray(params, dtype=np.float64), np.asarray(m, dtype=np.float64)
    edges, nominal_m = np.asarray(edges, dtype=np.float64), np.asarray(nominal_m, dtype=np.float64)
    samples, k = params.shape
    n_meas, B = m.shape[1], edges.shape[1] + 1
    which, counts_for = bins_of(params, edges), valid(m, flags, ok)
    with np.errstate(invalid="ignore", over="ignore"):
        d = m - nominal_m  # one rounded subtraction
    sums, counts = np.zeros((k, B, n_meas, 2)), np.zeros((k, B, n_meas), dtype=np.uint64)
    for first in range(0, samples, BLOCK):
        n = min(BLOCK, samples - first)
        hit = np.zeros((BLOCK, k, B, n_meas), dtype=bool)
        hit[:n] = (which[first:first + n, :, None] == np.arange(B)[None, None, :])[:, :, :, None] & counts_for[first:first + n, None, None, :]
        dd = np.zeros((BLOCK, n_meas))
        dd[:n] = d[first:first + n]
        with np.errstate(invalid="ignore", over="ignore"):
            leaf = np.where(hit, dd[:, None, None, :], 0.0)
            leaf2 = np.where(hit, (dd * dd)[:, None, None, :], 0.0)  # the product rounded, then added
            sums[..., 0] = sums[..., 0] + pair_tree(leaf)
            sums[..., 1] = sums[..., 1] + pair_tree(leaf2)
        counts += hit.sum(axis=0).astype(np.uint64)
    return sums, counts


def indices(sums, counts, nominal_m):
    """(cond_mean [k, B, m], cond_var [k, B, m], eta2 [m, k], first [m, k], bins_used [m, k] uint32) of the closing step."""
    k, B, m = counts.shape
    cond_mean, cond_var = np.full((k, B, m), math.nan), np.full((k, B, m), math.nan)
    eta2, first, bins_used = np.zeros((m, k)), np.zeros((m, k)), np.zeros((m, k), dtype=np.uint32)
    for j in range(k):
        for i in range(m):
            cells = [(int(counts[j, c, i]), float(sums[j, c, i, 0]), float(sums[j, c, i, 1])) for c in range(B)]
            for c, (n, s, q) in enumerate(cells):
                if n:
                    cond_mean[j, c, i] = float(nominal_m[i]) + s / float(n)
                if n >= 2:
                    cond_var[j, c, i] = (q - _div(s * s, float(n))) / float(n - 1)
            N, S, Q, used = 0, 0.0, 0.0, 0
            for n, s, q in cells:
                if n:
                    N, S, Q, used = N + n, S + s, Q + q, used + 1
            bins_used[i, j] = used
            if used < 2:
                continue  # +0.0
            dbar = _div(S, float(N))
            SST = Q - _div(S * S, float(N))
            SSB = SSW = 0.0
            for n, s, q in cells:
                if not n:
                    continue
                mu = _div(s, float(n))
                t = mu - dbar
                SSB = SSB + float(n) * (t * t)
                w = q - _div(s * s, float(n))
                SSW = SSW + w
            if not SST > 0.0 or N - used < 1:
                eta2[i, j] = first[i, j] = math.nan
                continue
            eta2[i, j] = _div(SSB, SST)
            first[i, j] = _div(SSB - float(used - 1) * _div(SSW, float(N - used)), SST)
    return cond_mean, cond_var, eta2, first, bins_used


def _div(a, b):
    """IEEE division of Python floats; b != 0 here (the callers' divisors are counts >= 1 or an SST > 0)."""
    return a / b
