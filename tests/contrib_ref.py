"""The reference of the tolerance contributors (include/ezpz_amd.h: ezpz_mc_moments, ezpz_mc_contributors), restated from the
header's text alone in Python floats and explicit loops: the sample vector and the complete-case rule, the moments as the
adjacent-pair tree over the 256 leaves of a block (mc_ref.pair_tree) with the blocks added left to right, and the closing step --
covariance, LDL^T with dropped dimensions, the two triangular solves, r2 and the contributions -- in the header's operation order.
tests/test_contributors_cpu.py holds the host entry to it bit for bit, tests/test_gpu_contributors.py the device."""
import math

import numpy as np

from mc_ref import BLOCK, pair_tree

MOMENT_MAX = 64
UINT64_MAX = 0xFFFFFFFFFFFFFFFF


def entries(K):
    return K + K * (K + 1) // 2


def g_at(K, a, b):
    """the place of G[a][b], a <= b: behind the K sums, the upper triangle row-major."""
    return K + sum(K - r for r in range(a)) + (b - a)


def complete(m, flags, ok):
    """[samples] bool: ok, every record's flag bit 0 clear and every m finite."""
    samples, n_meas = m.shape
    out = []
    for b in range(samples):
        c = True if ok is None else bool(ok[b])
        for i in range(n_meas):
            c = c and (flags is None or not (int(flags[b, i]) & 1)) and math.isfinite(float(m[b, i]))
        out.append(c)
    return out


def moments(params, m, flags, ok, nominal_p, nominal_m):
    """(moments [K + K (K + 1) / 2] float64, n_complete)."""
    samples, k = params.shape
    n_meas = m.shape[1]
    K = k + n_meas
    done = complete(m, flags, ok)
    z = []
    for b in range(samples):
        if not done[b]:
            z.append(None)
            continue
        z.append([float(params[b, j]) - float(nominal_p[j]) for j in range(k)] + [float(m[b, i]) - float(nominal_m[i]) for i in range(n_meas)])
    n_blocks = (samples + BLOCK - 1) // BLOCK

    def total(leaf):
        acc = 0.0
        for q in range(n_blocks):
            leaves = [0.0] * BLOCK
            for t in range(BLOCK):
                b = q * BLOCK + t
                if b < samples and z[b] is not None:
                    leaves[t] = leaf(z[b])
            acc = acc + pair_tree(leaves)
        return acc

    out = np.zeros(entries(K))
    for a in range(K):
        out[a] = total(lambda v, a=a: v[a])
    at = K
    for a in range(K):
        for b in range(a, K):
            assert at == g_at(K, a, b)
            out[at] = total(lambda v, a=a, b=b: v[a] * v[b])
            at += 1
    return out, sum(done)


def contributors(mom, n_complete, k, m, pivot_rel=2.0 ** -26):
    """(cov [K, K], beta [m, k], contrib [m, k], r2 [m], dropped) of the closing step."""
    K = k + m
    mom = [float(v) for v in mom]
    cov, beta, contrib, r2 = np.zeros((K, K)), np.zeros((m, k)), np.zeros((m, k)), np.zeros(m)
    if n_complete < 2:
        for arr in (cov, beta, contrib, r2):
            arr[...] = math.nan
        return cov, beta, contrib, r2, UINT64_MAX
    n = float(n_complete)
    c = [[0.0] * K for _ in range(K)]
    for a in range(K):
        for b in range(a, K):
            c[a][b] = c[b][a] = (mom[g_at(K, a, b)] - mom[a] * mom[b] / n) / (n - 1.0)
    L = [[0.0] * k for _ in range(k)]
    d, kept, dropped = [0.0] * k, [False] * k, 0
    for j in range(k):
        dj = c[j][j]
        for l in range(j):
            if kept[l]:
                t = L[j][l] * d[l]
                dj = dj - L[j][l] * t
        kept[j] = c[j][j] > 0.0 and dj > pivot_rel * c[j][j]
        if not kept[j]:
            dropped |= 1 << j
            continue
        d[j] = dj
        for i in range(j + 1, k):
            v = c[i][j]
            for l in range(j):
                if kept[l]:
                    t = L[j][l] * d[l]
                    v = v - L[i][l] * t
            L[i][j] = v / dj
    for i in range(m):
        y = [0.0] * k
        for j in range(k):
            if kept[j]:
                y[j] = c[j][k + i]
                for l in range(j):
                    if kept[l]:
                        y[j] = y[j] - L[j][l] * y[l]
        w = [y[j] / d[j] if kept[j] else 0.0 for j in range(k)]
        bi = [0.0] * k
        for j in range(k - 1, -1, -1):
            if kept[j]:
                bi[j] = w[j]
                for l in range(j + 1, k):
                    if kept[l]:
                        bi[j] = bi[j] - L[l][j] * bi[l]
        explained = 0.0
        for j in range(k):
            if kept[j]:
                explained = explained + bi[j] * c[j][k + i]
        vm = c[k + i][k + i]
        for j in range(k):
            beta[i, j] = bi[j]
            contrib[i, j] = math.nan if not vm > 0.0 else bi[j] * bi[j] * c[j][j] / vm if kept[j] else 0.0
        r2[i] = explained / vm if vm > 0.0 else math.nan
    for a in range(K):
        for b in range(K):
            cov[a, b] = c[a][b]
    return cov, beta, contrib, r2, dropped
