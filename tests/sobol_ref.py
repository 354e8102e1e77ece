"""The reference of the Sobol tolerance indices (include/ezpz_amd.h: ezpz_mc_sobol_sums, ezpz_mc_sobol_indices), restated from the
header's text alone in Python floats and explicit loops: the rows and the per-record complete-case rule, the leaves, the sums as
the adjacent-pair tree over the 256 leaves of a block (mc_ref.pair_tree) with the blocks added left to right, a FIXED dimension's
entries written as +0.0, and the closing step in the header's operation order.  tests/test_sobol_cpu.py holds the host entries to
it bit for bit, tests/test_gpu_sobol.py the device."""
import math

import numpy as np

from mc_ref import BLOCK, pair_tree

SOBOL_MAX = 32
SEED_B = 0x9E3779B97F4A7C15


def width(k):
    return 4 + 4 * k


def solved_rows(k, fixed_mask):
    return [0, 1] + [2 + j for j in range(k) if not (fixed_mask >> j) & 1]


def complete(f, flags, ok, fixed_mask):
    """[samples][m] bool: every solved row ok and, in every solved row, the record's flag bit 0 clear and its f finite."""
    samples, rows, m = f.shape
    solved = solved_rows(rows - 2, fixed_mask)
    out = []
    for b in range(samples):
        all_ok = all(ok is None or bool(ok[b, r]) for r in solved)
        out.append([all_ok and all((flags is None or not (int(flags[b, r, i]) & 1)) and math.isfinite(float(f[b, r, i])) for r in solved)
                    for i in range(m)])
    return out


def sums(f, flags, ok, nominal_m, fixed_mask=0):
    """(sums [m, 4 + 4 k] float64, n_complete [m] uint64)."""
    samples, rows, m = f.shape
    k = rows - 2
    done = complete(f, flags, ok, fixed_mask)
    n_blocks = (samples + BLOCK - 1) // BLOCK
    out = np.zeros((m, width(k)))
    n_complete = np.zeros(m, np.uint64)

    def total(leaf):
        """the sum of leaf[b] over the samples: leaf [samples] of Python floats, +0.0 where the sample is incomplete."""
        acc = 0.0
        for q in range(n_blocks):
            leaves = leaf[q * BLOCK:(q + 1) * BLOCK]
            acc = acc + pair_tree(leaves + [0.0] * (BLOCK - len(leaves)))
        return acc

    rows_f = f.tolist()
    for i in range(m):
        nom = float(nominal_m[i])
        live = [done[b][i] for b in range(samples)]
        n_complete[i] = sum(live)
        dA = [rows_f[b][0][i] - nom if live[b] else 0.0 for b in range(samples)]
        dB = [rows_f[b][1][i] - nom if live[b] else 0.0 for b in range(samples)]
        out[i, 0] = total(dA)
        out[i, 1] = total(dB)
        out[i, 2] = total([v * v if c else 0.0 for v, c in zip(dA, live)])
        out[i, 3] = total([v * v if c else 0.0 for v, c in zip(dB, live)])
        for j in range(k):
            if (fixed_mask >> j) & 1:
                continue  # written as +0.0
            t = [(rows_f[b][2 + j][i] - nom) - dA[b] if live[b] else 0.0 for b in range(samples)]
            p = [vb * vt if c else 0.0 for vb, vt, c in zip(dB, t, live)]
            q = [vt * vt if c else 0.0 for vt, c in zip(t, live)]
            out[i, 4 + j] = total(p)
            out[i, 4 + k + j] = total(q)
            out[i, 4 + 2 * k + j] = total([v * v if c else 0.0 for v, c in zip(p, live)])
            out[i, 4 + 3 * k + j] = total([v * v if c else 0.0 for v, c in zip(q, live)])
    return out, n_complete


def div(a, b):
    """IEEE division of Python floats (no ZeroDivisionError)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def indices(s, n_complete):
    """(var [m], first, total, first_var, total_var [m, k]) of the closing step."""
    m, w = s.shape
    k = w // 4 - 1
    var = np.full(m, math.nan)
    first, total, first_var, total_var = (np.full((m, k), math.nan) for _ in range(4))
    for i in range(m):
        if int(n_complete[i]) < 2:
            continue
        n = float(int(n_complete[i]))
        n2 = 2.0 * n
        sA, sB, sAA, sBB = (float(v) for v in s[i, :4])
        sab = sA + sB
        mean = div(sab, n2)
        v = div((sAA + sBB) - sab * mean, n2 - 1.0)
        var[i] = v
        if not v > 0.0:
            continue
        for j in range(k):
            P, Q, P2, Q2 = (float(s[i, 4 + c * k + j]) for c in range(4))
            pm = div(P, n)
            first[i, j] = div(pm, v)
            first_var[i, j] = div(div(div(P2, n) - pm * pm, n - 1.0), v * v)
            qm = div(div(Q, 2.0), n)
            total[i, j] = div(div(Q, n2), v)
            total_var[i, j] = div(div(div(div(Q2, 4.0), n) - qm * qm, n - 1.0), v * v)
    return var, first, total, first_var, total_var
