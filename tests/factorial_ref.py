"""The reference of the factorial effects (include/ezpz_amd.h: ezpz_mc_factorial), restated from the header's text alone: the
validity rule of the Monte-Carlo section, one rounded subtraction, the Walsh-Hadamard levels as numpy's element-wise IEEE additions
and subtractions over reshaped views -- level l pairs the two halves of axis 1 of the view [N / 2h, 2, h] -- the scaling, the masked
sums as the adjacent-pair tree of tests/effects_ref.py over blocks of 256 leaves with the blocks added left to right, and the closing
step in Python floats and explicit loops in the header's operation order.  tests/test_factorial_cpu.py holds the host entry to it
bit for bit, tests/test_gpu_factorial.py the device."""
import math

import numpy as np

from effects_ref import pair_tree, valid
from mc_ref import BLOCK

MAX_CORNERS, MAX_MEAS = 20, 32
DTYPE = np.dtype([("n_valid", "<u8"), ("complete", "<u4"), ("corner_hi", "<u4"), ("corner_lo", "<u4"), ("reserved", "<u4"),
                  ("mean_dev", "<f8"), ("var", "<f8"), ("m_hi", "<f8"), ("m_lo", "<f8")])
NAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def transform(y):
    """coef [N] of the values y [N], N = 2^kc: the levels in place, then the scaling."""
    w = np.array(y, dtype=np.float64)
    N = len(w)
    kc = N.bit_length() - 1
    assert N == 1 << kc
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(kc):
            h = 1 << l
            v = w.reshape(N // (2 * h), 2, h)
            lo, hi = v[:, 0, :].copy(), v[:, 1, :].copy()
            v[:, 0, :] = lo + hi
            v[:, 1, :] = hi - lo
        return w * 2.0 ** -kc


def masked_sum(sq, member):
    """the sum of sq [N] over the S with member[S], in the section's order: +0.0 leaves elsewhere and past N, blocks of 256 by the
    pair tree, the blocks left to right from +0.0."""
    N = len(sq)
    blocks = (N + BLOCK - 1) // BLOCK
    leaves = np.zeros(blocks * BLOCK)
    leaves[:N] = np.where(member, sq, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        per_block = pair_tree(leaves.reshape(blocks, BLOCK).T)
    total = 0.0
    for v in per_block.tolist():
        total = total + v
    return total


def factorial(m, flags, ok, nominal_m, want_coef=True):
    """(info [n_meas] DTYPE, main [n_meas, kc], pair [n_meas, kc, kc], ss_order [n_meas, kc + 1], ss_total, first, total [n_meas, kc],
    coef [n_meas, N])."""
    m, nominal_m = np.asarray(m, dtype=np.float64), np.asarray(nominal_m, dtype=np.float64)
    N, n_meas = m.shape
    kc = N.bit_length() - 1
    assert N == 1 << kc and kc >= 1
    n_valid = valid(m, flags, ok).sum(axis=0)
    info = np.zeros(n_meas, dtype=DTYPE)
    main, pair = np.full((n_meas, kc), NAN), np.full((n_meas, kc, kc), NAN)
    ss_order, ss_total = np.full((n_meas, kc + 1), NAN), np.full((n_meas, kc), NAN)
    first, total, coef = np.full((n_meas, kc), NAN), np.full((n_meas, kc), NAN), np.full((n_meas, N), NAN)
    S = np.arange(N, dtype=np.uint32)
    order = np.zeros(N, dtype=np.uint32)
    for c in range(kc):
        order += (S >> c) & 1
    for i in range(n_meas):
        info["n_valid"][i] = n_valid[i]
        if n_valid[i] != N:
            info["mean_dev"][i] = info["var"][i] = info["m_hi"][i] = info["m_lo"][i] = NAN
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            y = m[:, i] - nominal_m[i]  # one rounded subtraction
            cf = transform(y)
            sq = cf * cf  # the product rounded, then added
        coef[i] = cf
        for o in range(kc + 1):
            ss_order[i, o] = masked_sum(sq, order == o)
        for c in range(kc):
            ss_total[i, c] = masked_sum(sq, ((S >> c) & 1) != 0)
            main[i, c] = cf[1 << c]
            for e in range(kc):
                pair[i, c, e] = 0.0 if c == e else cf[(1 << c) | (1 << e)]
        var = 0.0
        for o in range(1, kc + 1):
            var = var + float(ss_order[i, o])
        hi = lo = 0
        for c in range(kc):
            a = float(main[i, c])
            if a > 0.0:
                hi |= 1 << c
            if a < 0.0:
                lo |= 1 << c
            first[i, c] = 0.0 if var == 0.0 else _div(a * a, var)
            total[i, c] = 0.0 if var == 0.0 else _div(float(ss_total[i, c]), var)
        info[i] = (N, 1, hi, lo, 0, cf[0], var, m[hi, i], m[lo, i])
    return info, main, pair, ss_order, ss_total, first, total, (coef if want_coef else None)


def _div(a, b):
    """IEEE division of Python floats; a zero divisor gives what the hardware gives (b is a sum of squares: +0.0 is handled by the
    caller, a NaN or an inf passes through)."""
    if b == 0.0:
        return math.nan
    return a / b
