"""The reference of the Monte-Carlo tolerance analysis (include/ezpz_amd.h: ezpz_mc_sample, ezpz_system_tolerance_mc), restated
from the header's text alone: Philox4x32-10 in Python integers, the three draws and the four kinds in Python floats in the
header's operation order, and the statistics as explicit loops -- the adjacent-pair tree over the 256 leaves of a block, the blocks
left to right, the formulas for mean, var and the bins.  tests/test_tolerance_mc_cpu.py checks it (known answers, moments) and holds
the host sampler to it; tests/test_gpu_tolerance_mc.py holds the device's statistics to it bit for bit."""
import math

import numpy as np

FIXED, UNIFORM, NORMAL, CORNER = range(4)
M32 = 0xFFFFFFFF
TWO_PI = 2.0 * math.pi  # (the double nearest 2 pi: doubling is exact)
TWO_M53 = 2.0 ** -53
UINT64_MAX = 0xFFFFFFFFFFFFFFFF
BLOCK = 256

STATS_DTYPE = np.dtype([("n_valid", "<u8"), ("n_in", "<u8"), ("argmin", "<u8"), ("argmax", "<u8"), ("nominal", "<f8"), ("sum_d", "<f8"),
                        ("sum_d2", "<f8"), ("mean", "<f8"), ("var", "<f8"), ("min", "<f8"), ("max", "<f8")])
TOTALS_DTYPE = np.dtype([("samples", "<u8"), ("n_ok", "<u8"), ("n_all_in", "<u8")])


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def words(seed, b, j, attempt):
    return philox4x32_10((b & M32, b >> 32, j, attempt), (seed & M32, seed >> 32))


def uniform(w):
    return (float(w[0] >> 5) * 67108864.0 + float(w[1] >> 6)) * TWO_M53


def normal(w):
    u1 = (float(w[0] >> 5) * 67108864.0 + float(w[1] >> 6) + 1.0) * TWO_M53
    u2 = (float(w[2] >> 5) * 67108864.0 + float(w[3] >> 6)) * TWO_M53
    angle = TWO_PI * u2
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(angle)


def normal_attempts(seed, b, j, trunc):
    """(z taken, the z of every attempt tried in order)."""
    tried = []
    for attempt in range(16):
        z = normal(words(seed, b, j, attempt))
        tried.append(z)
        if trunc == 0.0 or abs(z) <= trunc:
            return z, tried
    return math.copysign(trunc, tried[-1]), tried


def corner_ranks(dists):
    ranks, seen = [], 0
    for kind, _, _ in dists:
        ranks.append(seen if kind == CORNER else 0)
        seen += kind == CORNER
    return ranks


def draw(seed, b, j, dist, rank, nominal):
    kind, a, bb = dist
    if kind == UNIFORM:
        return nominal + (a + (bb - a) * uniform(words(seed, b, j, 0)))
    if kind == NORMAL:
        return nominal + a * normal_attempts(seed, b, j, bb)[0]
    if kind == CORNER:
        return nominal + (bb if (b >> rank) & 1 else a)
    return nominal


def sample(seed, dists, nominal, first, count):
    """params [count, n_param]; dists: (kind, a, b) per dimension."""
    ranks = corner_ranks(dists)
    out = np.zeros((count, len(dists)))
    for s in range(count):
        for j, d in enumerate(dists):
            out[s, j] = draw(seed, first + s, j, d, ranks[j], float(nominal[j]))
    return out


def pair_tree(leaves):
    v = list(leaves)
    assert len(v) == BLOCK
    h = 1
    while h < BLOCK:
        for t in range(0, BLOCK, 2 * h):
            v[t] = v[t] + v[t + h]
        h *= 2
    return v[0]


def statistics(m, flags, ok, nominal, limits=None, hist=None):
    """(stats [n_meas] STATS_DTYPE, totals [1] TOTALS_DTYPE, hist [n_meas, bins + 2] uint64 or None) of the samples m [samples,
    n_meas], flags [samples, n_meas], ok [samples], with nominal [n_meas]; limits = (lo [n_meas], hi [n_meas]); hist = (lo [n_meas],
    hi [n_meas], bins)."""
    samples, n_meas = m.shape
    stats = np.zeros(n_meas, dtype=STATS_DTYPE)
    bins = hist[2] if hist is not None else 0
    counts = np.zeros((n_meas, bins + 2), dtype=np.uint64) if bins else None
    all_in = [bool(ok[b]) for b in range(samples)]
    n_blocks = (samples + BLOCK - 1) // BLOCK
    for i in range(n_meas):
        nom = float(nominal[i])
        scale = float(bins) / (float(hist[1][i]) - float(hist[0][i])) if bins else 0.0
        n_valid = n_in = 0
        vmin, vmax, argmin, argmax = math.inf, -math.inf, UINT64_MAX, UINT64_MAX
        sum_d = sum_d2 = 0.0
        for q in range(n_blocks):
            leaves_d, leaves_d2 = [0.0] * BLOCK, [0.0] * BLOCK
            for t in range(BLOCK):
                b = q * BLOCK + t
                if b >= samples:
                    break
                v = float(m[b, i])
                valid = bool(ok[b]) and not (int(flags[b, i]) & 1) and math.isfinite(v)
                inside = valid and (limits is None or float(limits[0][i]) <= v <= float(limits[1][i]))
                all_in[b] = all_in[b] and inside
                if not valid:
                    continue
                d = v - nom
                leaves_d[t], leaves_d2[t] = d, d * d
                n_valid += 1
                n_in += inside
                if v < vmin:
                    vmin, argmin = v, b
                if v > vmax:
                    vmax, argmax = v, b
                if bins:
                    if v < float(hist[0][i]):
                        counts[i, 0] += 1
                    else:
                        k = math.floor((v - float(hist[0][i])) * scale)
                        counts[i, bins + 1 if k >= bins else 1 + k] += 1
            sum_d = sum_d + pair_tree(leaves_d)
            sum_d2 = sum_d2 + pair_tree(leaves_d2)
        mean = nom + sum_d / float(n_valid) if n_valid else math.nan
        var = (sum_d2 - sum_d * sum_d / float(n_valid)) / (float(n_valid) - 1.0) if n_valid > 1 else math.nan
        stats[i] = (n_valid, n_in, argmin, argmax, nom, sum_d, sum_d2, mean, var, vmin, vmax)
    totals = np.zeros(1, dtype=TOTALS_DTYPE)
    totals[0] = (samples, int(np.count_nonzero(ok)), sum(all_in))
    return stats, totals, counts
