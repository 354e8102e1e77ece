"""The Monte-Carlo quantiles' rule (include/ezpz_amd.h, "Monte-Carlo quantiles") restated as explicit numpy: validity,
the key order, the ranks, the band and the interpolated value, every float64 operation rounded once, nothing contracted."""
import numpy as np

DTYPE = np.dtype([("n_valid", "<u8"), ("rank", "<u8"), ("rank_lo", "<u8"), ("rank_hi", "<u8"), ("frac", "<f8"), ("lo", "<f8"),
                  ("hi", "<f8"), ("value", "<f8"), ("band_lo", "<f8"), ("band_hi", "<f8")])
NONE = 0xFFFFFFFFFFFFFFFF


def keys(v):
    bits = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return bits ^ np.where(bits >> np.uint64(63) != 0, np.uint64(NONE), np.uint64(1 << 63))


def valid_keys(m, flags, ok, i):
    """The sorted keys of record i's valid values."""
    good = np.isfinite(m[:, i]) & (True if flags is None else (flags[:, i] & 1) == 0) & (True if ok is None else np.asarray(ok) != 0)
    return np.sort(keys(m[good, i]))


def quantiles(m, flags, ok, probs, z=0.0):
    out = np.zeros((m.shape[1], len(probs)), dtype=DTYPE)
    for i in range(m.shape[1]):
        k = valid_keys(m, flags, ok, i)
        x = (k ^ np.where(k >> np.uint64(63) != 0, np.uint64(1 << 63), np.uint64(NONE))).view(np.float64)  # the values, in key order
        n = len(x)
        for q, p in enumerate(np.asarray(probs, dtype=np.float64)):
            if n == 0:
                out[i, q] = (0, NONE, NONE, NONE) + (np.nan,) * 6
                continue
            top = np.float64(n - 1)
            h = p * top
            rank = int(np.floor(h))
            g = h - np.float64(rank)
            lo, hi = x[rank], x[min(rank + 1, n - 1)]
            zs = np.float64(z) * np.sqrt((np.float64(n) * p) * (np.float64(1.0) - p))
            a, b = h - zs, h + zs
            k_lo = 0 if a <= 0.0 else int(np.floor(a))
            k_hi = n - 1 if b >= top else int(np.ceil(b))
            with np.errstate(over="ignore"):
                value = lo if g == 0.0 else lo + g * (hi - lo)
            out[i, q] = (n, rank, k_lo, k_hi, g, lo, hi, value, x[k_lo], x[k_hi])
    return out
