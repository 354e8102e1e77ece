"""The reference of the low-discrepancy draws (include/ezpz_amd.h: THE SEQUENCE), restated from the header's text in numpy: the
Sobol' point from direction numbers taken from the installed torch (30 bits) or scipy (32 bits) -- never from the library's table --
the shift from tests/mc_ref.py's Philox, u, and Wichura's AS 241 PPND16 in Python floats in the published operation order (the
coefficients are those of CPython's statistics.NormalDist.inv_cdf).  tests/test_sequence_cpu.py holds the host sampler to it and
tests/test_gpu_sequence.py the device's."""
import math

import numpy as np

import mc_ref

SEQUENCE = 1  # EZPZ_MC_SEQUENCE
DIMS = 64
SHIFT_ATTEMPT = 0xFFFFFFFF
TWO_M32 = 2.0 ** -32


def direction_numbers():
    """V [64, 32] uint32, bit 31 first.  scipy holds all 32 columns; torch the first 30 (the last two columns are then zero: they
    only reach samples >= 2^30)."""
    try:
        from scipy.stats import qmc
        return np.asarray(qmc.Sobol(d=DIMS, scramble=False, bits=32)._sv, dtype=np.uint32).copy(), 32
    except ImportError:
        import torch
        state = torch.quasirandom.SobolEngine(DIMS, scramble=False).sobolstate.numpy().astype(np.uint64)
        v = np.zeros((DIMS, 32), dtype=np.uint32)
        v[:, :state.shape[1]] = (state << np.uint64(32 - state.shape[1])).astype(np.uint32)
        return v, int(state.shape[1])


_V = None


def table():
    global _V
    if _V is None:
        _V = direction_numbers()
    return _V[0]


def points(j, first, count):
    """x [count] uint32 of the samples first .. first + count - 1 for dimension j."""
    b = np.arange(first, first + count, dtype=np.uint64)
    g = (b ^ (b >> np.uint64(1))).astype(np.uint64)
    x = np.zeros(count, dtype=np.uint32)
    v = table()[j]
    for c in range(32):
        x ^= np.where((g >> np.uint64(c)) & np.uint64(1), v[c], np.uint32(0)).astype(np.uint32)
    return x


def shift(seed, j):
    return mc_ref.words(seed, 0, j, SHIFT_ATTEMPT)[0]


def units(seed, j, first, count):
    """u [count]: ((x ^ s) + 0.5) * 2^-32, exact."""
    k = points(j, first, count) ^ np.uint32(shift(seed, j))
    return (k.astype(np.float64) + 0.5) * TWO_M32


def ppnd16(p):
    """(z, central): Wichura's AS 241 PPND16 as published; central: the branch of + - * / alone."""
    q = p - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                   4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q
        den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                   2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                 4.2313330701600911252e+1) * r + 1.0)
        return num / den, True
    r = p if q <= 0.0 else 1.0 - p
    r = math.sqrt(-math.log(r))
    if r <= 5.0:
        r = r - 1.6
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                   1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0)
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                   1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                 2.05319162663775882187e+0) * r + 1.0)
    else:
        r = r - 5.0
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                   2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0)
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                   7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                 5.99832206555887937690e-1) * r + 1.0)
    x = num / den
    return (-x if q < 0.0 else x), False


def normal_z(u, trunc):
    """(z, central) of one u by the header's rule."""
    if trunc == 0.0:
        return ppnd16(u)
    p_lo = 0.5 * math.erfc(trunc / math.sqrt(2.0))
    p_hi = 1.0 - p_lo
    z, central = ppnd16(p_lo + (p_hi - p_lo) * u)
    return min(max(z, -trunc), trunc), central


def sample(seed, dists, nominal, first, count):
    """(params [count, n_param], central [count, n_param] bool); dists: (kind, a, b, flagged) per dimension.  central: the draw is
    bit-reproducible between the host and the device (everything but a NORMAL draw off the inverse's central branch -- or a plain
    NORMAL draw)."""
    plain = mc_ref.sample(seed, [(k, a, b) for k, a, b, _ in dists], nominal, first, count)
    out, central = plain.copy(), np.ones(plain.shape, dtype=bool)
    for j, (kind, a, bb, flagged) in enumerate(dists):
        if kind == mc_ref.NORMAL:
            central[:, j] = False
        if not flagged or kind not in (mc_ref.UNIFORM, mc_ref.NORMAL):
            continue
        u = units(seed, j, first, count)
        nom = float(nominal[j])
        for s in range(count):
            if kind == mc_ref.UNIFORM:
                out[s, j] = nom + (a + (bb - a) * float(u[s]))
            else:
                z, central[s, j] = normal_z(float(u[s]), bb)
                out[s, j] = nom + a * z
    return out, central
