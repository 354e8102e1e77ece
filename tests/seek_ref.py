"""The reference of the dimension targets (include/ezpz_amd.h: ezpz_seek_step, ezpz_system_seek_targets), restated from the header's
text alone: STEP in Python floats -- the scaled columns, the normal matrix and the gradient as explicit sums, the hold rule, the
damping with its relative floor, L diag(d) L^T without square roots, the two substitutions, the clamp and the end test -- and the
run as the loop the header states, its evaluations made by the host-form entries (solve_batch_params, param_sensitivity, measure,
measure_response).  Python floats are IEEE doubles and nothing here is fused: the library's bytes are expected to be these.
tests/test_seek_cpu.py holds the host entry to `step`; tests/test_gpu_seek.py holds the runs to `run`."""
import math

import numpy as np

REACHED, MINIMUM, ITERATIONS, STALLED, START_FAILED = range(5)
TRIAL, STEP_MINIMUM, PIVOT = range(3)
DBL_MAX = 1.7976931348623157e308
INFO_DTYPE = np.dtype([("status", "<u4"), ("iterations", "<u4"), ("accepted", "<u4"), ("rejected", "<u4"), ("cost0", "<f8"),
                       ("cost", "<f8"), ("worst", "<f8"), ("mu", "<f8")])


def finite(v):
    return abs(v) <= DBL_MAX


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


class Policy:
    """EzpzSeekConfig with the defaults of ezpz_default_seek_config: the tables as lists of floats."""

    def __init__(self, n_param, n_meas, weight=None, tol=None, lo=None, hi=None, scale=None, max_iterations=40, mu0=1e-3, mu_up=10.0,
                 mu_down=0.1, mu_min=1e-12, mu_max=1e12, step_tol=1e-12, sens_lambda=1e-9):
        def table(v, n, default):
            return [float(a) for a in np.broadcast_to(np.asarray(default if v is None else v, dtype=np.float64), (n,))]

        self.weight, self.tol = table(weight, n_meas, 1.0), table(tol, n_meas, 1e-6)
        self.lo, self.hi, self.scale = table(lo, n_param, -math.inf), table(hi, n_param, math.inf), table(scale, n_param, 1.0)
        self.max_iterations, self.mu0, self.mu_up, self.mu_down, self.mu_min, self.mu_max = max_iterations, mu0, mu_up, mu_down, mu_min, mu_max
        self.step_tol, self.sens_lambda = step_tol, sens_lambda


def step(p, m, D, t, pol, mu):
    """STEP: (kind, p_trial, delta, held bits)."""
    n, k = len(p), len(m)
    p, m, t = [float(v) for v in p], [float(v) for v in m], [float(v) for v in t]
    w, lo, hi, s = pol.weight, pol.lo, pol.hi, pol.scale
    e = [w[i] * (t[i] - m[i]) for i in range(k)]
    Dp = [[(w[i] * float(D[i][r])) * s[r] for r in range(n)] for i in range(k)]
    A = [[0.0] * n for _ in range(n)]
    g = [0.0] * n
    for r in range(n):
        for c in range(n):
            acc = 0.0
            for i in range(k):
                acc = acc + Dp[i][r] * Dp[i][c]
            A[r][c] = acc
        acc = 0.0
        for i in range(k):
            acc = acc + Dp[i][r] * e[i]
        g[r] = acc
    held = [lo[r] == hi[r] or (p[r] == lo[r] and g[r] < 0.0) or (p[r] == hi[r] and g[r] > 0.0) for r in range(n)]
    bits = sum(1 << r for r in range(n) if held[r])
    free = [r for r in range(n) if not held[r]]
    same = (list(p), [0.0] * n, bits)
    if not free:
        return (STEP_MINIMUM,) + same
    amax = 0.0
    for r in free:
        if A[r][r] > amax:
            amax = A[r][r]
    f = 1e-2 * amax
    if f < 1e-300:
        f = 1e-300
    M = [row[:] for row in A]
    for r in free:
        M[r][r] = A[r][r] + mu * (A[r][r] if A[r][r] > f else f)
    d = [1.0] * n
    for a, kk in enumerate(free):
        d[kk] = M[kk][kk]
        if not (d[kk] > 0.0) or not finite(d[kk]):
            return (PIVOT,) + same
        for i in free[a + 1:]:
            for j in free[a + 1:]:
                M[i][j] = M[i][j] - (M[i][kk] * M[j][kk]) / d[kk]
    y = g[:]
    for a, kk in enumerate(free):
        for i in free[a + 1:]:
            y[i] = y[i] - (M[i][kk] / d[kk]) * y[kk]
    v = [0.0] * n
    for r in free:
        v[r] = y[r] / d[r]
    for a in range(len(free) - 1, 0, -1):
        i = free[a]
        for kk in free[:a]:
            v[kk] = v[kk] - (M[i][kk] / d[kk]) * v[i]
    if any(not finite(v[r]) for r in free):
        return (PIVOT,) + same
    delta = [0.0] * n
    pt = list(p)
    for r in free:
        delta[r] = s[r] * v[r]
        pt[r] = clamp(p[r] + delta[r], lo[r], hi[r])
    small = all(abs(delta[r]) <= pol.step_tol * (abs(p[r]) + pol.step_tol) for r in free)
    unmoved = all(pt[r] == p[r] for r in range(n))
    return (STEP_MINIMUM if small or unmoved else TRIAL, pt, delta, bits)


def evaluate(system, x_from, positions, q, records, pol, config=None):
    """EVALUATE of the header through the host-form entries: (good, x, m, D)."""
    x, st, _ = system.solve_batch_params(np.asarray(x_from, dtype=np.float64)[None, :], positions, np.asarray(q, dtype=np.float64)[None, :],
                                         config=config)
    S, sens = system.param_sensitivity(x, positions, np.asarray(q, dtype=np.float64)[None, :], lam=pol.sens_lambda)
    m, flags = system.measure(x, records, want_flags=True)
    D = system.measure_response(x, records, S)
    good = bool(st["converged"][0] != 0 and st["n_unsatisfied"][0] == 0 and sens[0] == 0)
    good = good and not any(pol.weight[i] > 0.0 and (flags[0, i] & 1) for i in range(len(pol.weight)))
    good = good and bool(np.all(np.abs(m) <= DBL_MAX)) and bool(np.all(np.abs(D) <= DBL_MAX))
    return good, x[0], m[0], D[0]


def judge(m, t, pol):
    """(cost, worst, reached) of the measurements m."""
    cost, worst, reached = 0.0, 0.0, True
    for i in range(len(m)):
        dev = float(t[i]) - float(m[i])
        e = pol.weight[i] * dev
        cost = cost + e * e
        if pol.weight[i] > 0.0:
            if abs(dev) > worst:
                worst = abs(dev)
            if not abs(dev) <= pol.tol[i]:
                reached = False
    return cost, worst, reached


def run_one(system, x0, positions, params0, records, t, pol, config=None):
    """One system's seek: (params, x, m, info tuple, cost_trace)."""
    n, k = len(params0), len(t)
    nan = math.nan
    trace = [nan] * (pol.max_iterations + 1)
    p = [clamp(float(params0[r]), pol.lo[r], pol.hi[r]) for r in range(n)]
    good, x, m, D = evaluate(system, x0, positions, p, records, pol, config)
    if not good:
        return p, np.array(x0, dtype=np.float64), [nan] * k, (START_FAILED, 0, 0, 0, nan, nan, nan, pol.mu0), trace
    cost, worst, reached = judge(m, t, pol)
    cost0, mu, it, accepted, rejected, stalled = cost, pol.mu0, 0, 0, 0, False
    trace[0] = cost0
    status = REACHED if reached else None
    while status is None:
        kind, pt, _, _ = step(p, m, D, t, pol, mu)
        if kind == STEP_MINIMUM:
            status = MINIMUM
        elif stalled:
            status = STALLED
        elif it == pol.max_iterations:
            status = ITERATIONS
        else:
            it += 1
            accept = False
            if kind == TRIAL:
                good, x_t, m_t, D_t = evaluate(system, x, positions, pt, records, pol, config)
                cost_t, worst_t, reached_t = judge(m_t, t, pol)
                accept = good and cost_t < cost
            if accept:
                p, x, m, D, cost, worst = pt, x_t, m_t, D_t, cost_t, worst_t
                accepted += 1
                mu = mu * pol.mu_down
                if mu < pol.mu_min:
                    mu = pol.mu_min
                if reached_t:
                    status = REACHED
            else:
                rejected += 1
                if mu >= pol.mu_max:
                    stalled = True
                else:
                    mu = mu * pol.mu_up
                    if mu > pol.mu_max:
                        mu = pol.mu_max
            trace[it] = cost
    return p, x, m, (status, it, accepted, rejected, cost0, cost, worst, mu), trace


def run(system, x0, positions, params0, records, targets, pol, config=None):
    """The batch, system after system: (params, x, m, info [batch] INFO_DTYPE, cost_trace [batch, 1 + max_iterations])."""
    batch = len(targets)
    out = [run_one(system, x0[b], positions, params0[b], records, targets[b], pol, config) for b in range(batch)]
    info = np.zeros(batch, dtype=INFO_DTYPE)
    for b, o in enumerate(out):
        info[b] = o[3]
    return (np.array([o[0] for o in out], dtype=np.float64).reshape(batch, -1), np.array([o[1] for o in out], dtype=np.float64),
            np.array([o[2] for o in out], dtype=np.float64).reshape(batch, -1), info, np.array([o[4] for o in out], dtype=np.float64))
