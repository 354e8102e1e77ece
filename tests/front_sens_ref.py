"""Test infrastructure: a numpy executor of the sensitivity route of the fronts (csrc/front_sens_kernel.hip.hpp) --
front_ref.Plan's blob and the tables csrc/front_sens_plan.cpp derives from it (ezpz_debug_front_sens_tables), operation for
operation what the kernel does: the factorisation with an all-zero right-hand side, then per listed position the rhs rows
zeroed, g_j in a residual-space vector that is zero elsewhere, the rhs-only assembly stream, the forward pass over the fronts
(rhs-only extend-add, the remote children's last rows as chunks, row S against the panel, the rows below into the update
matrix's last row) and the backward pass.  It checks the HOST tables on the CPU.  Also the inputs of the sensitivity tests of
the fronts (the CPU test measures the reference's spread on exactly the systems the GPU test checks).  Not part of the product."""
import numpy as np

import ezpz_amd as E
import front_ref as F
import gen
import sensitivity_ref as R
from oracle import oracle as O
from front_ref import FASM_NOP, FASM_RHS, FRONT_EXPORTS, FRONT_REMOTE_PARENT, tri

LAM = 1e-9
# name -> (family, points, seed) of gen.graph_sketch; tree60 is the system of test_graph_families_on_fronts
WIDE = {"tree60": ("tree", 60, 11), "tree108": ("tree", 108, 7020), "tree144": ("tree", 144, 7036), "comb213": ("comb", 213, 7019)}
# name -> the workgroup counts at which the planner gives its share of the LDS a plan
WIDE_WGS = {"tree60": (1, 2, 4), "tree108": (1, 2, 4), "tree144": (4,), "comb213": (4,)}


def inputs(name):
    """sketchN = gen.connected_sketch(N, 1000 + N); band / hub = gen.graph_sketch(name, 50, default_rng(21));
    mixed40 = gen.mixed_sketch(40, 77): all 13 kinds with a parameter, drawn weights -- mixed40:unit with every weight 1.0,
    mixed40:double with every weight 2.0, mixed40+corner with the disjoint corner of `corner` appended;
    linear100 = gen.linear_chain(100): the linear build -- linear100:weighted with weights of default_rng(78).uniform(0.5, 2.0);
    WIDE (tree60, tree108, tree144, comb213): gen.graph_sketch systems chosen by the shape of their plans -- fronts of up to 63
    rows, remote children of more than 50 rows, minimum-degree plans (tests/test_front_sens_cpu.py pins those shapes)."""
    if name in WIDE:
        family, npts, seed = WIDE[name]
        rng = np.random.default_rng(seed)
        if seed >= 7000:  # the draw of tests/test_gpu_fuzz.py and test_fronts_cpu.py: the number of points comes first
            assert int(rng.integers(20, 500)) == npts, name
        return gen.graph_sketch(family, npts, rng)
    if name.startswith("mixed40"):
        recs, g = gen.mixed_sketch(40, 77)
        if name == "mixed40+corner":
            extra, vals = corner(len(g))
            return np.concatenate([recs, extra]), np.concatenate([g, vals])
        if name != "mixed40":
            recs["weight"] = {"mixed40:unit": 1.0, "mixed40:double": 2.0}[name]
        return recs, g
    if name.startswith("linear100"):
        recs, g = gen.linear_chain(100)
        if name != "linear100":
            assert name == "linear100:weighted"
            recs["weight"] = np.random.default_rng(78).uniform(0.5, 2.0, len(recs))
        return recs, g
    if name.startswith("sketch"):
        return gen.connected_sketch(int(name[6:]), 1000 + int(name[6:]))
    return gen.graph_sketch(name, 50, np.random.default_rng(21))


CORNER_FIXED = 8  # the corner's records: 8 Fixed, then the three constraints whose guards fire


def corner(n):
    """A component of its own on the variables n .. n + 7: four points Q1, Q2, P, D, every coordinate held by a Fixed, Q1 == Q2
    exactly -- a line of length zero, an arc of radius zero -- and three constraints with a parameter on them whose residual's
    guard fires there: VerticalPointLineDistance, LinesAtAngle, ArcLength.  (No PointLineDistance: the oracle's Jacobian of it
    is NaN without a degenerate flag at a line of length zero.)  Returns the records and the Fixed values."""
    Q1, Q2, P, D = [(n + 2 * i, n + 2 * i + 1) for i in range(4)]
    vals = np.asarray([1.0, 2.0, 1.0, 2.0, 3.0, 2.5, 4.0, 4.0])
    cons = [O.fixed(n + i, float(v)) for i, v in enumerate(vals)]
    cons += [O.vertical_point_line_distance(P, Q1, Q2, 1.0, weight=1.5), O.lines_at_angle(Q1, Q2, P, D, ("deg", 30.0), weight=0.7),
             O.arc_length(Q1, Q2, P, 2.0)]
    return O.stack(cons), vals


def driven(recs):
    return np.asarray([i for i in range(len(recs)) if R.has_param(recs[i])], dtype=np.uint32)


_SYSTEMS = {}


def system(name, batch=2, pick=None):
    """name -> dict(recs, n_vars, pos, params [B, k], x [B, n] (the oracle's answers), lam): every constraint with a parameter
    listed (pick: a function of that list), draws of default_rng(33): parameters +-1e-3, starts +-0.02."""
    key = (name, batch, None if pick is None else pick.__name__)
    if key not in _SYSTEMS and name == "mixed40:double":
        # mixed40:unit at the same values with every weight 2.0 and 4 x lambda: J and g scaled by 2, JtJ + lam I and Jt g by 4
        _SYSTEMS[key] = dict(system("mixed40:unit", batch, pick), recs=inputs(name)[0], lam=4.0 * LAM)
    if key not in _SYSTEMS and name == "mixed40+corner":
        # mixed40's own draw; the corner's three constraints listed after the others (not its Fixed), its variables at the
        # Fixed values themselves
        assert pick is None
        base, (recs, g) = system("mixed40", batch), inputs(name)
        n_base, n = len(base["recs"]), base["n_vars"]
        first = n_base + CORNER_FIXED
        pos = np.concatenate([base["pos"], np.arange(first, len(recs), dtype=np.uint32)])
        own = recs["param"][first:][None, :] + np.random.default_rng(34).uniform(-1e-3, 1e-3, (batch, len(recs) - first))
        tail = np.repeat(g[None, n:], batch, axis=0)
        _SYSTEMS[key] = dict(recs=recs, n_vars=len(g), pos=pos, params=np.concatenate([base["params"], own], axis=1),
                             x=np.concatenate([base["x"], tail], axis=1), lam=LAM, start=np.concatenate([base["start"], tail], axis=1))
    if key not in _SYSTEMS:
        recs, g = inputs(name)
        rng = np.random.default_rng(33)
        pos = driven(recs)
        if pick is not None:
            pos = pick(pos)
        params = recs["param"][pos][None, :] + rng.uniform(-1e-3, 1e-3, (batch, len(pos)))
        x0 = g[None, :] + rng.uniform(-0.02, 0.02, (batch, len(g)))
        x = R._solved(recs, x0, pos, params)
        _SYSTEMS[key] = dict(recs=recs, n_vars=len(g), pos=pos, params=params, x=x, lam=LAM, start=x0)
    return _SYSTEMS[key]


_REFS = {}


def references(name, batch=2, pick=None):
    """[(S by Cholesky, spread)] per system (remembered)."""
    key = (name, batch, None if pick is None else pick.__name__)
    if key not in _REFS:
        s = system(name, batch, pick)
        _REFS[key] = [R.reference(s["recs"], s["n_vars"], s["x"][b], s["pos"], s["params"][b], s["lam"]) for b in range(batch)]
    return _REFS[key]


def two_row(recs, pos):
    """The places in `pos` of the listed constraints with two rows (ArcRadius, ArcLength, PointsAtAngle)."""
    return [j for j, p in enumerate(pos) if O.residual_dim(recs[int(p)]) == 2]


# kinds.hpp: kind_is_linear, in the oracle's numbering
LINEAR_KINDS = (O.FIXED, O.SCALAR_EQUAL, O.VERTICAL, O.HORIZONTAL, O.VERTICAL_DISTANCE, O.HORIZONTAL_DISTANCE, O.CIRCLE_RADIUS,
                O.POINTS_COINCIDENT, O.MIDPOINT)


def sixteen(pos):
    """16 listed positions spaced evenly over the driven constraints."""
    return pos[np.linspace(0, len(pos) - 1, 16).astype(int)]


class Tables:
    """The tables of a `positions` list for the plan front_ref.Plan(recs, n_vars, wgs) makes."""

    def __init__(self, recs, n_vars, wgs, positions, max_wgs=32, lds_bytes=160 * 1024):
        recs = np.ascontiguousarray(recs)
        pos = np.ascontiguousarray(positions, dtype=np.uint32)
        L = E.lib()
        info = np.zeros(4, np.uint64)
        args = (recs.ctypes.data, len(recs), n_vars, wgs, max_wgs, lds_bytes, pos.ctypes.data if len(pos) else None, len(pos))
        size = L.ezpz_debug_front_sens_tables(*args, None, 0, info.ctypes.data)
        assert size > 0, size
        self.w = np.zeros(size // 4, np.uint32)
        assert L.ezpz_debug_front_sens_tables(*args, self.w.ctypes.data, size, info.ctypes.data) == size
        self.n_wgs, self.n_param, self.w_home, n_words = [int(v) for v in self.w[:4]]
        assert n_words == len(self.w) == int(info[1]) and self.n_param == len(pos)

    def wg(self, g):
        w_asm_offs, asm_trips, w_ext, n_fronts = [int(v) for v in self.w[4 + 4 * g: 8 + 4 * g]]
        return w_asm_offs, asm_trips, w_ext, n_fronts

    def home(self, j):
        return int(self.w[self.w_home + 2 * j]), int(self.w[self.w_home + 2 * j + 1])


class Executor:
    """One system at x: factorise once, then one right-hand side after the other."""

    def __init__(self, plan, tables, x_caller, lam):
        self.plan, self.T, self.x, self.lam = plan, tables, np.asarray(x_caller, dtype=np.float64), lam
        G = plan.n_wgs
        assert tables.n_wgs == G
        self.ws = [np.zeros(int(plan.wgs[g]["ws_doubles"])) for g in range(G)]
        self.evals = [F.evaluate(plan, g, self.x) for g in range(G)]
        self.rn = [np.zeros(int(plan.wgs[g]["n_rows"]) + 1) for g in range(G)]  # the residual-space vector: all zero between passes
        self.chunks = {}
        self.bad = False
        for g in list(range(1, G)) + [0]:
            self._factor(g)

    def _stream(self, g):
        W = self.plan.wgs[g]
        t_end = int(W["t_cons"]) if int(W["t_cons"]) != 0xFFFFFFFF else int(W["tab_bytes"])
        return self.plan.arr("<u4", int(W["o_tables"]) + int(W["t_stream"]), (t_end - int(W["t_stream"])) // 4)

    def _factor(self, g):
        """front_ref.linear_step's factorisation with r = 0 (the rhs rows come out as zeros and are not used)."""
        plan, w = self.plan, self.ws[g]
        W = plan.wgs[g]
        descs, level_ptr, children, rows, exports, maps = plan.wg_tables(g)
        _, jv = self.evals[g]
        stream = self._stream(g)
        pan = int(W["l_panels"])
        w[pan:] = 0.0
        offs = stream[int(W["asm_word0"]): int(W["asm_word0"]) + int(W["asm_trips"])]
        for tr in range(int(W["asm_trips"])):
            base = int(offs[tr])
            wdt = int(stream[base]) >> 24
            for l in range(64):
                hdr = int(stream[base + l])
                if hdr & FASM_NOP:
                    continue
                acc = 0.0
                if not hdr & FASM_RHS:
                    for q in range(wdt):
                        op = int(stream[base + 64 * (1 + q) + l])
                        acc += jv[op & 0xFFFF] * jv[op >> 16]
                if hdr & F.FASM_DIAG:
                    acc += self.lam
                w[pan + (hdr & 0xFFFF)] = acc
        for lv in range(int(W["n_levels"])):
            for k in range(int(level_ptr[lv]), int(level_ptr[lv + 1])):
                d = descs[k]
                K, S = int(d["K"]), int(d["S"])
                S1, Rr = S + 1, S - K
                nU = (Rr + 1) * (Rr + 2) // 2
                P = w[int(d["panel"]): int(d["panel"]) + S1 * K]
                U = w[int(d["upd"]): int(d["upd"]) + nU] if Rr else w[0:0]
                base = int(d["src_off"])
                n_e = int(d["src_n"])
                for tr in range((n_e + 63) // 64):
                    vdt = int(d["src_v"][min(tr, 3)])
                    for l in range(64):
                        hdr = int(stream[base + l])
                        if hdr & FASM_NOP:
                            continue
                        acc = w[pan + (hdr & 0xFFFF)]
                        for q in range(vdt):
                            sw = int(stream[base + 64 * (1 + q) + l])
                            acc += w[pan + (sw & 0xFFFF)] + w[pan + (sw >> 16)]
                        w[pan + (hdr & 0xFFFF)] = acc
                    base += 64 * (1 + vdt)
                for c in children[int(d["child0"]): int(d["child0"]) + int(d["n_child"])]:
                    Rc1 = int(c["rows"])
                    m = maps[int(c["map"]): int(c["map"]) + Rc1]
                    for a in range(Rc1):
                        for b in range(a + 1):
                            e = tri(a, b)
                            if e == Rc1 * (Rc1 + 1) // 2 - 1:
                                continue
                            val = self.chunks[int(c["upd"]) + e]
                            i, j = int(m[a]), int(m[b])
                            if j < K:
                                P[j * S1 + i] += val
                            else:
                                U[tri(i - K, j - K)] += val
                A = P.reshape(K, S1).T.copy()
                for j in range(K):
                    piv = A[j, j]
                    if not piv > 0.0:
                        self.bad = True
                    with np.errstate(all="ignore"):
                        rinv = 1.0 / np.sqrt(piv)
                        lcol = A[:, j] * rinv
                    lcol[:j + 1] = 0.0
                    A[j + 1:, j] = lcol[j + 1:]
                    A[j, j] = rinv
                    for kk in range(j + 1, K):
                        A[kk:, kk] -= lcol[kk:] * lcol[kk]
                P[:] = A.T.reshape(-1)
                for a in range(Rr + 1):
                    for b in range(a + 1):
                        if a == Rr and b == Rr:
                            continue
                        acc = 0.0
                        for kk in range(K):
                            acc += P[kk * S1 + K + a] * P[kk * S1 + K + b]
                        U[tri(a, b)] -= acc
                if int(d["flags"]) & FRONT_REMOTE_PARENT:
                    for e in range(nU - 1):
                        self.chunks[int(d["up_chunk"]) + e] = U[e]

    def _forward(self, g):
        plan, w, T = self.plan, self.ws[g], self.T.w
        W = plan.wgs[g]
        descs, level_ptr, children, rows, exports, maps = plan.wg_tables(g)
        _, jv = self.evals[g]
        r = self.rn[g]
        pan = int(W["l_panels"])
        w_asm_offs, asm_trips, w_ext, n_fronts = self.T.wg(g)
        assert n_fronts == int(W["n_fronts"])
        # the rhs rows zeroed
        for d in descs:
            K, S = int(d["K"]), int(d["S"])
            S1, Rr = S + 1, S - K
            for c in range(K):
                w[int(d["panel"]) + c * S1 + S] = 0.0
            if Rr:
                for b in range(Rr + 1):
                    w[int(d["upd"]) + tri(Rr, b)] = 0.0
        # the rhs-only assembly stream
        for tr in range(asm_trips):
            base = int(T[w_asm_offs + tr])
            wdt = int(T[base]) >> 24
            for l in range(64):
                hdr = int(T[base + l])
                assert hdr >> 24 == wdt and hdr & FASM_RHS
                if hdr & FASM_NOP:
                    continue
                acc = 0.0
                for q in range(wdt):
                    op = int(T[base + 64 * (1 + q) + l])
                    acc += jv[op & 0xFFFF] * r[op >> 16]
                w[pan + (hdr & 0xFFFF)] = -acc
        for lv in range(int(W["n_levels"])):
            for k in range(int(level_ptr[lv]), int(level_ptr[lv + 1])):
                d = descs[k]
                K, S = int(d["K"]), int(d["S"])
                S1, Rr = S + 1, S - K
                o_p, o_u = int(d["panel"]), int(d["upd"])
                # rhs-only extend-add
                base, n_trips = int(T[w_ext + 2 * k]), int(T[w_ext + 2 * k + 1])
                for _ in range(n_trips):
                    vdt = int(T[base]) >> 24
                    for l in range(64):
                        hdr = int(T[base + l])
                        if hdr & FASM_NOP:
                            continue
                        dst = pan + (hdr & 0xFFFF)
                        assert dst in [o_p + c * S1 + S for c in range(K)] + [o_u + tri(Rr, b) for b in range(Rr)], "not a rhs row"
                        acc = w[dst]
                        for q in range(vdt):
                            sw = int(T[base + 64 * (1 + q) + l])
                            acc += w[pan + (sw & 0xFFFF)] + w[pan + (sw >> 16)]
                        w[dst] = acc
                    base += 64 * (1 + vdt)
                # remote children: the last rows of their update matrices
                for c in children[int(d["child0"]): int(d["child0"]) + int(d["n_child"])]:
                    last = int(c["rows"]) - 1
                    m = maps[int(c["map"]): int(c["map"]) + last + 1]
                    for b in range(last):
                        val = self.chunks[("rhs", int(c["upd"]) + tri(last, b))]
                        i, j = int(m[last]), int(m[b])
                        assert i == S
                        if j < K:
                            w[o_p + j * S1 + i] += val
                        else:
                            w[o_u + tri(i - K, j - K)] += val
                # row S against the panel
                y = np.zeros(K)
                for c in range(K):
                    t = w[o_p + c * S1 + S]
                    for j in range(c):
                        t -= w[o_p + j * S1 + c] * y[j]
                    y[c] = t * w[o_p + c * S1 + c]
                    w[o_p + c * S1 + S] = y[c]
                # the rows below
                for b in range(Rr):
                    acc = 0.0
                    for c in range(K):
                        acc += y[c] * w[o_p + c * S1 + K + b]
                    v = w[o_u + tri(Rr, b)] - acc
                    if int(d["flags"]) & FRONT_REMOTE_PARENT:
                        self.chunks[("rhs", int(d["up_chunk"]) + tri(Rr, b))] = v
                    else:
                        w[o_u + tri(Rr, b)] = v

    def _backward(self, g):
        plan, w = self.plan, self.ws[g]
        W = plan.wgs[g]
        descs, level_ptr, children, rows, exports, maps = plan.wg_tables(g)
        dv = w[int(W["l_d"]): int(W["l_d"]) + int(W["n_loc"])]
        for gh in plan.arr(F.FRONT_GHOST, W["o_ghosts"], int(W["n_ghost"])):
            dv[int(gh["local"])] = self.chunks[("step", int(gh["chunk"]))]
        for lv in reversed(range(int(W["n_levels"]))):
            for k in range(int(level_ptr[lv]), int(level_ptr[lv + 1])):
                d = descs[k]
                K, S = int(d["K"]), int(d["S"])
                S1 = S + 1
                P = w[int(d["panel"]): int(d["panel"]) + S1 * K]
                frow = rows[int(d["rows"]): int(d["rows"]) + S]
                t = np.array([P[kk * S1 + S] for kk in range(K)])
                for rr in range(K, S):
                    xr = dv[int(frow[rr])]
                    for kk in range(K):
                        t[kk] -= P[kk * S1 + rr] * xr
                xs = np.zeros(K)
                for j in reversed(range(K)):
                    xs[j] = t[j] * P[j * S1 + j]
                    for kk in range(j):
                        t[kk] -= P[kk * S1 + j] * xs[j]
                for kk in range(K):
                    dv[int(frow[kk])] = xs[kk]
                    if int(d["flags"]) & FRONT_EXPORTS and int(exports[int(d["exp0"]) + kk]) != 0xFFFFFFFF:
                        self.chunks[("step", int(exports[int(d["exp0"]) + kk]))] = xs[kk]

    def row(self, j, position):
        """S[j, :] in the caller's variable order."""
        plan = self.plan
        G = plan.n_wgs
        hw, hi = self.T.home(j)
        cons = plan.arr(F.DEVCON, plan.wgs[hw]["o_cons"], int(plan.wgs[hw]["n_cons"]))
        d = cons[hi]
        assert int(d["pos"]) == int(position), "the home table names another constraint"
        g, _ = E.constraint_param_derivative(plan.recs[int(position)], self.x)
        for k in range(len(g)):
            self.rn[hw][int(d["row0"]) + k] = g[k]
        self.chunks = {k: v for k, v in self.chunks.items() if not isinstance(k, tuple)}
        for wg in list(range(1, G)) + [0]:
            self._forward(wg)
        self.rn[hw][:] = 0.0
        for wg in range(G):
            self._backward(wg)
        out = np.zeros(plan.n_vars)
        for wg in range(G):
            W = plan.wgs[wg]
            vg = plan.arr("<u4", W["o_var_glob"], int(W["n_loc"]))
            dv = self.ws[wg][int(W["l_d"]): int(W["l_d"]) + int(W["n_loc"])]
            out[vg[:int(W["n_own"])]] = dv[:int(W["n_own"])]
        return out


def executed(recs, n_vars, wgs, positions, x, lam):
    """S [k, n_vars] of one system (recs with its parameters substituted) through the plan and the tables; the bad-pivot flag."""
    plan = F.Plan(recs, n_vars, wgs)
    assert plan.ok and plan.n_wgs == wgs, (plan.ok, wgs)
    ex = Executor(plan, Tables(recs, n_vars, wgs, positions), x, lam)
    return np.stack([ex.row(j, p) for j, p in enumerate(positions)]), ex.bad
