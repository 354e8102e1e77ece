// The component planner's HIP source text (see comp_classes.hpp, comp_program.hpp): the classes, the kernel entries, the lane and
// wavefront forms of a small system.  Plain C++17, no device code.
#include "comp_classes.hpp"
#include "policy.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <numeric>

namespace ezpz {

namespace {

// ---- source text of the class-specialised kernel (see jit_kernel.hip.hpp) ---------------------------------------------------------
// Every statement below is one operation of the class program, in the interpreter's order (comp_kernel.hip.hpp), with
// literal indices; doubles are written as hexadecimal floating literals (exact).
std::string hexf(double v) {
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%a", v);
    return std::string("(") + buf + ")";
}

// one line of a function body: the statements side by side
void line(std::string& o, std::initializer_list<std::string> statements) {
    o += "       ";
    for (const std::string& s : statements)
        if (!s.empty()) o += " " + s;
    o += "\n";
}

// The linear solve of a class (newton.rs:73-102) is ONE sequence of statements on the scalars D<v> (diagonal), V<v> (right-hand side,
// then y, then the step) and L<s> (strict lower entries), written by the two walkers below.  A caller asks for the statements of
// the factorisation (kFactor: what depends on lambda alone -- D, the reciprocals Y, L), of the right-hand side (kRhs: V, the two
// substitutions), or both; either part alone is the whole sequence with the other part's statements left out, so every quantity
// receives exactly the same operations in the same order whichever way it is computed.
enum SolvePart : unsigned { kFactor = 1, kRhs = 2 };

// D<v> = sum j^2 + lambda, V<v> = sum j * -r, L<s> = sum j_a * j_b from the class program's lists (Jacobian values: the constants of
// a linear class, else J[])
void emit_assembly(std::string& o, const Class& cl, unsigned parts) {
    const Program& Q = cl.Q;
    const bool fac = parts & kFactor, rhs = parts & kRhs;
    auto jv = [&](uint32_t slot) { return cl.linear ? hexf(cl.jconst[slot]) : "J[" + S(slot) + "]"; };
    for (uint32_t v = 0; v < Q.c.n_vars; ++v) {
        const std::string D = "D" + S(v), V = "V" + S(v);
        o += "        double " + (fac ? D + " = 0.0" : "") + (fac && rhs ? ", " : "") + (rhs ? V + " = 0.0" : "") + ";\n";
        for (uint32_t q = Q.colj_ptr[v]; q < Q.colj_ptr[v + 1]; ++q) {
            const std::string j = jv(Q.colj_items[2 * q]);
            line(o, {fac ? D + " += " + j + " * " + j + ";" : "", rhs ? V + " += " + j + " * -r[" + S(Q.colj_items[2 * q + 1]) + "];" : ""});
        }
        if (fac) line(o, {D + " = " + D + " + lambda;"});
    }
    for (uint32_t s = 0; s < Q.c.zlo && fac; ++s) {
        line(o, {"double L" + S(s) + " = 0.0;"});
        for (uint32_t q = Q.apair_ptr[s]; q < Q.apair_ptr[s + 1]; ++q)
            line(o, {"L" + S(s) + " += " + jv(Q.apairs[2 * q]) + " * " + jv(Q.apairs[2 * q + 1]) + ";"});
    }
}

// The elimination on the assembled scalars: level by level the left-looking Cholesky with the forward substitution riding along,
// then the backward substitution into d[] and dmax -- the same statements in `solve` / `factor` + `solve_f` of a class and in the
// wavefront kernel's `tail`.  `recip`: divisions by a column's diagonal through its refined reciprocal Y<v> (jit_kernel.hip.hpp:
// recip_of / div_by).  `store_f` (the factorisation alone): D, Y and L also go into F -- D<v> at 2 v, Y<v> at 2 v + 1, L<s> at 2 NV + s.
void emit_elimination(std::string& o, const Class& cl, unsigned parts, bool recip, bool store_f) {
    const Program& Q = cl.Q;
    const bool fac = parts & kFactor, rhs = parts & kRhs;
    const uint32_t nv = Q.c.n_vars;
    auto div = [&](const std::string& num, uint32_t col) {
        return num + " = " + (recip ? "ezpz::jit::div_by(" + num + ", D" + S(col) + ", Y" + S(col) + ", ok)" : num + " / D" + S(col)) + ";";
    };
    const PartDesc part = Q.parts.empty() ? PartDesc{0, 0, 0, 0} : Q.parts[0];
    for (uint32_t lv = 0; lv < part.nlev; ++lv) {
        const uint32_t c0 = Q.lvl_cptr[part.lvl0 + lv], c1 = Q.lvl_cptr[part.lvl0 + lv + 1];
        const uint32_t s0 = Q.lvl_sptr[part.lvl0 + lv], s1 = Q.lvl_sptr[part.lvl0 + lv + 1];
        for (uint32_t v = c0; v < c1; ++v) {
            const std::string D = "D" + S(v), V = "V" + S(v), Y = "Y" + S(v);
            for (uint32_t q = Q.fwd_ptr[v]; q < Q.fwd_ptr[v + 1]; ++q) {
                const std::string l = "L" + S(Q.fwd_items[2 * q]);
                line(o, {fac ? D + " -= " + l + " * " + l + ";" : "", rhs ? V + " -= " + l + " * V" + S(Q.fwd_items[2 * q + 1]) + ";" : ""});
            }
            if (fac) line(o, {"if (!(" + D + " > 0.0)) bad = true;"});
            line(o, {fac ? D + " = sqrt(" + D + ");" : "",
                     fac && recip ? "const double " + Y + " = ezpz::jit::recip_of(" + D + ", ok);" : fac && store_f ? "const double " + Y + " = 0.0;" : "",
                     store_f ? "F[" + S(2 * v) + "] = " + D + "; F[" + S(2 * v + 1) + "] = " + Y + ";" : "", rhs ? div(V, v) : ""});
        }
        for (uint32_t s = s0; s < s1 && fac; ++s) {
            const std::string L = "L" + S(s);
            for (uint32_t q = Q.lpair_ptr[s]; q < Q.lpair_ptr[s + 1]; ++q) line(o, {L + " -= L" + S(Q.lpairs[2 * q]) + " * L" + S(Q.lpairs[2 * q + 1]) + ";"});
            line(o, {div(L, Q.l_col[s]), store_f ? "F[" + S(2 * nv + s) + "] = " + L + ";" : ""});
        }
    }
    for (uint32_t lv = part.nlev; lv-- > 0 && rhs;) {
        const uint32_t c0 = Q.lvl_cptr[part.lvl0 + lv], c1 = Q.lvl_cptr[part.lvl0 + lv + 1];
        for (uint32_t v = c0; v < c1; ++v) {
            const std::string V = "V" + S(v);
            for (uint32_t q = Q.bwd_ptr[v]; q < Q.bwd_ptr[v + 1]; ++q) line(o, {V + " -= L" + S(Q.bwd_items[2 * q]) + " * V" + S(Q.bwd_items[2 * q + 1]) + ";"});
            line(o, {div(V, v), "d[" + S(v) + "] = " + V + ";", "dmax = ezpz::dev::fmax_abs(dmax, " + V + ");"});
        }
    }
}

// EZPZ_JIT_FASTDIV (measurements): bit 0 linear classes, bit 1 non-linear classes of the component kernels, bit 2 the
// lane-per-system kernels get the shared-reciprocal division (jit_kernel.hip.hpp: recip_of / div_by); the others divide plainly.
unsigned fastdiv_mask() {
    static const unsigned mask = [] {
        const char* e = std::getenv("EZPZ_JIT_FASTDIV");
        return e ? (unsigned)std::atoi(e) : 3u;  // (lane kernels: per-lane reciprocals cost `square` its second wavefront per SIMD, 1148 -> 1008 M solves/s)
    }();
    return mask;
}

// `lane`: the class is a whole system solved by one lane (jit_kernel.hip.hpp, lane_kernel): constraint parameters and
// the caller's constraint positions are literals, and load / store / pos_of map the caller's numbering.
void emit_class(std::string& o, size_t k, const Class& cl, bool lane = false, const EzpzConstraint* cs = nullptr) {
    const bool fastdiv = (fastdiv_mask() >> (lane ? 2 : cl.linear ? 0 : 1)) & 1u;
    const Program& Q = cl.Q;
    const uint32_t nv = Q.c.n_vars, m = Q.c.n_rows, zj = Q.c.zj, zlo = Q.c.zlo, nc = Q.c.n_cons;
    const bool lin = cl.linear;
    auto con_expr = [&](const DevCon& d, uint32_t ci) {
        std::string e = "ezpz::jit::mkcon(" + S(d.kind) + ", " + S(d.tag) + ", " + S(d.nrows);
        for (int i = 0; i < 8; ++i) e += ", " + S(d.ids[i]);
        e += ", " + hexf(d.weight) + ", " + (lane ? hexf(cs[d.pos].param) : "par[" + S(ci) + "]") + ")";
        return e;
    };
    o += "struct Cls" + S(k) + " {\n";
    o += "    static constexpr int NV = " + S(nv) + ", M = " + S(m) + ", NC = " + S(nc) + ", ZJS = " + S(lin ? 0 : zj) +
         ", STRIDE = " + S(cl.H.ninst_pad) + ";\n";
    o += std::string("    static constexpr bool LINEAR = ") + (lin ? "true" : "false") + ";\n";
    const std::string xs = "const double (&x)[" + S(nv) + "], const double (&par)[" + S(std::max(nc, 1u)) + "]";
    // residual sweep (solver.rs:318-356): r = weight * residual, sum of squares, maximum, degenerate mask
    o += "    static __device__ __forceinline__ void residuals(" + xs + ", double (&r)[" + S(std::max(m, 1u)) +
         "], bool active, double& sq, double& mx, unsigned long long& wm) {\n";
    // (one lane per system: in request order, so that the sum of squares is formed exactly like the reference's
    // sequential sum over the rows -- the accept test `sum < previous` of a stalled solve hinges on its last bit)
    std::vector<uint32_t> sweep(nc);
    std::iota(sweep.begin(), sweep.end(), 0u);
    if (lane) std::sort(sweep.begin(), sweep.end(), [&](uint32_t a, uint32_t b) { return Q.cons[a].pos < Q.cons[b].pos; });
    for (uint32_t ci : sweep) {
        const DevCon& d = Q.cons[ci];
        o += "        { const DevCon c = " + con_expr(d, ci) + "; double r0, r1; const bool deg = ezpz::dev::con_residual<LINEAR>(c, x, r0, r1);\n";
        o += "          const double w0 = c.weight * r0; r[" + S(d.row0) + "] = w0; if (active) { sq += w0 * w0; mx = ezpz::dev::fmax_abs(mx, w0); }\n";
        if (d.nrows > 1)
            o += "          const double w1 = c.weight * r1; r[" + S(d.row0 + 1) + "] = w1; if (active) { sq += w1 * w1; mx = ezpz::dev::fmax_abs(mx, w1); }\n";
        o += "          if (!LINEAR && deg) wm |= 1ull << " + S(ci) + "; (void)r1; }\n";
    }
    o += "        (void)x; (void)par; (void)r; (void)active; (void)sq; (void)mx; (void)wm;\n    }\n";
    // Jacobian sweep (solver.rs:359-440)
    o += "    static __device__ __forceinline__ void jacobian(" + xs + ", double (&J)[" + S(lin ? 1u : std::max(zj, 1u)) +
         "], unsigned long long& wm) {\n";
    if (!lin)
        for (uint32_t ci = 0; ci < nc; ++ci) {
            const DevCon& d = Q.cons[ci];
            uint32_t loc[4];
            std::memcpy(loc, d.jloc, 16);
            o += "        { const DevCon c = " + con_expr(d, ci) + "; ezpz::dev::JacWriter<double*> w; w.jv = J; w.jbase = " + S(d.jbase) +
                 "; w.loc[0] = " + S(loc[0]) + "u; w.loc[1] = " + S(loc[1]) + "u; w.loc[2] = " + S(loc[2]) + "u; w.loc[3] = " + S(loc[3]) +
                 "u; w.weight = c.weight;\n";
            o += "          if (ezpz::dev::con_jacobian<false>(c, x, w)) wm |= 1ull << " + S(ci) + "; }\n";
        }
    o += "        (void)x; (void)par; (void)J; (void)wm;\n    }\n";
    // the linear solve (newton.rs:73-102), twice: `solve` divides by a column's diagonal through the column's refined
    // reciprocal (jit_kernel.hip.hpp: recip_of / div_by -- the tail of the compiler's own division sequence, exact while
    // no operand needs scaling; `ok` says whether every operand was in that range), `solve_exact` is the same
    // statements with plain divisions and serves the lanes whose `ok` came back false
    for (int fast = 1; fast >= 0; --fast) {
        o += std::string("    static __device__ __forceinline__ bool ") + (fast ? "solve" : "solve_exact") + "(const double (&J)[" +
             S(lin ? 1u : std::max(zj, 1u)) + "], const double (&r)[" + S(std::max(m, 1u)) + "], double lambda, double (&d)[" + S(nv) +
             "], double& dmax" + (fast ? ", bool& ok" : "") + ") {\n        bool bad = false;\n";
        emit_assembly(o, cl, kFactor | kRhs);
        emit_elimination(o, cl, kFactor | kRhs, fast && fastdiv, false);
        o += std::string("        (void)J; (void)r;") + (fast ? " (void)ok;" : "") + "\n        return bad;\n    }\n";
    }
    // A linear class's matrix J^T J + lambda I is the same for every instance and every system: `factor` is the part of `solve` that
    // depends on lambda alone (diagonals, their refined reciprocals, the entries of L), `solve_f` the rest (right-hand side, the
    // two substitutions) on a factorisation the caller keeps -- in scalar registers, once per lambda and launch
    // (jit_kernel.hip.hpp: solve_kernel_grid_fast).  The two are `solve`'s statements dealt out by the same walkers (SolvePart).
    // F: D<v> at 2 v, Y<v> at 2 v + 1, L<s> at 2 NV + s.
    o += "    static constexpr int NF = " + S(lin && !lane ? 2 * nv + zlo : 1) + ";\n";
    if (lin && !lane) {
        o += "    static __device__ __forceinline__ bool factor(double lambda, double (&F)[NF], bool& ok) {\n        bool bad = false;\n";
        emit_assembly(o, cl, kFactor);
        emit_elimination(o, cl, kFactor, fastdiv, true);
        o += "        (void)ok;\n        return bad;\n    }\n";
        // (OK: what div_by folds its range test into -- jit_kernel.hip.hpp: DivRange)
        o += "    template <class OK> static __device__ __forceinline__ void solve_f(const double (&F)[NF], const double (&r)[" + S(std::max(m, 1u)) + "], double (&d)[" + S(nv) +
             "], double& dmax, OK& ok) {\n";
        for (uint32_t v = 0; v < nv; ++v) o += "        const double D" + S(v) + " = F[" + S(2 * v) + "], Y" + S(v) + " = F[" + S(2 * v + 1) + "]; (void)Y" + S(v) + ";\n";
        for (uint32_t s2 = 0; s2 < zlo; ++s2) o += "        const double L" + S(s2) + " = F[" + S(2 * nv + s2) + "];\n";
        emit_assembly(o, cl, kRhs);
        emit_elimination(o, cl, kRhs, fastdiv, false);
        o += "        (void)r; (void)ok;\n    }\n";
    }
    // unsatisfied check (lib.rs:305-327, :358-370)
    o += "    static __device__ __forceinline__ void unsatisfied(" + xs + ", bool active, double& unsat, uint8_t* mask, const uint32_t* pos) {\n";
    for (uint32_t ci = 0; ci < nc; ++ci) {
        const DevCon& d = Q.cons[ci];
        o += "        { const DevCon c = " + con_expr(d, ci) + "; double r0, r1; ezpz::dev::con_residual<LINEAR>(c, x, r0, r1);\n";
        o += std::string("          bool sat = fabs(r0) < ezpz::dev::EPS;") + (d.nrows > 1 ? " sat = sat && (fabs(r1) < ezpz::dev::EPS);" : "") + "\n";
        o += "          if (active) { if (!sat) unsat += 1.0; if (mask) mask[" + (lane ? S(d.pos) : "pos[(size_t)" + S(ci) + " * STRIDE]") + "] = sat ? 0 : 1; } (void)r1; }\n";
    }
    o += "        (void)x; (void)par; (void)active; (void)unsat; (void)mask; (void)pos;\n    }\n";
    o += "    static __device__ __forceinline__ void unsatisfied_from_r(const double (&r)[" + S(std::max(m, 1u)) +
         "], bool active, double& unsat, uint8_t* mask, const uint32_t* pos) {\n";
    for (uint32_t ci = 0; ci < nc; ++ci) {
        const DevCon& d = Q.cons[ci];
        o += "        { bool sat = fabs(r[" + S(d.row0) + "]) < ezpz::dev::EPS;" +
             (d.nrows > 1 ? " sat = sat && (fabs(r[" + S(d.row0 + 1) + "]) < ezpz::dev::EPS);" : "") + "\n";
        o += "          if (active) { if (!sat) unsat += 1.0; if (mask) mask[" + (lane ? S(d.pos) : "pos[(size_t)" + S(ci) + " * STRIDE]") + "] = sat ? 0 : 1; } }\n";
    }
    o += "        (void)r; (void)active; (void)unsat; (void)mask; (void)pos;\n    }\n";
    if (lane) {  // the caller's numbering: variables (row of x0 / x_out) and constraint positions
        o += "    static __device__ __forceinline__ void load(const double* row, double (&x)[" + S(nv) + "]) {\n       ";
        for (uint32_t v = 0; v < nv; ++v) o += " x[" + S(v) + "] = row[" + S(Q.var_of[v]) + "];";
        o += "\n    }\n    static __device__ __forceinline__ void store(double* row, const double (&x)[" + S(nv) + "]) {\n       ";
        for (uint32_t v = 0; v < nv; ++v) o += " row[" + S(Q.var_of[v]) + "] = x[" + S(v) + "];";
        o += "\n    }\n    static __device__ __forceinline__ uint32_t pos_of(int ci) {\n        switch (ci) {\n";
        for (uint32_t ci = 0; ci < nc; ++ci) o += "        case " + S(ci) + ": return " + S(Q.cons[ci].pos) + ";\n";
        o += "        default: return 0;\n        }\n    }\n";
    }
    o += "};\n\n";
}

const char* tf(bool b) { return b ? "true" : "false"; }

const char kPreamble[] = "#include \"jit_kernel.hip.hpp\"\nusing ezpz::DevCon;\n\n";

}  // namespace

// ---- the kernel of a component plan: a wavefront runs `shape.slots_k[k]` slots of every class k -------------------------------------
std::string comp_kernel_source(const std::vector<Class>& classes, const CompKernelShape& shape) {
    const uint32_t T = shape.waves, G = shape.wgs;
    std::string o = kPreamble;
    for (size_t k = 0; k < classes.size(); ++k) emit_class(o, k, classes[k]);
    std::string seq;
    for (size_t k = 0; k < classes.size(); ++k)
        for (uint32_t j = 0; j < shape.slots_k[k]; ++j) seq += (seq.empty() ? "Cls" : ", Cls") + S(k);
    bool any_nonlinear = false;
    for (const Class& cl : classes) any_nonlinear = any_nonlinear || !cl.linear;
    static const char* env_mw = std::getenv("EZPZ_JIT_MINWAVES");  // occupancy hint (waves per SIMD), for measurements
    // (the slots' state + ~40 working registers: with the matching occupancy as a hint the compiler spends the
    // whole register budget of that occupancy on scheduling -- 2000 x 2000: 66.9 -> 74.2 M solves/s at 3; a hint
    // the state does not fit costs spills: 2400 x 2400 at 3 instead of 2: 53 -> 43)
    const int min_waves = env_mw ? std::atoi(env_mw) : (int)std::min<uint64_t>(4, std::max<uint64_t>(1, 512 / (shape.vgprs + 50)));
    const std::string bounds = S(T * 64) + (min_waves > 0 ? ", " + std::to_string(min_waves) : "");
    // eval()'s sums riding in the first iteration's rendezvous (jit_kernel.hip.hpp: FUSE) -- one rendezvous less per system.
    // Measured on one box, 65 536 systems per launch, once the kernels of one-workgroup systems carried no grid code:
    // 2000 x 2000 (four wavefronts per system, three per SIMD) 96.0 -> 101.9 M solves/s, 800 x 800 (two, three) 195.8 ->
    // 214.2, 2400 x 2400 (four, two per SIMD: eight slots per lane) 65.3 -> 60.1, the over-constrained variant (non-linear
    // classes) 24.8 -> 23.8: taken for linear systems compiled for three or more wavefronts per SIMD;
    // One workgroup per system only.
    const bool fuse = !any_nonlinear && min_waves >= 3;
    const std::string slots = "<ezpz::jit::Slots<" + seq + ">, " + S(T);
    // two entries: batches, and (`_one`) one-call launches that stay resident for the caller's next request
    for (int one = 0; one < 2; ++one) {
        o += "extern \"C\" __global__ void __launch_bounds__(" + bounds + ") ezpz_jit_solve" + (one ? "_one" : "") + "(const ezpz::jit::JitArgs a) {\n";
        o += "    __shared__ double smem[ezpz::jit::kRedDoubles + 16];\n";
        if (G > 1)  // a system on several workgroups: the kernel with the reductions' grid stage (jit_kernel.hip.hpp: solve_kernel_grid)
            o += "    ezpz::jit::solve_kernel_grid" + slots + ", " + tf(any_nonlinear) + ", " + tf(shape.unit_weights) + ", " + tf(one) + ">(a, smem);\n}\n";
        else
            o += "    ezpz::jit::solve_kernel" + slots + ", " + tf(any_nonlinear) + ", " + tf(shape.unit_weights) + ", " + tf(one) + ", " + tf(fuse) + ", false>(a, smem);\n}\n";
    }
    // a LINEAR system with unit weights: the kernel that does not wait for the verdicts of the LM control (jit_kernel.hip.hpp:
    // solve_kernel_fast / solve_kernel_grid_fast) and, for a system on one workgroup, the loop over the systems that kernel
    // lists (`_list`; several workgroups: the first entry reads the list itself).  The first needs far fewer registers than the
    // loop: compiled for four wavefronts per SIMD while its state fits
    if (any_nonlinear || !shape.unit_weights) return o;
    uint64_t fast_vg = 0;  // the next system's x, parameters (doubles), ids; one slot's x, d, r; the eight partials
    uint64_t widest = 0;
    for (size_t k = 0; k < classes.size(); ++k) {
        const ClassLayout& H = classes[k].H;
        fast_vg += (2ull * (H.nv + H.ncons) + H.nv) * shape.slots_k[k];
        widest = std::max<uint64_t>(widest, 2ull * (2 * H.nv + H.m));
    }
    fast_vg += widest + 16;
    static const char* env_fw = std::getenv("EZPZ_JIT_FAST_MINWAVES");  // occupancy hint, for measurements
    // (several workgroups per system: the variant with a wavefront per SIMD less has the registers to let the values wait in
    // LDS for stores that go out back to back; EZPZ_JIT_GRID_STAGE=0: slot by slot there too, for measurements)
    static const int grid_stage = [] {
        const char* e = std::getenv("EZPZ_JIT_GRID_STAGE");
        return e ? std::atoi(e) : 1;  // (2 = its piece of the row as whole lines where contiguous: measured 2-6 % slower on the ladder)
    }();
    const int fast_waves = env_fw ? std::atoi(env_fw) : (fast_vg + 40 <= 128 ? 4 : fast_vg + 40 <= 168 ? 3 : 2);
    // Every wavefront's variables one contiguous run: the one-workgroup kernel moves a wavefront's piece of a row as full lines
    // (jit_kernel.hip.hpp: fast_wave, IO 2) -- for systems of four wavefronts or more: same box, previous build / this one, M solves/s:
    // 2000 x 2000 134.8 -> 142.0, 2400 x 2400 113.1 -> 111.5, but 800 x 800 (two wavefronts per system) 289 -> 274; and not for a
    // system on several workgroups (the ladder, same box: 256 systems per launch 0.93 -> 0.99 M, but the 64-system launches of the
    // bench leg 0.87 -> 0.81 M: the first system's piece goes through LDS before anything starts)
    const bool lines = shape.contiguous && T >= 4;
    // (twice: for the estimated occupancy and for one wavefront per SIMD less -- the loader takes the first that keeps its
    // registers out of scratch memory, jit.cpp: ensure_loaded)
    for (int variant = 0; variant < (fast_waves > 2 && !env_fw ? 2 : 1); ++variant) {
        o += "extern \"C\" __global__ void __launch_bounds__(" + S(T * 64) + ", " + std::to_string(fast_waves - variant) +
             ") ezpz_jit_solve_fast" + (variant ? "_b" : "") + "(const ezpz::jit::JitArgs a) {\n";
        o += std::string("    ezpz::jit::") + (G > 1 ? "solve_kernel_grid_fast" : "solve_kernel_fast") + slots +
             (G > 1 ? (variant && grid_stage ? (grid_stage >= 2 && lines ? ", 2" : ", 1") : ", 0") : lines ? ", true" : ", false") + ">(a);\n}\n";
    }
    if (G == 1) {
        o += "extern \"C\" __global__ void __launch_bounds__(" + bounds + ") ezpz_jit_solve_list(const ezpz::jit::JitArgs a) {\n";
        o += "    __shared__ double smem[ezpz::jit::kRedDoubles + 16];\n";
        o += "    ezpz::jit::solve_kernel_grid" + slots + ", false, true, false>(a, smem);\n}\n";
    }
    return o;
}

// ---- one lane per system (jit_kernel.hip.hpp, lane_kernel) --------------------------------------------------------------------------
std::string lane_class_source(const Class& cl, const EzpzConstraint* cs) {
    std::string cls = kPreamble;
    emit_class(cls, 0, cl, true, cs);
    return cls;
}

std::string lane_kernel_source(const std::string& cls, bool unit_weights) {
    std::string o = cls;
    for (int one = 0; one < 2; ++one) {  // (batches; `_one`: one-call launches that stay resident, jit_kernel.hip.hpp)
        o += std::string("extern \"C\" __global__ void __launch_bounds__(256) ezpz_jit_lane") + (one ? "_one" : "") + "(const ezpz::jit::LaneArgs a) {\n";
        o += std::string("    ezpz::jit::lane_kernel<Cls0, ") + tf(unit_weights) + ", " + tf(one) + ">(a);\n}\n";
    }
    return o;
}

namespace {

// The elimination of the wavefront kernel ACROSS its lanes (`tail_wave`): lane i holds row i of L (its entries a<k> = L(i, k),
// its diagonal and its right-hand side), columns are eliminated right-looking in the class program's order -- the pivot's
// square root and the column's division once per column instead of once per entry, the update of the later columns one
// multiply-subtract per column pair on all lanes at once, operands of other lanes through v_readlane -- and the backward
// substitution walks every column's entries in the serial order.  Every entry receives exactly the operations of `tail`
// (emit_elimination) in the same order -- the columns are taken in an order that respects every list of the class program
// (a row's updates, an entry's updates), the backward sums follow their lists;
// entries that are structurally zero hold zeros and receive multiples of zero -- so the step is the same bits
// (tests/test_gpu_lanes.py) as long as those multiples ARE zero: a right-hand side that is not finite (a NaN guess, an
// overflow) would turn 0 x y_k into NaN on rows the serial order never touches, so `fin` reports whether every y_k was
// finite and the kernel repeats the solve with the serial `tail` when not (pivots never see the right-hand side: `bad` is
// the same either way; a non-finite entry of L fails its row's pivot in both orders).  wave_row_structure checks what that rests on (lists complete and compatible with one column order, fill closed) and the serial
// `tail` stays when it does not hold.
struct WaveRows {
    bool ok = false;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> col;  // per column k: (row i, slot) ascending in i
    std::vector<std::vector<uint32_t>> bwd;                         // per column k: its rows in the backward sum's order
    std::vector<uint32_t> order;                                    // the columns in elimination order
    std::vector<uint32_t> slot_row;
};
WaveRows wave_row_structure(const Class& cl) {
    WaveRows w;
    auto why = [&](int code) {
        static const bool dbg = debug_topic("jit");
        if (dbg) std::fprintf(stderr, "[ezpz jit] wave: elimination across lanes not used (check %d)\n", code);
        return w;
    };
    const Program& Q = cl.Q;
    const uint32_t nv = Q.c.n_vars, zlo = Q.c.zlo;
    if (nv < 2 || nv > 64) return why(1);
    w.col.assign(nv, {});
    w.slot_row.assign(zlo, ~0u);
    std::vector<std::vector<uint32_t>> slot_of(nv, std::vector<uint32_t>(nv, ~0u));
    // edges of "column a is eliminated before column b": what fixes the order in which an entry receives its updates
    std::vector<std::vector<uint32_t>> after(nv);
    std::vector<uint32_t> waiting(nv, 0);
    auto before = [&](uint32_t x, uint32_t y) {
        after[x].push_back(y);
        ++waiting[y];
    };
    for (uint32_t j = 0; j < nv; ++j) {
        uint32_t last = ~0u;
        for (uint32_t q = Q.fwd_ptr[j]; q < Q.fwd_ptr[j + 1]; ++q) {
            const uint32_t slot = Q.fwd_items[2 * q], k = Q.fwd_items[2 * q + 1];
            if (slot >= zlo || k >= j || Q.l_col[slot] != k || slot_of[j][k] != ~0u) return why(2);
            // row j's diagonal and right-hand side take their updates in the list's order, then column j is eliminated
            if (last != ~0u) before(last, k);
            before(k, j);
            last = k;
            w.slot_row[slot] = j;
            slot_of[j][k] = slot;
        }
    }
    for (uint32_t s2 = 0; s2 < zlo; ++s2)
        if (w.slot_row[s2] == ~0u) return why(3);
    w.bwd.assign(nv, {});
    for (uint32_t k = 0; k < nv; ++k) {
        for (uint32_t i = k + 1; i < nv; ++i)
            if (slot_of[i][k] != ~0u) w.col[k].push_back({i, slot_of[i][k]});
        // backward list of column k: the same entries, in the order the serial sum takes them
        if (Q.bwd_ptr[k + 1] - Q.bwd_ptr[k] != w.col[k].size()) return why(4);
        for (uint32_t q = Q.bwd_ptr[k]; q < Q.bwd_ptr[k + 1]; ++q) {
            const uint32_t slot = Q.bwd_items[2 * q], i = Q.bwd_items[2 * q + 1];
            if (i >= nv || i <= k || slot_of[i][k] != slot) return why(5);
            w.bwd[k].push_back(i);
        }
    }
    // an entry's updates: one per earlier column in which both its row and its column have entries, in the list's order
    for (uint32_t s2 = 0; s2 < zlo; ++s2) {
        const uint32_t i = w.slot_row[s2], j = Q.l_col[s2];
        size_t want = 0;
        for (uint32_t k = 0; k < j; ++k) want += slot_of[i][k] != ~0u && slot_of[j][k] != ~0u;
        if (Q.lpair_ptr[s2 + 1] - Q.lpair_ptr[s2] != want) return why(6);
        uint32_t last = ~0u;
        for (uint32_t q = Q.lpair_ptr[s2]; q < Q.lpair_ptr[s2 + 1]; ++q) {
            const uint32_t sa = Q.lpairs[2 * q], sb = Q.lpairs[2 * q + 1];
            if (sa >= zlo || sb >= zlo) return why(7);
            const uint32_t k = Q.l_col[sa];
            if (k >= j || Q.l_col[sb] != k || slot_of[i][k] != sa || slot_of[j][k] != sb) return why(7);
            if (last != ~0u) before(last, k);
            last = k;
        }
    }
    // fill closed: two entries of a column imply the entry between their rows
    for (uint32_t k = 0; k < nv; ++k)
        for (size_t x = 0; x < w.col[k].size(); ++x)
            for (size_t y = x + 1; y < w.col[k].size(); ++y)
                if (slot_of[w.col[k][y].first][w.col[k][x].first] == ~0u) return why(8);
    // one order of the columns that respects every list, taken in rounds (every column whose predecessors are all in earlier
    // rounds, ascending): the class program's own order when its lists ascend, and columns of different branches of the
    // elimination tree stay next to each other, which is what lets emit_tail_wave group their pivots
    std::vector<char> done(nv, 0);
    while (w.order.size() < nv) {
        std::vector<uint32_t> round;
        for (uint32_t v = 0; v < nv; ++v)
            if (!done[v] && waiting[v] == 0) round.push_back(v);
        if (round.empty()) return why(9);  // (lists that contradict each other: no such order)
        for (uint32_t v : round) {
            done[v] = 1;
            w.order.push_back(v);
        }
        for (uint32_t v : round)
            for (uint32_t y : after[v]) --waiting[y];
    }
    w.ok = true;
    return w;
}
void emit_wave_row_table(std::string& o, const Class& cl) {
    const WaveRows w = wave_row_structure(cl);
    if (!w.ok) return;
    const Program& Q = cl.Q;
    const uint32_t nv = Q.c.n_vars, nq = 2 * nv + Q.c.zlo;
    // kWaveRow[k * 64 + lane] = where lane's entry of column k sits among the assembled quantities (nq = a zero)
    o += "__device__ const uint16_t kWaveRow[" + S((nv - 1) * 64) + "] = {";
    for (uint32_t k = 0; k + 1 < nv; ++k)
        for (uint32_t l = 0; l < 64; ++l) {
            const uint32_t row = std::min(l, nv - 1);
            uint32_t at = nq;
            for (const auto& e : w.col[k])
                if (e.first == row) at = 2 * nv + e.second;
            o += ((k * 64 + l) % 32 == 0 ? "\n    " : " ") + S(at) + ",";
        }
    o += "\n};\n";
}
void emit_tail_wave(std::string& o, const Class& cl) {
    const WaveRows w = wave_row_structure(cl);
    if (!w.ok) {
        o += "    static constexpr bool HAS_TAIL_WAVE = false;\n    static constexpr int NROW = 1;\n";
        o += "    static __device__ __forceinline__ uint32_t row_slot(int, int) { return 0; }\n";
        o += "    static __device__ __forceinline__ bool tail_wave(const double*, double, const uint32_t (&)[1], int, double*, double&, bool&) { return false; }\n";
        return;
    }
    const uint32_t nv = cl.Q.c.n_vars;
    o += "    static constexpr bool HAS_TAIL_WAVE = true;\n    static constexpr int NROW = " + S(nv - 1) + ";\n";
    o += "    static __device__ __forceinline__ uint32_t row_slot(int k, int lane) { return kWaveRow[k * 64 + lane]; }\n";
    o += "    static __device__ __forceinline__ bool tail_wave(const double* Q, double lambda, const uint32_t (&rs)[" + S(nv - 1) +
         "], int lane, double* d, double& dmax, bool& fin) {\n        using ezpz::jit::lane_value;\n        bool bad = false;\n";
    o += "        const int me = lane < NV ? lane : NV - 1;\n        double Dm = Q[me] + lambda, Vm = Q[NV + me];\n";
    for (uint32_t k = 0; k + 1 < nv; ++k) o += "        double a" + S(k) + " = Q[rs[" + S(k) + "]];\n";
    // Updates are applied in w.order (what fixes every entry's rounding); a column's pivot, its square root and its divisions
    // only need the updates of ITS row to have been applied, so they are issued as early as that allows, together with the
    // other columns that are ready then: independent square-root / division chains next to each other instead of one after
    // the other (a sparse sketch's elimination tree is wide: 14 columns in 8 such groups for two rectangles).
    {
        const Program& Q = cl.Q;
        std::vector<char> pivoted(nv, 0), applied(nv, 0);
        auto ready = [&](uint32_t j) {
            for (uint32_t q = Q.fwd_ptr[j]; q < Q.fwd_ptr[j + 1]; ++q)
                if (!applied[Q.fwd_items[2 * q + 1]]) return false;
            return true;
        };
        size_t pos = 0;
        while (pos < w.order.size()) {
            std::vector<uint32_t> R;
            for (uint32_t j = 0; j < nv; ++j)
                if (!pivoted[j] && ready(j)) R.push_back(j);
            for (uint32_t k : R) o += "        const double P" + S(k) + " = lane_value(Dm, " + S(k) + "); if (!(P" + S(k) + " > 0.0)) bad = true;\n";
            for (uint32_t k : R) o += "        const double D" + S(k) + " = sqrt(P" + S(k) + ");\n";
            for (uint32_t k : R)
                o += "        const double Y" + S(k) + " = lane_value(Vm, " + S(k) + ") / D" + S(k) + "; fin = fin && __builtin_isfinite(Y" + S(k) + ");\n";
            for (uint32_t k : R) {
                pivoted[k] = 1;
                if (!w.col[k].empty()) o += "        a" + S(k) + " = a" + S(k) + " / D" + S(k) + ";\n";
            }
            while (pos < w.order.size() && pivoted[w.order[pos]]) {
                const uint32_t k = w.order[pos++];
                applied[k] = 1;
                if (w.col[k].empty()) continue;
                const std::string K = S(k);
                for (size_t x = 0; x + 1 < w.col[k].size(); ++x) {
                    const std::string J = S(w.col[k][x].first);
                    o += "        a" + J + " -= a" + K + " * lane_value(a" + K + ", " + J + ");\n";
                }
                o += "        Dm -= a" + K + " * a" + K + "; Vm -= a" + K + " * Y" + K + ";\n";
            }
        }
    }
    // backward substitution: a column as soon as the rows of its entries are known, the ready columns' sums and divisions
    // side by side (every sum in its list's order)
    {
        std::vector<char> known(nv, 0);
        uint32_t left = nv;
        while (left) {
            std::vector<uint32_t> G;
            for (uint32_t k = nv; k-- > 0;) {
                if (known[k]) continue;
                bool ok = true;
                for (uint32_t i : w.bwd[k]) ok = ok && known[i];
                if (ok) G.push_back(k);
            }
            for (uint32_t k : G) {
                o += "        double X" + S(k) + " = Y" + S(k) + ";\n";
                for (uint32_t i : w.bwd[k]) o += "        X" + S(k) + " -= lane_value(a" + S(k) + ", " + S(i) + ") * X" + S(i) + ";\n";
            }
            for (uint32_t k : G) {
                o += "        X" + S(k) + " = X" + S(k) + " / D" + S(k) + "; d[" + S(k) + "] = X" + S(k) + "; dmax = ezpz::dev::fmax_abs(dmax, X" + S(k) + ");\n";
                known[k] = 1;
                --left;
            }
        }
    }
    o += "        (void)Vm; (void)Dm;\n        return bad;\n    }\n";
}

}  // namespace

// ---- one wavefront per system (jit_kernel.hip.hpp, wave_kernel): the latency shape of a small system -------------------------------
// The lane class (same statements, same order) plus what spreads the sweeps and the assembly over 64 lanes: the constraint
// records as a table (lane ci evaluates constraint ci through a dispatch over the kinds present), the operand pairs of
// every assembled quantity -- D_v and V_v per variable, L_s per strict lower entry -- padded to the longest list (a padding
// pair multiplies the zero behind the Jacobian's slots), and the elimination as `tail` on the assembled quantities.
// Empty when a list is too long for a lane's registers (a hub variable of dozens of constraints): the lane kernel serves.
std::string wave_kernel_source(const std::string& cls, const Class& cl, const EzpzConstraint* cs, bool unit_weights) {
    const Program& Q = cl.Q;
    const uint32_t nv = Q.c.n_vars, m = Q.c.n_rows, zj = Q.c.zj, zlo = Q.c.zlo, nc = Q.c.n_cons;
    if (nc > 64 || m > 64 || nv > 64 || zj + 1 + m >= 0xFFFFu) return "";
    const uint32_t nq = 2 * nv + zlo, nqr = (nq + 63) / 64;
    // operand pairs (a | b << 16): indices into A = [J slots | 0 | -r rows]
    std::vector<std::vector<uint32_t>> pairs(nq);
    for (uint32_t v = 0; v < nv; ++v)
        for (uint32_t q = Q.colj_ptr[v]; q < Q.colj_ptr[v + 1]; ++q) {
            const uint32_t slot = Q.colj_items[2 * q], row = Q.colj_items[2 * q + 1];
            pairs[v].push_back(slot | (slot << 16));
            pairs[nv + v].push_back(slot | ((zj + 1 + row) << 16));
        }
    for (uint32_t s2 = 0; s2 < zlo; ++s2)
        for (uint32_t q = Q.apair_ptr[s2]; q < Q.apair_ptr[s2 + 1]; ++q) pairs[2 * nv + s2].push_back(Q.apairs[2 * q] | (Q.apairs[2 * q + 1] << 16));
    uint32_t pmax = 1;
    for (const auto& p : pairs) pmax = std::max<uint32_t>(pmax, (uint32_t)p.size());
    if (pmax > 16 || nqr > 3) return "";
    std::string o = cls;
    // tables
    o += "namespace {\n__device__ const ezpz::DevCon kWaveCons[" + S(nc) + "] = {\n";
    for (uint32_t ci = 0; ci < nc; ++ci) {
        const DevCon& d = Q.cons[ci];
        o += "    {{";
        for (int i = 0; i < 8; ++i) o += (i ? ", " : "") + S(d.ids[i]);
        o += "}, " + hexf(cs[d.pos].param) + ", " + hexf(d.weight) + ", " + S(d.row0) + ", " + S(d.jbase) + ", " + S(d.pos) + ", " + S(d.kind) +
             ", " + S(d.tag) + ", " + S(d.nrows) + ", " + S(d.nslots) + ", {";
        for (int i = 0; i < 16; ++i) o += (i ? ", " : "") + S(d.jloc[i]);
        o += "}},\n";
    }
    o += "};\n__device__ const uint32_t kWavePairs[" + S(nqr * pmax * 64) + "] = {";
    const uint32_t pad = zj | (zj << 16);
    for (uint32_t k = 0; k < nqr; ++k)
        for (uint32_t p = 0; p < pmax; ++p)
            for (uint32_t l = 0; l < 64; ++l) {
                const uint32_t q = k * 64 + l;
                o += (((k * pmax + p) * 64 + l) % 16 == 0 ? "\n    " : " ") + S(q < nq && p < pairs[q].size() ? pairs[q][p] : pad) + "u,";
            }
    o += "\n};\n";
    // rows in request order (constraints by position, their rows in order), the caller's id of every internal variable
    std::vector<uint32_t> order(nc);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return Q.cons[a].pos < Q.cons[b].pos; });
    o += "__device__ const uint8_t kWaveVarOf[" + S(nv) + "] = {";
    for (uint32_t v = 0; v < nv; ++v) o += S(Q.var_of[v]) + ", ";
    o += "};\n";
    if (cl.linear) {
        o += "__device__ const double kWaveJ[" + S(std::max(zj, 1u)) + "] = {";
        for (uint32_t s2 = 0; s2 < zj; ++s2) o += hexf(cl.jconst[s2]) + ", ";
        o += "};\n";
    }
    emit_wave_row_table(o, cl);
    o += "}  // namespace\n\nstruct ClsW : Cls0 {\n";
    o += "    static constexpr int ZJ = " + S(zj) + ", NQ = " + S(nq) + ", PMAX = " + S(pmax) + ";\n";
    o += "    static __device__ __forceinline__ DevCon con(int ci) { return kWaveCons[ci]; }\n";
    o += "    static __device__ __forceinline__ uint32_t pair(int k, int p, int lane) { return kWavePairs[(k * PMAX + p) * 64 + lane]; }\n";
    // the sum of squares and maximum of a residual vector in request order, straight-line (literal LDS offsets)
    o += "    static __device__ __forceinline__ void sum_rows(const double* rows, double& sq, double& mx) {\n        double w;\n";
    for (uint32_t ci : order)
        for (uint32_t rr = 0; rr < Q.cons[ci].nrows; ++rr)
            o += "        w = rows[" + S(Q.cons[ci].row0 + rr) + "]; sq += w * w; mx = ezpz::dev::fmax_abs(mx, w);\n";
    o += "        (void)w; (void)rows;\n    }\n";
    o += "    static __device__ __forceinline__ uint32_t var_of(int v) { return kWaveVarOf[v]; }\n";
    o += std::string("    static __device__ __forceinline__ double jconst(int s) { return ") + (cl.linear ? "kWaveJ[s]" : "0.0") + "; }\n";
    // the kinds present, each with its evaluator instantiated for that kind alone
    std::vector<uint32_t> kinds;
    for (const DevCon& d : Q.cons)
        if (std::find(kinds.begin(), kinds.end(), (uint32_t)d.kind) == kinds.end()) kinds.push_back(d.kind);
    o += "    template <class XP>\n    static __device__ __forceinline__ bool residual_of(const DevCon& c, XP xs, double& r0, double& r1) {\n        switch (c.kind) {\n";
    for (uint32_t k : kinds)
        o += "        case " + S(k) + ": { DevCon k = c; k.kind = " + S(k) + "; return ezpz::dev::con_residual<LINEAR>(k, xs, r0, r1); }\n";
    o += "        default: r0 = 0.0; r1 = 0.0; return false;\n        }\n    }\n";
    o += "    template <class XP, class JP>\n    static __device__ __forceinline__ bool jacobian_of(const DevCon& c, XP xs, const ezpz::dev::JacWriter<JP>& w) {\n        switch (c.kind) {\n";
    for (uint32_t k : kinds)
        o += "        case " + S(k) + ": { DevCon k = c; k.kind = " + S(k) + "; return ezpz::dev::con_jacobian<false>(k, xs, w); }\n";
    o += "        default: return false;\n        }\n    }\n";
    const bool fastdiv = (fastdiv_mask() >> 2) & 1u;
    for (int fast = 1; fast >= 0; --fast) {
        o += std::string("    static __device__ __forceinline__ bool ") + (fast ? "tail" : "tail_exact") +
             "(const double* Q, double lambda, double* d, double& dmax" + (fast ? ", bool& ok" : "") + ") {\n        bool bad = false;\n";
        for (uint32_t v = 0; v < nv; ++v)
            o += "        double D" + S(v) + " = Q[" + S(v) + "] + lambda, V" + S(v) + " = Q[" + S(nv + v) + "];\n";
        for (uint32_t s2 = 0; s2 < zlo; ++s2) o += "        double L" + S(s2) + " = Q[" + S(2 * nv + s2) + "];\n";
        emit_elimination(o, cl, kFactor | kRhs, fast && fastdiv, false);
        o += std::string("        (void)Q; (void)lambda;") + (fast ? " (void)ok;" : "") + "\n        return bad;\n    }\n";
    }
    emit_tail_wave(o, cl);
    o += "};\n\nextern \"C\" __global__ void __launch_bounds__(64) ezpz_jit_wave(const ezpz::jit::LaneArgs a) {\n";
    o += std::string("    ezpz::jit::wave_kernel<ClsW, ") + tf(unit_weights) + ">(a);\n}\n";
    return o;
}

}  // namespace ezpz
