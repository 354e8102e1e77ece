// Component plan (see comp_program.hpp): the plans -- components, classes, layouts, blobs, the lane and batch plans, the overlay.
// The kernels' source text is comp_source.cpp's.  Plain C++17, no device code.
#include "comp_program.hpp"
#include "comp_classes.hpp"
#include "policy.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>

#include "kinds.hpp"
#include "program.hpp"

namespace ezpz {

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
// What is worth a component plan, and what its 16-bit fields hold.
// (policy.hpp: the one table of launch-shape thresholds)
const EzpzLaunchPolicy kPolicy = launch_policy_for(256);
const size_t kMinInstances = kPolicy.comp_min_components;  // fewer components than two wavefronts' lanes: the other launch shapes serve
const size_t kMaxClasses = kPolicy.comp_max_classes;
const size_t kMaxClassVars = kPolicy.comp_max_component_vars, kMaxClassCons = kPolicy.comp_max_component_constraints;  // (the warning mask of a chunk is one 64-bit word per lane)

// Partial derivatives of the nine linear kinds in emission order (constraint_eval.hip.hpp con_jacobian; reference
// ezpz/src/constraints.rs:1252-1357,:1456-1512,:1599-1642).
int linear_partials(uint32_t kind, double pd[8]) {
    switch (kind) {
    case EZPZ_VERTICAL_DISTANCE:
    case EZPZ_HORIZONTAL_DISTANCE:
    case EZPZ_VERTICAL:
    case EZPZ_HORIZONTAL:
    case EZPZ_SCALAR_EQUAL:
        pd[0] = 1.0, pd[1] = -1.0;
        return 2;
    case EZPZ_FIXED:
    case EZPZ_CIRCLE_RADIUS:
        pd[0] = 1.0;
        return 1;
    case EZPZ_POINTS_COINCIDENT:
        pd[0] = 1.0, pd[1] = -1.0, pd[2] = 1.0, pd[3] = -1.0;
        return 4;
    case EZPZ_MIDPOINT:
        pd[0] = 1.0, pd[1] = -0.5, pd[2] = -0.5, pd[3] = 1.0, pd[4] = -0.5, pd[5] = -0.5;
        return 6;
    default:
        return 0;
    }
}

// The constant Jacobian of a linear class: slot values exactly as con_jacobian's writer stores them.
void linear_jacobian(Class& cl) {
    cl.jconst.assign(cl.Q.c.zj, 0.0);
    for (const DevCon& d : cl.Q.cons) {
        double pd[8];
        const int np = linear_partials(d.kind, pd);
        for (int e = 0; e < np; ++e) {
            const uint32_t code = d.jloc[e];
            const uint32_t slot = d.jbase + (code & 0x7Fu);
            const double w = d.weight * pd[e];
            if (code & 0x80u)
                cl.jconst[slot] = cl.jconst[slot] + w;
            else
                cl.jconst[slot] = w;
        }
    }
}

bool f32_exact(double v) { return (double)(float)v == v; }

uint32_t f32_bits(double v) {
    const float f = (float)v;
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

void push_double(std::vector<uint32_t>& w, double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    w.push_back((uint32_t)u);
    w.push_back((uint32_t)(u >> 32));
}

void align4(std::vector<uint32_t>& w) {
    while (w.size() % 4) w.push_back(0);
}

// One operation = one or more 8-word records.  `items` holds `words_per_item` words per item; `head` (0 or 2 words) goes
// into w2:w3 of the first record (the linear build's constants), shrinking that build's item room to w4..w7.
void emit_op(std::vector<uint32_t>& out, uint32_t opcode, uint32_t a, uint32_t b, const std::vector<uint32_t>& items,
             uint32_t words_per_item, uint32_t items_per_rec, uint32_t item_word0, const uint32_t* head,
             uint32_t first_flags = 0, uint32_t last_flags = 0) {
    const size_t n = items.size() / words_per_item;
    size_t done = 0;
    bool first = true;
    do {
        const size_t take = std::min<size_t>(items_per_rec, n - done);
        const bool last = done + take == n;
        uint32_t rec[kCompRecWords] = {0, 0, 0, 0, 0, 0, 0, 0};
        rec[0] = opcode | ((uint32_t)take << 8) | (first ? kCompFirst | first_flags : 0u) | (last ? kCompLast | last_flags : 0u);
        rec[1] = a | (b << 16);
        if (head) rec[2] = head[0], rec[3] = head[1];
        for (size_t k = 0; k < take * words_per_item; ++k) rec[item_word0 + k] = items[done * words_per_item + k];
        out.insert(out.end(), rec, rec + kCompRecWords);
        done += take;
        first = false;
    } while (done < n);
}

// The class program in the blob: the operation stream of the linear solve in execution order (+ one read-ahead pad
// record) and the constraint records (+ pad).  `params`: requests whose parameters go into the records as literals
// (w13:w14; a class that is a whole system shared by every lane) -- null: parameters come from per-instance tables.
// `fuse` (general records only): the assembly of an entry of JtJ sits right before the elimination of its column / slot
// and hands its value over in the accumulator (kCompKeep / kCompCont) instead of through the entry's row of state.
void emit_class_program(std::vector<uint32_t>& blob, Class& cl, bool LIN, const EzpzConstraint* params, bool request_order = false,
                        bool fuse = false) {
    const Program& Q = cl.Q;
    ClassLayout& H = cl.H;
    const uint32_t nv = Q.c.n_vars, zlo = Q.c.zlo, ncons = Q.c.n_cons;
    // ---- operation stream of the linear solve, in execution order ----
    std::vector<uint32_t> ops, items;
    fuse = fuse && !LIN;
    // the pairs of list i as `a | b << 16` items, appended
    auto pairs = [&](const std::vector<uint32_t>& ptr, const std::vector<uint32_t>& list, uint32_t i) {
        for (uint32_t q = ptr[i]; q < ptr[i + 1]; ++q) items.push_back(list[2 * q] | (list[2 * q + 1] << 16));
    };
    // an operation of the general build whose items are one list's pairs
    auto emit_list = [&](uint32_t opcode, uint32_t a, uint32_t b, const std::vector<uint32_t>& ptr, const std::vector<uint32_t>& list,
                         uint32_t first_flags = 0, uint32_t last_flags = 0) {
        items.clear();
        pairs(ptr, list, a);
        emit_op(ops, opcode, a, b, items, 1, kCompItemsGen, 2, nullptr, first_flags, last_flags);
    };
    const PartDesc part = Q.parts.empty() ? PartDesc{0, 0, 0, 0} : Q.parts[0];
    if (fuse) {
        // column by column in elimination order (the numbering is level-major, so every entry a column reads is done): its
        // diagonal, then the slots below it while d_j is still in a register
        // (an entry's assembly and its elimination share ONE record when their items fit it: COMP_DIAGCOL / COMP_SLOTA)
        auto emit_merged = [&](uint32_t opcode, uint32_t a, uint32_t n0) {
            uint32_t rec[kCompRecWords] = {0, 0, 0, 0, 0, 0, 0, 0};
            rec[0] = opcode | ((uint32_t)items.size() << 8) | kCompFirst | kCompLast | (n0 << 24);
            rec[1] = a;
            for (size_t k = 0; k < items.size(); ++k) rec[2 + k] = items[k];
            ops.insert(ops.end(), rec, rec + kCompRecWords);
        };
        for (uint32_t v = 0; v < nv; ++v) {
            const uint32_t nd = Q.colj_ptr[v + 1] - Q.colj_ptr[v], nc = Q.fwd_ptr[v + 1] - Q.fwd_ptr[v];
            if (nd + nc <= kCompItemsGen) {
                items.clear();
                pairs(Q.colj_ptr, Q.colj_items, v);
                pairs(Q.fwd_ptr, Q.fwd_items, v);
                emit_merged(COMP_DIAGCOL, v, nd);
            } else {
                emit_list(COMP_DIAG, v, 0, Q.colj_ptr, Q.colj_items, 0, kCompKeep);
                emit_list(COMP_COL, v, 0, Q.fwd_ptr, Q.fwd_items, kCompCont, 0);
            }
            for (uint32_t qs = Q.bwd_ptr[v]; qs < Q.bwd_ptr[v + 1]; ++qs) {
                const uint32_t s = Q.bwd_items[2 * qs];
                const uint32_t na = Q.apair_ptr[s + 1] - Q.apair_ptr[s], nl = Q.lpair_ptr[s + 1] - Q.lpair_ptr[s];
                if (na + nl <= kCompItemsGen) {
                    items.clear();
                    pairs(Q.apair_ptr, Q.apairs, s);
                    pairs(Q.lpair_ptr, Q.lpairs, s);
                    emit_merged(COMP_SLOTA, s, na);
                } else {
                    emit_list(COMP_OFF, s, 0, Q.apair_ptr, Q.apairs, 0, kCompKeep);
                    emit_list(COMP_SLOT, s, Q.l_col[s], Q.lpair_ptr, Q.lpairs, kCompCont, kCompDivReg);
                }
            }
        }
    } else {
        // the assembly of every entry (linear build: the sums of constants are formed here), then the elimination level by level
        for (uint32_t v = 0; v < nv; ++v) {
            if (!LIN) {
                emit_list(COMP_DIAG, v, 0, Q.colj_ptr, Q.colj_items);
                continue;
            }
            items.clear();
            double acc = 0.0;
            for (uint32_t q = Q.colj_ptr[v]; q < Q.colj_ptr[v + 1]; ++q) {
                const double jv = cl.jconst[Q.colj_items[2 * q]];
                acc += jv * jv;
                items.push_back(Q.colj_items[2 * q + 1]);
                items.push_back(f32_bits(jv));
            }
            std::vector<uint32_t> head;
            push_double(head, acc);
            emit_op(ops, COMP_DIAG, v, 0, items, 2, kCompItemsLin, 4, head.data());
        }
        for (uint32_t s = 0; s < zlo; ++s) {
            if (!LIN) {
                emit_list(COMP_OFF, s, 0, Q.apair_ptr, Q.apairs);
                continue;
            }
            items.clear();
            double acc = 0.0;
            for (uint32_t q = Q.apair_ptr[s]; q < Q.apair_ptr[s + 1]; ++q)
                acc += cl.jconst[Q.apairs[2 * q]] * cl.jconst[Q.apairs[2 * q + 1]];
            std::vector<uint32_t> head;
            push_double(head, acc);
            emit_op(ops, COMP_OFF, s, 0, items, 1, kCompItemsGen, 4, head.data());
        }
        for (uint32_t lv = 0; lv < part.nlev; ++lv) {
            const uint32_t c0 = Q.lvl_cptr[part.lvl0 + lv], c1 = Q.lvl_cptr[part.lvl0 + lv + 1];
            const uint32_t s0 = Q.lvl_sptr[part.lvl0 + lv], s1 = Q.lvl_sptr[part.lvl0 + lv + 1];
            for (uint32_t v = c0; v < c1; ++v) emit_list(COMP_COL, v, 0, Q.fwd_ptr, Q.fwd_items);
            for (uint32_t s = s0; s < s1; ++s) emit_list(COMP_SLOT, s, Q.l_col[s], Q.lpair_ptr, Q.lpairs);
        }
    }
    for (uint32_t lv = part.nlev; lv-- > 0;) {
        const uint32_t c0 = Q.lvl_cptr[part.lvl0 + lv], c1 = Q.lvl_cptr[part.lvl0 + lv + 1];
        for (uint32_t v = c0; v < c1; ++v) emit_list(COMP_BWD, v, 0, Q.bwd_ptr, Q.bwd_items);
    }
    H.n_ops = (uint32_t)(ops.size() / kCompRecWords);

    // ---- lay the class out in the blob: operation stream (+ one pad record), constraint records, tables ----
    align4(blob);
    H.ops_off = (uint32_t)blob.size();
    blob.insert(blob.end(), ops.begin(), ops.end());
    blob.resize(blob.size() + kCompRecWords, 0);  // the interpreter reads one record ahead
    H.cons_off = (uint32_t)blob.size();
    std::vector<uint32_t> rec_order(ncons);
    std::iota(rec_order.begin(), rec_order.end(), 0u);
    if (request_order)  // (one lane per system: sums of squares formed like the reference's sequential sum over the rows)
        std::sort(rec_order.begin(), rec_order.end(), [&](uint32_t x, uint32_t y) { return Q.cons[x].pos < Q.cons[y].pos; });
    for (uint32_t ci : rec_order) {
        const DevCon& d = Q.cons[ci];
        uint32_t rec[kCompConWords] = {};
        rec[0] = d.kind | ((uint32_t)d.tag << 8) | ((uint32_t)d.nrows << 16) | ((uint32_t)d.nslots << 24);
        rec[1] = d.row0 | (d.jbase << 16);
        for (int e = 0; e < 4; ++e) rec[2 + e] = d.ids[2 * e] | (d.ids[2 * e + 1] << 16);
        std::memcpy(&rec[6], d.jloc, 16);
        std::memcpy(&rec[10], &d.weight, 8);
        rec[12] = ci;
        if (params) std::memcpy(&rec[13], &params[d.pos].param, 8);
        rec[15] = d.pos;
        blob.insert(blob.end(), rec, rec + kCompConWords);
    }
    blob.resize(blob.size() + kCompConWords, 0);  // read-ahead pad
}

// EZPZ_DEBUG=comp in the environment: say on stderr why a system did not get a component plan.
#define COMP_REJECT(...)                                                            \
    do {                                                                            \
        static const bool dbg_ = debug_topic("comp");        \
        if (dbg_) std::fprintf(stderr, "[ezpz comp] no plan: " __VA_ARGS__), std::fputc('\n', stderr); \
        return false;                                                               \
    } while (0)

// comp_plan_build, one method per phase in the order build() lists them; a phase that returns false ends the build without a plan.
class CompPlanner {
  public:
    CompPlanner(const EzpzConstraint* cs, uint32_t n_cs, uint32_t n_vars, const CompLimits& lim, CompPlan& plan)
        : cs(cs), C(n_cs), n(n_vars), lim(lim), plan(plan), blob(plan.blob) {}
    bool build() {
        if (!find_components() || !find_classes() || !analyse_classes() || !lay_out_classes()) return false;
        deal_chunks();
        if (choose_slots()) {
            find_wave_ranges();
            plan.jit_source = comp_kernel_source(classes, shape);
            write_slot_tables();
        }
        if (!plan.interpretable && plan.jit_source.empty())
            COMP_REJECT("%llu rows of state do not fit the LDS and the system has no multi-workgroup specialised form",
                        (unsigned long long)rows_persistent);
        return true;
    }

  private:
    const EzpzConstraint* const cs;
    const uint32_t C, n;
    const CompLimits& lim;
    CompPlan& plan;
    std::vector<uint32_t>& blob;

    uint64_t m_total = 0;                          // find_components
    std::vector<uint32_t> vert_items, con_items;  // (what the components' spans view)
    std::vector<Component> comps;
    std::vector<Class> classes;                    // find_classes, analyse_classes, lay_out_classes
    uint32_t scratch_rows = 1;
    struct Chunk {
        uint32_t cls, inst0, count, cost, rows;
    };
    std::vector<Chunk> chunks;                     // deal_chunks
    uint64_t rows_persistent = 0;
    std::vector<uint32_t> nchunk;                  // choose_slots: chunks of class k
    CompKernelShape shape;
    std::vector<uint32_t> wave_lo, wave_n;         // find_wave_ranges

    // connected components: every variable of every row of a constraint belongs to one component
    bool find_components() {
        std::vector<uint32_t> parent(n);
        std::iota(parent.begin(), parent.end(), 0u);
        auto find = [&](uint32_t a) {
            while (parent[a] != a) a = parent[a] = parent[parent[a]];
            return a;
        };
        for (uint32_t i = 0; i < C; ++i) {
            if (cs[i].kind >= EZPZ_NUM_KINDS) return false;
            const KindInfo& K = kKinds[cs[i].kind];
            uint32_t first = NONE;
            for (int r = 0; r < K.n_rows; ++r)
                for (int e = 0; e < K.n_nz[r]; ++e) {
                    const uint32_t v = cs[i].ids[K.nz[r][e]];
                    if (v >= n) return false;  // MissingGuess: reported by the ordinary symbolic phase
                    if (first == NONE)
                        first = v;
                    else {
                        const uint32_t ra = find(v), rb = find(first);
                        if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
                    }
                }
            m_total += K.n_rows;
        }
        std::vector<uint32_t> comp_of(n, NONE);
        uint32_t n_comps = 0;
        for (uint32_t v = 0; v < n; ++v) {  // roots are the smallest member: components come out in order of first variable
            const uint32_t r = find(v);
            if (comp_of[r] == NONE) comp_of[r] = n_comps++;
            comp_of[v] = comp_of[r];
        }
        if (n_comps < kMinInstances) COMP_REJECT("%u components", n_comps);
        // members by counting sort: variables and constraints of a component in ascending order
        std::vector<uint32_t> vert_ptr(n_comps + 1, 0), con_ptr(n_comps + 1, 0), con_comp(C);
        vert_items.resize(n), con_items.resize(C);
        for (uint32_t v = 0; v < n; ++v) ++vert_ptr[comp_of[v] + 1];
        for (uint32_t i = 0; i < C; ++i) {
            con_comp[i] = comp_of[cs[i].ids[kKinds[cs[i].kind].nz[0][0]]];
            ++con_ptr[con_comp[i] + 1];
        }
        for (uint32_t c = 0; c < n_comps; ++c) vert_ptr[c + 1] += vert_ptr[c], con_ptr[c + 1] += con_ptr[c];
        {
            std::vector<uint32_t> vfill(vert_ptr.begin(), vert_ptr.end() - 1), cfill(con_ptr.begin(), con_ptr.end() - 1);
            for (uint32_t v = 0; v < n; ++v) vert_items[vfill[comp_of[v]]++] = v;
            for (uint32_t i = 0; i < C; ++i) con_items[cfill[con_comp[i]]++] = i;
        }
        comps.resize(n_comps);
        for (uint32_t c = 0; c < n_comps; ++c) {
            comps[c].verts = Span{vert_items.data() + vert_ptr[c], vert_ptr[c + 1] - vert_ptr[c]};
            comps[c].cons = Span{con_items.data() + con_ptr[c], con_ptr[c + 1] - con_ptr[c]};
        }
        for (const Component& c : comps)
            if (c.verts.size() > kMaxClassVars || c.cons.size() > kMaxClassCons)
                COMP_REJECT("a component of %zu variables, %zu constraints", c.verts.size(), c.cons.size());
        return true;
    }

    // constraint ci in its component's own numbering
    void local_con(const Component& comp, uint32_t ci, EzpzConstraint& out) const {
        out = cs[ci];
        const KindInfo& K = kKinds[out.kind];
        bool used[8] = {false, false, false, false, false, false, false, false};
        for (int r = 0; r < K.n_rows; ++r)
            for (int e = 0; e < K.n_nz[r]; ++e) used[K.nz[r][e]] = true;
        for (int k = 0; k < 8; ++k) {
            if (k < K.n_ids && used[k])
                out.ids[k] = (uint32_t)(std::lower_bound(comp.verts.begin(), comp.verts.end(), out.ids[k]) - comp.verts.begin());
            else
                out.ids[k] = 0;  // ids a kind never dereferences
        }
        out.priority = 0;
        out.flags = 0;
    }

    // classes: components with the same kinds, tags, weights and local variable pattern
    bool find_classes() {
        plan.unit_weights = true;
        for (uint32_t i = 0; i < C; ++i)
            if (cs[i].weight != 1.0) plan.unit_weights = false;
        std::vector<std::vector<uint32_t>> class_sig;  // (at most kMaxClasses: compared one by one)
        std::vector<uint32_t> sig;
        for (uint32_t ic = 0; ic < comps.size(); ++ic) {
            const Component& comp = comps[ic];
            sig.clear();
            sig.push_back((uint32_t)comp.verts.size());
            sig.push_back((uint32_t)comp.cons.size());
            for (uint32_t ci : comp.cons) {
                EzpzConstraint lc;
                local_con(comp, ci, lc);
                uint64_t wbits;
                std::memcpy(&wbits, &lc.weight, 8);
                sig.push_back(lc.kind | ((uint32_t)lc.tag << 16));
                sig.push_back((uint32_t)wbits);
                sig.push_back((uint32_t)(wbits >> 32));
                for (int k = 0; k < 8; ++k) sig.push_back(lc.ids[k]);
            }
            size_t k = 0;
            while (k < class_sig.size() && class_sig[k] != sig) ++k;
            if (k == class_sig.size()) {
                if (classes.size() >= kMaxClasses) COMP_REJECT("more than %zu classes", kMaxClasses);
                class_sig.push_back(sig);
                classes.emplace_back();
                classes.back().rep = ic;
            }
            classes[k].instances.push_back(ic);
        }
        return true;
    }

    // per class: the symbolic phase of the representative, its constant Jacobian when linear, its cost
    bool analyse_classes() {
        bool all_linear = true;
        for (Class& cl : classes) {
            const Component& rep = comps[cl.rep];
            std::vector<EzpzConstraint> local(rep.cons.size());
            for (size_t k = 0; k < rep.cons.size(); ++k) local_con(rep, rep.cons[k], local[k]);
            BuildError be;
            if (!build_program(local.data(), local.size(), rep.verts.size(), cl.Q, be, 1, false)) return false;
            const Program& Q = cl.Q;
            if (Q.c.n_parts != 1 || Q.c.zj >= 0xFFFF || Q.c.zlo >= 0xFFFF || Q.c.n_rows >= 0xFFFF) return false;
            for (const DevCon& d : Q.cons) cl.linear = cl.linear && kind_is_linear(d.kind);
            if (cl.linear) {
                linear_jacobian(cl);
                for (double v : cl.jconst) cl.consts_f32 = cl.consts_f32 && f32_exact(v);
            }
            all_linear = all_linear && cl.linear && cl.consts_f32;
            uint32_t cost = 8;
            for (const DevCon& d : Q.cons) cost += kind_is_linear(d.kind) ? 12 : 60;
            cost += 40 * Q.c.n_vars + 14 * Q.c.zlo + 4 * (uint32_t)(Q.colj_items.size() / 2 + Q.apairs.size() / 2 + Q.lpairs.size() / 2 +
                                                                    Q.fwd_items.size() / 2 + Q.bwd_items.size() / 2);
            cl.cost = cost;
        }
        plan.linear = all_linear;
        return true;
    }

    // per class: the rows of a chunk's state, then its program and its tables over the instances in the blob
    bool lay_out_classes() {
        const bool LIN = plan.linear;
        blob.clear();
        for (Class& cl : classes) {
            const Program& Q = cl.Q;
            const uint32_t nv = Q.c.n_vars, m = Q.c.n_rows, zj = Q.c.zj, zlo = Q.c.zlo, ncons = Q.c.n_cons;
            ClassLayout& H = cl.H;
            H.nv = nv, H.m = m, H.zj = zj, H.ncons = ncons;
            H.o_d = nv;
            H.o_r0 = 2 * nv;
            H.o_r1 = 2 * nv + m;
            H.o_j = 2 * nv + 2 * m;
            H.o_wm = H.o_j + (LIN ? 0 : zj);
            H.rows_p = H.o_wm + (LIN ? 0 : 1);
            H.s_l = nv;
            scratch_rows = std::max(scratch_rows, nv + zlo);
            const uint32_t ninst = (uint32_t)cl.instances.size();
            H.ninst_pad = (ninst + 63) & ~63u;

            emit_class_program(blob, cl, LIN, nullptr);
            align4(blob);
            H.ids_off = (uint32_t)blob.size();
            blob.resize(blob.size() + (size_t)nv * H.ninst_pad, 0);
            for (uint32_t kv = 0; kv < nv; ++kv)
                for (uint32_t i = 0; i < ninst; ++i)
                    blob[H.ids_off + (size_t)kv * H.ninst_pad + i] = comps[cl.instances[i]].verts[Q.var_of[kv]];
            align4(blob);
            H.par_off = (uint32_t)blob.size();
            blob.resize(blob.size() + (size_t)2 * ncons * H.ninst_pad, 0);
            for (uint32_t ci = 0; ci < ncons; ++ci)
                for (uint32_t i = 0; i < ninst; ++i) {
                    const double p = cs[comps[cl.instances[i]].cons[Q.cons[ci].pos]].param;
                    std::memcpy(&blob[H.par_off + 2 * ((size_t)ci * H.ninst_pad + i)], &p, 8);
                }
            align4(blob);
            H.pos_off = (uint32_t)blob.size();
            blob.resize(blob.size() + (size_t)ncons * H.ninst_pad, 0);
            for (uint32_t ci = 0; ci < ncons; ++ci)
                for (uint32_t i = 0; i < ninst; ++i)
                    blob[H.pos_off + (size_t)ci * H.ninst_pad + i] = comps[cl.instances[i]].cons[Q.cons[ci].pos];
            // (the overlay of a call with driven parameters is a table of its own, laid out like this one: comp_param_overlay)
            H.ovl_off = plan.ovl_words;
            plan.ovl_words += ncons * H.ninst_pad;
            if (blob.size() > (64u << 20)) return false;

            plan.zj += (uint64_t)zj * ninst;
            plan.za += (uint64_t)Q.c.za * ninst;
            plan.zl += (uint64_t)(zlo + nv) * ninst;
            plan.max_levels = std::max(plan.max_levels, Q.c.n_levels);
        }
        return true;
    }

    // chunks of <= 64 instances, dealt to the wavefronts of the interpreter (longest processing time first), and their CompChunks
    void deal_chunks() {
        for (size_t k = 0; k < classes.size(); ++k) {
            const uint32_t ninst = (uint32_t)classes[k].instances.size();
            for (uint32_t i0 = 0; i0 < ninst; i0 += 64)
                chunks.push_back(Chunk{(uint32_t)k, i0, std::min<uint32_t>(64, ninst - i0), classes[k].cost, classes[k].H.rows_p});
        }
        for (const Chunk& c : chunks) rows_persistent += c.rows;
        // Wavefronts per workgroup (= per system): more of them shorten a solve, but every one pays the reductions of
        // the LM control, and a CU holds 160 KiB of LDS: take the count that puts the most wavefronts on a CU (several
        // workgroups side by side when the state allows it), the smaller workgroup on a tie.
        const uint32_t max_waves = plan.linear ? lim.max_waves_linear : lim.max_waves_general;
        const size_t fixed_bytes = 3 * 4 * 16 * 8 + 64;  // reduction scratch + flags + warning counters
        auto bytes_for = [&](uint32_t w) { return (rows_persistent + (uint64_t)w * scratch_rows) * 512 + fixed_bytes; };
        uint32_t W = 0;
        uint64_t best_waves = 0;
        for (uint32_t w = 1; w <= max_waves; w <<= 1) {
            if (w > chunks.size() && w > 1) break;
            const uint64_t bytes = bytes_for(w);
            if (bytes > lim.lds_bytes) continue;
            const uint64_t per_cu = std::min<uint64_t>(lim.lds_bytes / bytes, 32 / w);
            const uint64_t waves = std::min<uint64_t>(per_cu * w, 16);  // beyond 4 per SIMD nothing is gained
            if (waves > best_waves) best_waves = waves, W = w;
        }
        // State that does not fit one CU's LDS (one large system: the 200 000-variable ladder): no interpreter, but the
        // class-specialised kernel keeps its state in registers and spreads the system over several workgroups (choose_slots).
        plan.interpretable = W != 0;
        if (!plan.interpretable) W = 1;
        std::vector<uint32_t> order(plan.interpretable ? chunks.size() : 0);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return chunks[a].cost > chunks[b].cost; });
        std::vector<uint64_t> load(W, 0);
        std::vector<std::vector<uint32_t>> of_wave(W);
        for (uint32_t c : order) {
            const uint32_t w = (uint32_t)(std::min_element(load.begin(), load.end()) - load.begin());
            load[w] += chunks[c].cost;
            of_wave[w].push_back(c);
        }
        align4(blob);
        plan.o_waves = (uint32_t)blob.size();
        blob.resize(blob.size() + W + 1, 0);
        while (blob.size() % 32) blob.push_back(0);
        plan.o_chunks = (uint32_t)blob.size();
        uint32_t row = 0, nch = 0;
        for (uint32_t w = 0; w < W; ++w) {
            std::sort(of_wave[w].begin(), of_wave[w].end());  // class-major, instances ascending
            blob[plan.o_waves + w] = nch;
            for (uint32_t c : of_wave[w]) {
                const ClassLayout& H = classes[chunks[c].cls].H;
                CompChunk ch{};
                ch.count = chunks[c].count;
                ch.nv = H.nv, ch.m = H.m, ch.ncons = H.ncons;
                ch.n_ops = H.n_ops, ch.ops_off = H.ops_off, ch.cons_off = H.cons_off;
                ch.row0 = row;
                ch.o_d = H.o_d, ch.o_r0 = H.o_r0, ch.o_r1 = H.o_r1, ch.o_j = H.o_j, ch.o_wm = H.o_wm, ch.s_l = H.s_l;
                ch.stride = H.ninst_pad;
                ch.ids_off = H.ids_off + chunks[c].inst0;
                ch.par_off = H.par_off + 2 * chunks[c].inst0;
                ch.pos_off = H.pos_off + chunks[c].inst0;
                ch.ovl_off = H.ovl_off + chunks[c].inst0;
                const uint32_t* p = reinterpret_cast<const uint32_t*>(&ch);
                blob.insert(blob.end(), p, p + sizeof(CompChunk) / 4);
                row += chunks[c].rows;
                ++nch;
            }
        }
        blob[plan.o_waves + W] = nch;
        blob.resize(blob.size() + 16, 0);
        plan.n_waves = W;
        plan.n_chunks = nch;
        plan.n_classes = (uint32_t)classes.size();
        plan.n_instances = (uint32_t)comps.size();
        plan.rows_persistent = (uint32_t)rows_persistent;
        plan.scratch_rows = scratch_rows;
        plan.lds_bytes = plan.interpretable ? (uint32_t)bytes_for(W) : 0u;
        plan.n_vars = n;
        plan.n_cons = C;
        plan.n_rows = (uint32_t)m_total;
    }

    // The class-specialised kernel: a wavefront gets ceil(chunks of class k / T) slots of every class k -- the same sequence for
    // every wavefront, so one body of code serves them all; a slot beyond a class's last chunk runs with no active lane.  T = the
    // fewest wavefronts per system (every one pays the LM control's reductions) whose slots still fit the register file.
    // False: the system has no such kernel.
    bool choose_slots() {
        nchunk.resize(classes.size());
        for (size_t k = 0; k < classes.size(); ++k) nchunk[k] = ((uint32_t)classes[k].instances.size() + 63) / 64;
        auto per_slot = [&](size_t k) {  // registers of one slot's state
            const ClassLayout& H = classes[k].H;
            return 2ull * (2 * H.nv + 2 * H.m + (classes[k].linear ? 0 : H.zj) + H.ncons) + H.nv + 4;
        };
        std::vector<uint32_t>& slots_k = shape.slots_k;  // slots of class k per wavefront
        slots_k.assign(classes.size(), 0);
        auto slots_for = [&](uint32_t t) {  // ... with t wavefronts per system; returns their registers
            uint64_t v = 0;
            for (size_t k = 0; k < classes.size(); ++k) slots_k[k] = (nchunk[k] + t - 1) / t, v += per_slot(k) * slots_k[k];
            return v;
        };
        uint32_t T = 0, G = 1;
        static const char* env_t = std::getenv("EZPZ_JIT_WAVES");
        if (env_t && std::atoi(env_t) > 0 && plan.interpretable) {
            T = (uint32_t)std::atoi(env_t);
        } else {
            // measured (2000 x 2000 / 2400 x 2400 / 800 x 800, M solves/s): the fewest wavefronts whose slots take up to
            // ~176 VGPRs win -- T = 2 / 4 / 8 on 2000 x 2000 (224 / 112 / 56 VGPRs of state): 58 / 68 / 57; T = 4 / 8 on
            // 2400 x 2400 (153 / 97): 53 / 36; T = 2 / 4 / 8 on 800 x 800 (112 / 56 / 41): 153 / 120 / 72
            for (uint32_t t = 1; t <= 8 && !T; t <<= 1)
                if (slots_for(t) <= 176) T = t;
        }
        if (T) {
            slots_for(T);
        } else {
            // One workgroup cannot hold the system: G workgroups of 4 wavefronts share it (grid reductions, see
            // jit_kernel.hip.hpp).  A wavefront takes slots of every class in proportion to the class's chunks, ~112
            // VGPRs of state in all.
            T = 4;
            uint64_t weight = 0;
            for (size_t k = 0; k < classes.size(); ++k) weight += (uint64_t)nchunk[k] * per_slot(k);
            uint32_t waves = 0;
            for (size_t k = 0; k < classes.size(); ++k) {
                slots_k[k] = std::max<uint32_t>(1, (uint32_t)((double)nchunk[k] * 112.0 / (double)weight + 0.5));
                waves = std::max(waves, (nchunk[k] + slots_k[k] - 1) / slots_k[k]);
            }
            G = (waves + T - 1) / T;
            if (G <= 1) {  // few chunks of many big classes: one workgroup after all, one slot per class and wavefront
                G = 1;
                T = 8;
                slots_for(T);
            }
        }
        shape.waves = T, shape.wgs = G;
        shape.vgprs = 0;
        for (size_t k = 0; k < classes.size(); ++k) shape.vgprs += per_slot(k) * slots_k[k];
        shape.unit_weights = plan.unit_weights;
        return T <= 16 && shape.vgprs <= 360 && G <= 256 && (plan.interpretable || G > 1);
    }

    // wavefront w of the system's G * T owns chunks w * slots_k[k] + j, j < slots_k[k], of every class k: what its slots hold
    template <class F>
    void for_each_slot(uint32_t w, F&& f) const {
        for (size_t k = 0; k < classes.size(); ++k)
            for (uint32_t j = 0; j < shape.slots_k[k]; ++j) f(classes[k], w * shape.slots_k[k] + j);
    }

    // The caller's variables of every wavefront: one contiguous run?  Then the kernels that do not wait for verdicts move a
    // wavefront's piece of a row as whole lines (comp_source.cpp: comp_kernel_source; jit_kernel.hip.hpp: fast_wave).
    void find_wave_ranges() {
        const uint32_t waves = shape.wgs * shape.waves;
        wave_lo.assign(waves, 0), wave_n.assign(waves, 0);
        bool contiguous = true;
        for (uint32_t w = 0; w < waves && contiguous; ++w) {
            uint32_t lo = ~0u, hi = 0, cnt = 0;
            for_each_slot(w, [&](const Class& cl, uint32_t chunk) {
                const uint32_t ninst = (uint32_t)cl.instances.size();
                for (uint32_t i = chunk * 64; i < ninst && i < chunk * 64 + 64; ++i)
                    for (uint32_t kv = 0; kv < cl.H.nv; ++kv) {
                        const uint32_t id = comps[cl.instances[i]].verts[cl.Q.var_of[kv]];
                        lo = std::min(lo, id), hi = std::max(hi, id), ++cnt;
                    }
            });
            if (cnt == 0) continue;  // (a wavefront beyond the system's last chunk)
            // (every variable belongs to one instance: as many variables as the run is long means exactly the run)
            contiguous = hi - lo + 1 == cnt;
            wave_lo[w] = lo, wave_n[w] = cnt;
        }
        shape.contiguous = contiguous;
    }

    // blob: [wave][slot] {ids_off, par_off, pos_off, count}, and [wave] {first variable, count} when the ranges are contiguous
    void write_slot_tables() {
        const uint32_t waves = shape.wgs * shape.waves;
        align4(blob);
        plan.o_jit_slots = (uint32_t)blob.size();
        for (uint32_t w = 0; w < waves; ++w)
            for_each_slot(w, [&](const Class& cl, uint32_t chunk) {
                const ClassLayout& H = cl.H;
                const uint32_t ninst = (uint32_t)cl.instances.size();
                const uint32_t inst0 = std::min(chunk * 64, H.ninst_pad ? H.ninst_pad - 64 : 0u);
                const uint32_t count = (uint64_t)chunk * 64 < ninst ? std::min<uint32_t>(64, ninst - chunk * 64) : 0u;
                blob.push_back(H.ids_off + inst0);
                blob.push_back(H.par_off + 2 * inst0);
                blob.push_back(H.pos_off + inst0);
                blob.push_back(count);
            });
        blob.resize(blob.size() + 16, 0);
        plan.o_jit_ranges = 0;
        if (shape.contiguous) {
            plan.o_jit_ranges = (uint32_t)blob.size();
            for (uint32_t w = 0; w < waves; ++w) blob.push_back(wave_lo[w]), blob.push_back(wave_n[w]);
            blob.resize(blob.size() + 16, 0);
        }
        plan.jit_waves = shape.waves;
        plan.jit_slots = std::accumulate(shape.slots_k.begin(), shape.slots_k.end(), 0u);
        plan.jit_wgs = shape.wgs;
    }
};

}  // namespace

bool comp_plan_build(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, const CompLimits& lim, CompPlan& plan) {
    plan = CompPlan();
    if (n_cs == 0 || n_vars < kMinInstances || n_cs > 0x3FFFFFFFu || n_vars > 0x3FFFFFFFu) return false;
    return CompPlanner(cs, (uint32_t)n_cs, (uint32_t)n_vars, lim, plan).build();
}

// ---- one lane per system (jit_kernel.hip.hpp, lane_kernel) --------------------------------------------------------------------------
bool lane_plan_build(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, LanePlan& plan) {
    plan = LanePlan();
    // what a lane can hold in registers: x, the accepted x, r, r_next, d, the Jacobian values of one iteration, L
    if (n_cs == 0 || n_vars == 0 || n_vars > kPolicy.lane_max_vars || n_cs > kPolicy.lane_max_constraints) return false;
    Class cl;
    BuildError be;
    if (!build_program(cs, n_cs, n_vars, cl.Q, be, 1, false)) return false;
    const Program& Q = cl.Q;
    if (Q.c.zj + Q.c.zlo > 220 || Q.c.n_rows > 48) return false;
    plan.unit_weights = true;
    for (const DevCon& d : Q.cons) {
        cl.linear = cl.linear && kind_is_linear(d.kind);
        if (d.weight != 1.0) plan.unit_weights = false;
    }
    if (cl.linear) linear_jacobian(cl);
    cl.H.ninst_pad = 1;
    const std::string cls = lane_class_source(cl, cs);
    plan.jit_source = lane_kernel_source(cls, plan.unit_weights);
    plan.n_vars = (uint32_t)n_vars;
    plan.n_cons = (uint32_t)n_cs;
    plan.n_rows = Q.c.n_rows;
    plan.wave_source = wave_kernel_source(cls, cl, cs, plan.unit_weights);
    return true;
}

// ---- lanes across the batch (batch_kernel.hip.hpp) ------------------------------------------------------------------------------------
bool batch_plan_build(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, BatchPlan& plan) {
    plan = BatchPlan();
    if (n_cs == 0 || n_vars == 0 || n_vars > 60000 || n_cs > 60000) return false;
    Class cl;
    BuildError be;
    if (!build_program(cs, n_cs, n_vars, cl.Q, be, 1, false, true)) return false;
    const Program& Q = cl.Q;
    if (Q.c.n_parts != 1 || Q.c.zj >= 0xFFFF || Q.c.zlo >= 0xFFFF || Q.c.n_rows >= 0xFFFF) return false;
    plan.unit_weights = true;
    for (const DevCon& d : Q.cons)
        if (d.weight != 1.0) plan.unit_weights = false;
    cl.linear = false;  // the general records: Jacobian values are stored (no constant folding here)
    emit_class_program(plan.blob, cl, false, cs, true, true);
    align4(plan.blob);
    plan.var_off = (uint32_t)plan.blob.size();
    plan.blob.insert(plan.blob.end(), Q.var_of.begin(), Q.var_of.end());
    plan.blob.resize(plan.blob.size() + 16, 0);
    // ... and its inverse: the state row of the caller's variable c (the rows of a batch are moved in tiles of eight of the
    // caller's consecutive variables, batch_kernel.hip.hpp)
    plan.inv_off = (uint32_t)plan.blob.size();
    std::vector<uint32_t> inv(Q.var_of.size(), 0);
    for (uint32_t k = 0; k < (uint32_t)Q.var_of.size(); ++k) inv[Q.var_of[k]] = k;
    plan.blob.insert(plan.blob.end(), inv.begin(), inv.end());
    plan.blob.resize(plan.blob.size() + 16, 0);
    plan.nv = Q.c.n_vars, plan.m = Q.c.n_rows, plan.zj = Q.c.zj, plan.zlo = Q.c.zlo, plan.ncons = Q.c.n_cons;
    plan.n_ops = cl.H.n_ops, plan.ops_off = cl.H.ops_off, plan.cons_off = cl.H.cons_off;
    plan.o_d = plan.nv;
    plan.o_r = 2 * plan.nv;
    plan.o_rn = plan.o_r + plan.m;
    plan.o_j = plan.o_rn + plan.m;
    plan.o_dg = plan.o_j + plan.zj;
    plan.o_l = plan.o_dg + plan.nv;
    plan.rows = plan.o_l + plan.zlo;
    if (debug_topic("lanes")) {  // the operation stream by kind: records and items (an item is two loads)
        uint64_t recs[8] = {}, items[8] = {};
        for (uint32_t io = 0; io < plan.n_ops; ++io) {
            const uint32_t w = plan.blob[plan.ops_off + io * kCompRecWords];
            recs[w & 7u] += 1;
            items[w & 7u] += (w >> 8) & 0xFFu;
        }
        std::fprintf(stderr, "[ezpz lanes] nv %u m %u zj %u zlo %u rows %u ops %u |", plan.nv, plan.m, plan.zj, plan.zlo, plan.rows, plan.n_ops);
        const char* names[] = {"DIAG", "OFF", "COL", "SLOT", "BWD", "DIAGCOL", "SLOTA"};
        const uint32_t codes[] = {COMP_DIAG, COMP_OFF, COMP_COL, COMP_SLOT, COMP_BWD, COMP_DIAGCOL, COMP_SLOTA};
        for (int k = 0; k < 7; ++k)
            std::fprintf(stderr, " %s %llu recs %llu items", names[k], (unsigned long long)recs[codes[k] & 7u], (unsigned long long)items[codes[k] & 7u]);
        std::fputc('\n', stderr);
    }
    return true;
}

// The interpreter's overlay for a call that drives parameters (ezpz_system_solve_batch_params): a table laid out like the
// chunks' parameter tables -- [constraint of the class][instance], CompChunk::ovl_off -- that holds, for the constraint a lane
// evaluates, its place in the call's list (slot_of_pos[caller's position]) or kNoParamSlot.  The parameter tables themselves, and
// everything the plan derives from the topology, stay as they are: no value of a parameter went into classes or programs.
void comp_param_overlay(const CompPlan& plan, const uint32_t* slot_of_pos, std::vector<uint32_t>& out) {
    out.assign(std::max<uint32_t>(plan.ovl_words, 1), 0xFFFFFFFFu);
    const CompChunk* chunks = reinterpret_cast<const CompChunk*>(plan.blob.data() + plan.o_chunks);
    for (uint32_t c = 0; c < plan.n_chunks; ++c) {
        const CompChunk& ch = chunks[c];
        for (uint32_t ci = 0; ci < ch.ncons; ++ci)
            for (uint32_t l = 0; l < ch.count; ++l)
                out[ch.ovl_off + (size_t)ci * ch.stride + l] = slot_of_pos[plan.blob[ch.pos_off + (size_t)ci * ch.stride + l]];
    }
}

}  // namespace ezpz
