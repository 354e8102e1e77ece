// Host side of the dimension sensitivities on the FRONTAL shape: the tables front_sens_kernel needs to run a
// right-hand side through a factorisation that is already in the panels -- derived from the FrontPlan's blob alone (the blob
// itself is not changed), plain C++ with no device in sight: tests/front_sens_ref.py executes them in numpy,
// tools/asan_front_sens.cpp drives this file under the sanitizers.
#include <algorithm>
#include <cstring>

#include "fronts.hpp"
#include "front_sens_types.hpp"
#include "policy.hpp"

namespace ezpz {

namespace {

struct Entry {
    uint32_t hdr;
    std::vector<uint32_t> ops;
};

// trips of 64 entries of `width` words each: headers, then the words; short trips are filled with `pad_hdr` / `pad_op`
void emit_trip(std::vector<uint32_t>& out, const Entry* e, size_t n, uint32_t width, uint32_t pad_hdr, uint32_t pad_op) {
    const size_t at = out.size();
    out.resize(at + 64 * (1 + (size_t)width), pad_op);
    for (uint32_t l = 0; l < 64; ++l) {
        out[at + l] = l < n ? ((e[l].hdr & 0x00FFFFFFu) | (width << 24)) : (pad_hdr | (width << 24));
        for (uint32_t q = 0; q < width; ++q)
            if (l < n && q < e[l].ops.size()) out[at + 64 * (1 + (size_t)q) + l] = e[l].ops[q];
    }
}

}  // namespace

bool front_sens_tables(const FrontPlan& plan, const uint32_t* positions, size_t n_param, std::vector<uint32_t>& out) {
    const unsigned char* const blob = plan.blob.data();
    const uint32_t G = plan.n_wgs;
    if (plan.blob.size() < (size_t)G * sizeof(FrontWg)) return false;
    const FrontWg* const wgs = reinterpret_cast<const FrontWg*>(blob);
    out.assign(4 + 4 * (size_t)G, 0u);
    for (uint32_t g = 0; g < G; ++g) {
        const FrontWg& W = wgs[g];
        const unsigned char* const tab = blob + W.o_tables;
        const FrontDesc* const descs = reinterpret_cast<const FrontDesc*>(tab);
        const uint32_t* const stream = reinterpret_cast<const uint32_t*>(tab + W.t_stream);
        // ---- the rhs-only assembly stream ------------------------------------------------------------------------------------
        std::vector<Entry> rhs;
        for (uint32_t t = 0; t < W.asm_trips; ++t) {
            const uint32_t* st = stream + stream[W.asm_word0 + t];
            const uint32_t w = st[0] >> 24;
            for (uint32_t l = 0; l < 64; ++l) {
                const uint32_t hdr = st[l];
                if (!(hdr & FASM_RHS) || (hdr & FASM_NOP)) continue;
                Entry e;
                e.hdr = hdr;
                for (uint32_t q = 0; q < w; ++q) e.ops.push_back(st[64 * (1 + q) + l]);
                rhs.push_back(std::move(e));
            }
        }
        std::stable_sort(rhs.begin(), rhs.end(), [](const Entry& a, const Entry& b) { return a.ops.size() < b.ops.size(); });
        std::vector<uint32_t> trips, words;
        for (size_t i = 0; i < rhs.size();) {
            const uint32_t w = (uint32_t)rhs[i].ops.size();
            size_t n = 1;
            while (n < 64 && i + n < rhs.size() && rhs[i + n].ops.size() == w) ++n;
            trips.push_back((uint32_t)words.size());
            emit_trip(words, &rhs[i], n, w, FASM_NOP | FASM_RHS, W.zj | (W.n_rows << 16));
            i += n;
        }
        FrontSensWg& T = *reinterpret_cast<FrontSensWg*>(&out[4 + 4 * (size_t)g]);
        T.asm_trips = (uint32_t)trips.size();
        T.w_asm_offs = (uint32_t)out.size();
        const uint32_t w_words = (uint32_t)(out.size() + trips.size());
        for (uint32_t t : trips) out.push_back(w_words + t);
        out.insert(out.end(), words.begin(), words.end());
        // ---- the rhs-only extend-add, per front ------------------------------------------------------------------------------
        const uint32_t w_ext = (uint32_t)out.size();
        out.resize(out.size() + 2 * (size_t)W.n_fronts, 0u);
        for (uint32_t k = 0; k < W.n_fronts; ++k) {
            const FrontDesc& d = descs[k];
            const uint32_t K = d.K, S = d.S, S1 = S + 1, R = S - K;
            // the front's rhs rows, as the source stream names destinations: doubles from l_panels
            std::vector<uint32_t> dsts;
            for (uint32_t c = 0; c < K; ++c) dsts.push_back(d.panel + c * S1 + S - W.l_panels);
            for (uint32_t b = 0; b < R; ++b) dsts.push_back(d.upd + R * (R + 1) / 2 + b - W.l_panels);
            std::sort(dsts.begin(), dsts.end());
            std::vector<Entry> ext;
            const uint32_t* st = stream + d.src_off;
            for (uint32_t e0 = 0, tr = 0; e0 < d.src_n; e0 += 64, ++tr) {
                const uint32_t v = d.src_v[tr < 3 ? tr : 3];
                for (uint32_t l = 0; l < 64; ++l) {
                    const uint32_t hdr = st[l];
                    if ((hdr & FASM_NOP) || !std::binary_search(dsts.begin(), dsts.end(), hdr & 0xFFFFu)) continue;
                    Entry e;
                    e.hdr = hdr & 0xFFFFu;
                    for (uint32_t q = 0; q < v; ++q) e.ops.push_back(st[64 * (1 + q) + l]);
                    while (!e.ops.empty() && e.ops.back() == 0u) e.ops.pop_back();  // (padding sources)
                    ext.push_back(std::move(e));
                }
                st += 64 * (1 + (size_t)v);
            }
            uint32_t n_trips = 0;
            const uint32_t first = (uint32_t)out.size();
            for (size_t i = 0; i < ext.size(); i += 64, ++n_trips) {
                const size_t n = std::min<size_t>(64, ext.size() - i);
                uint32_t v = 0;
                for (size_t l = 0; l < n; ++l) v = std::max<uint32_t>(v, (uint32_t)ext[i + l].ops.size());
                emit_trip(out, &ext[i], n, v, FASM_NOP, 0u);
            }
            out[w_ext + 2 * (size_t)k] = n_trips ? first : 0u;
            out[w_ext + 2 * (size_t)k + 1] = n_trips;
        }
        FrontSensWg& T2 = *reinterpret_cast<FrontSensWg*>(&out[4 + 4 * (size_t)g]);  // (`out` has grown)
        T2.w_ext = w_ext;
        T2.n_fronts = W.n_fronts;
    }
    // ---- the home of each listed constraint -----------------------------------------------------------------------------------
    std::vector<uint32_t> home_wg(std::max<uint32_t>(plan.n_cons, 1), 0xFFFFFFFFu), home_idx(std::max<uint32_t>(plan.n_cons, 1), 0u);
    for (uint32_t g = 0; g < G; ++g) {
        const FrontWg& W = wgs[g];
        const DevCon* const cons = reinterpret_cast<const DevCon*>(blob + W.o_cons);
        for (uint32_t i = 0; i < W.n_cons; ++i) {
            const uint32_t pos = cons[i].pos;
            if (pos >= plan.n_cons || home_wg[pos] != 0xFFFFFFFFu) return false;  // (a constraint is evaluated once)
            home_wg[pos] = g;
            home_idx[pos] = i;
        }
    }
    const uint32_t w_home = (uint32_t)out.size();
    for (size_t j = 0; j < n_param; ++j) {
        const uint32_t pos = positions[j];
        if (pos >= plan.n_cons || home_wg[pos] == 0xFFFFFFFFu) return false;
        out.push_back(home_wg[pos]);
        out.push_back(home_idx[pos]);
    }
    FrontSensHead& H = *reinterpret_cast<FrontSensHead*>(out.data());
    H.n_wgs = G;
    H.n_param = (uint32_t)n_param;
    H.w_home = w_home;
    H.n_words = (uint32_t)out.size();
    return true;
}

}  // namespace ezpz

extern "C" long ezpz_debug_front_sens_tables(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, uint32_t wgs, uint32_t max_wgs,
                                             uint64_t lds_bytes, const uint32_t* positions, size_t n_param, unsigned char* buf,
                                             size_t cap, uint64_t* info) {
    if ((!cs && n_cs) || (!positions && n_param)) return EZPZ_ERR_INVALID_ARGUMENT;
    for (size_t j = 0; j < n_param; ++j)
        if (positions[j] >= n_cs) return EZPZ_ERR_INVALID_ARGUMENT;
    ezpz::FrontOptions opt;
    opt.wgs = wgs;
    if (max_wgs) opt.max_wgs = max_wgs;
    if (lds_bytes) opt.lds_bytes = (size_t)lds_bytes;
    ezpz::FrontPlan plan;
    const char* why = nullptr;
    if (!ezpz::front_plan_build(cs, n_cs, n_vars, opt, plan, &why)) return 0;
    std::vector<uint32_t> tabs;
    if (!ezpz::front_sens_tables(plan, positions, n_param, tabs)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (info) {
        info[0] = plan.n_wgs;
        info[1] = tabs.size();
        info[2] = plan.blob.size();
        info[3] = 0;
    }
    if (buf && cap) std::memcpy(buf, tabs.data(), std::min(cap, tabs.size() * sizeof(uint32_t)));
    return (long)(tabs.size() * sizeof(uint32_t));
}
