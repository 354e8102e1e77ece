// g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iezpz_amd/csrc -Iinclude tools/asan_front_sens.cpp ezpz_amd/csrc/front_sens_plan.cpp ezpz_amd/csrc/fronts.cpp -o /tmp/asan_front_sens && /tmp/asan_front_sens
// front_sens_tables (front_sens_plan.cpp: the rhs-only assembly streams, the rhs-only extend-add and the homes of the listed
// constraints, derived from a FrontPlan's blob) under ASan + UBSan on a few hundred random plans: the graph families
// of tests/gen.py (random tree with chords, wide band, hub, comb) and its polyline sketch, restated here, 10 ... 400 points, on
// 1 ... 4 workgroups, with random `positions` lists -- and every table checked for what the kernel relies on: offsets inside the
// tables, destinations inside the workgroup's workspace, homes that name the listed constraint.  Host only: no device is touched.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "front_sens_types.hpp"
#include "fronts.hpp"
using namespace ezpz;

static EzpzConstraint con(uint16_t kind, std::initializer_list<uint32_t> ids, double param) {
    EzpzConstraint c;
    std::memset(&c, 0, sizeof(c));
    c.kind = kind;
    int k = 0;
    for (uint32_t id : ids) c.ids[k++] = id;
    c.param = param;
    c.weight = 1.0;
    return c;
}

int main() {
    std::mt19937_64 rng(2024);
    auto below = [&](uint64_t n) { return (uint32_t)(rng() % n); };
    const uint16_t DISTANCE = 2, VERTICAL_DISTANCE = 4, HORIZONTAL_DISTANCE = 5, FIXED = 9;
    size_t tried = 0, planned = 0, tables = 0, words = 0, listed = 0, rhs_entries = 0, ext_entries = 0;
    for (int trial = 0; trial < 320; ++trial) {
        const int family = trial % 5;  // tree, band, hub, comb, polyline
        const uint32_t npts = 10 + below(trial % 8 == 0 ? 391 : 111);
        std::vector<EzpzConstraint> cs = {con(FIXED, {0}, 0.0), con(FIXED, {1}, 0.0)};
        for (uint32_t i = 1; i < npts; ++i) {
            uint32_t a, b;
            if (family == 0)
                a = below(i), b = below(i);
            else if (family == 1)
                a = i - 1, b = i > 2 + below(11) ? i - 2 - below(11) : 0;
            else if (family == 2)
                a = 0, b = i - 1;
            else if (family == 3)
                a = i % 5 ? i - 1 : (i >= 5 ? i - 5 : 0), b = i % 5 ? (i >= 2 ? i - 2 : 0) : (i >= 10 ? i - 10 : 0);
            else
                a = i - 1, b = i > 2 ? i - 2 - below(2) : 0;
            const double len = 0.6 + (double)below(1000) / 700.0;
            cs.push_back(con(DISTANCE, {2 * i, 2 * i + 1, 2 * a, 2 * a + 1}, len));
            if (b != a)
                cs.push_back(below(2) ? con(DISTANCE, {2 * i, 2 * i + 1, 2 * b, 2 * b + 1}, len + 0.3)
                                      : con(HORIZONTAL_DISTANCE, {2 * i, 2 * i + 1, 2 * b, 2 * b + 1}, 0.5 * len));
            else
                cs.push_back(con(VERTICAL_DISTANCE, {2 * i, 2 * i + 1, 2 * a, 2 * a + 1}, 0.5 * len));
        }
        const size_t n_vars = 2 * (size_t)npts;
        FrontOptions opt;
        opt.wgs = 1 + below(4);
        if (trial % 6 == 0) opt.lds_bytes = 64 * 1024;
        FrontPlan plan;
        ++tried;
        if (!front_plan_build(cs.data(), cs.size(), n_vars, opt, plan)) continue;
        ++planned;
        // a random list: every constraint here has a parameter; a shuffled part of them, sometimes one, sometimes all
        std::vector<uint32_t> pos(cs.size());
        for (uint32_t i = 0; i < pos.size(); ++i) pos[i] = i;
        std::shuffle(pos.begin(), pos.end(), rng);
        pos.resize(trial % 4 == 0 ? pos.size() : trial % 4 == 1 ? 1 : 1 + below(pos.size()));
        std::vector<uint32_t> T;
        if (!front_sens_tables(plan, pos.data(), pos.size(), T)) {
            std::printf("trial %d: no tables for a plan of %u workgroups\n", trial, plan.n_wgs);
            return 1;
        }
        ++tables;
        words += T.size();
        listed += pos.size();
        // ---- what the kernel relies on --------------------------------------------------------------------------------------------------
        const FrontSensHead& H = *reinterpret_cast<const FrontSensHead*>(T.data());
        bool ok = H.n_wgs == plan.n_wgs && H.n_param == pos.size() && H.n_words == T.size() && H.w_home + 2 * pos.size() == T.size();
        const FrontWg* wgs = reinterpret_cast<const FrontWg*>(plan.blob.data());
        for (uint32_t g = 0; ok && g < plan.n_wgs; ++g) {
            const FrontSensWg& W = *reinterpret_cast<const FrontSensWg*>(&T[4 + 4 * g]);
            const FrontWg& P = wgs[g];
            const uint32_t room = P.ws_doubles - P.l_panels;
            ok = W.n_fronts == P.n_fronts && W.w_asm_offs + W.asm_trips <= T.size() && W.w_ext + 2 * W.n_fronts <= T.size();
            for (uint32_t t = 0; ok && t < W.asm_trips; ++t) {
                const uint32_t at = T[W.w_asm_offs + t];
                ok = at + 64 <= T.size();
                if (!ok) break;
                const uint32_t w = T[at] >> 24;
                ok = at + 64 * (1 + (size_t)w) <= T.size();
                for (uint32_t l = 0; ok && l < 64; ++l) {
                    const uint32_t hdr = T[at + l];
                    ok = (hdr >> 24) == w && (hdr & FASM_RHS) && (hdr & 0xFFFFu) < room;
                    for (uint32_t q = 0; ok && q < w; ++q) {
                        const uint32_t op = T[at + 64 * (1 + q) + l];
                        ok = (op & 0xFFFFu) <= P.zj && (op >> 16) <= P.n_rows;
                    }
                    if (!(hdr & FASM_NOP)) ++rhs_entries;
                }
            }
            for (uint32_t k = 0; ok && k < W.n_fronts; ++k) {
                uint32_t at = T[W.w_ext + 2 * k];
                for (uint32_t t = 0; ok && t < T[W.w_ext + 2 * k + 1]; ++t) {
                    ok = at + 64 <= T.size();
                    if (!ok) break;
                    const uint32_t v = T[at] >> 24;
                    ok = at + 64 * (1 + (size_t)v) <= T.size();
                    for (uint32_t l = 0; ok && l < 64; ++l) {
                        const uint32_t hdr = T[at + l];
                        ok = (hdr >> 24) == v && (hdr & 0xFFFFu) < room;
                        for (uint32_t q = 0; ok && q < v; ++q) {
                            const uint32_t x = T[at + 64 * (1 + q) + l];
                            ok = (x & 0xFFFFu) < room && (x >> 16) < room;
                        }
                        if (!(hdr & FASM_NOP)) ++ext_entries;
                    }
                    at += 64 * (1 + v);
                }
            }
        }
        for (size_t j = 0; ok && j < pos.size(); ++j) {
            const uint32_t hw = T[H.w_home + 2 * j], hi = T[H.w_home + 2 * j + 1];
            ok = hw < plan.n_wgs && hi < wgs[hw].n_cons && reinterpret_cast<const DevCon*>(plan.blob.data() + wgs[hw].o_cons)[hi].pos == pos[j];
        }
        if (!ok) {
            std::printf("trial %d: a table entry is out of range (%u workgroups, %zu listed)\n", trial, plan.n_wgs, pos.size());
            return 1;
        }
    }
    std::printf("systems %zu, frontal plans %zu, tables %zu (%zu words, %zu listed constraints, %zu rhs assembly entries, %zu rhs extend-add entries): all in range\n",
                tried, planned, tables, words, listed, rhs_entries, ext_entries);
    return 0;
}
