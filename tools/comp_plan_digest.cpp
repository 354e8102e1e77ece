// g++ -std=c++17 -O1 -Iezpz_amd/csrc -Iinclude tools/comp_plan_digest.cpp ezpz_amd/csrc/comp_program.cpp ezpz_amd/csrc/comp_source.cpp ezpz_amd/csrc/program.cpp -o /tmp/comp_plan_digest
// Pins what the component planner outputs (tests/test_comp_plan_cpu.py): one line per case with a 64-bit digest of every output of
// comp_plan_build (blob, generated source, scalar fields, comp_param_overlay for a fixed pattern), lane_plan_build (both sources,
// scalars) and batch_plan_build (blob, scalars), plus the properties of the case the test counts.  The outputs are a pure function of
// the request, CompLimits and the EZPZ_JIT_* switches, which are read once per process: one run per setting.
//   comp_plan_digest [--trials N] [--dump DIR] [--time N] [NAME:FILE:N_VARS ...]
// Cases: N seeded random block systems (the generator and seed of tools/asan_comp_plan.cpp; the first block topology of each, on its
// own, goes through the lane and batch builders), a block system whose Jacobian constants are not f32-exact, a hub, and every FILE: a raw
// EzpzConstraint array as numpy's records.tofile() writes it.
//   --dump DIR   also writes every blob and source as a file: `diff -r` of two builds' dumps shows where a digest moved
//   --time N     instead: N timed builds of every FILE's plan (component plan if it has one, else lane plan), min / median / max
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "comp_program.hpp"
using namespace ezpz;

namespace {

struct Hash {  // FNV-1a, 64 bits
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    }
    void u64(uint64_t v) { bytes(&v, 8); }
};
uint64_t digest(const void* p, size_t n) {
    Hash h;
    h.u64(n);
    h.bytes(p, n);
    return h.h;
}
uint64_t digest(const std::vector<uint32_t>& v) { return digest(v.data(), v.size() * 4); }
uint64_t digest(const std::string& s) { return digest(s.data(), s.size()); }

std::string g_dump;
void dump(const std::string& name, const char* what, const void* p, size_t n) {
    if (g_dump.empty()) return;
    const std::string path = g_dump + "/" + name + "." + what;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, n, f) != n) std::fprintf(stderr, "cannot write %s\n", path.c_str()), std::exit(2);
    std::fclose(f);
}
void dump(const std::string& name, const char* what, const std::vector<uint32_t>& v) { dump(name, what, v.data(), v.size() * 4); }
void dump(const std::string& name, const char* what, const std::string& s) { dump(name, what, s.data(), s.size()); }

bool has(const std::string& s, const char* needle) { return s.find(needle) != std::string::npos; }

void comp_case(const std::string& name, const std::vector<EzpzConstraint>& cs, size_t n_vars, const CompLimits& lim) {
    CompPlan p;
    if (!comp_plan_build(cs.data(), cs.size(), n_vars, lim, p)) {
        std::printf(" comp=rejected");
        return;
    }
    std::vector<uint32_t> slot_of_pos(cs.size()), overlay;
    for (size_t i = 0; i < cs.size(); ++i) slot_of_pos[i] = i % 3 == 1 ? 0xFFFFFFFFu : (uint32_t)((i * 2654435761ull) % 11);
    comp_param_overlay(p, slot_of_pos.data(), overlay);
    const uint64_t scalars[] = {p.o_waves, p.o_chunks, p.n_waves, p.n_chunks, p.n_classes, p.n_instances, p.linear, p.unit_weights,
                                p.rows_persistent, p.scratch_rows, p.lds_bytes, p.ovl_words, p.n_vars, p.n_cons, p.n_rows, p.max_levels,
                                p.zj, p.za, p.zl, p.jit_waves, p.jit_slots, p.o_jit_slots, p.o_jit_ranges, p.jit_wgs, p.interpretable};
    std::string text;
    for (uint64_t v : scalars) text += std::to_string(v) + "\n";
    // (what the test counts: interpretable, workgroups per system, wavefront ranges, a non-linear class, weights, and linear classes
    // whose constants keep the plan off the linear build)
    const bool nonlinear = has(p.jit_source, "LINEAR = false");
    std::printf(" comp=%016" PRIx64 ",%016" PRIx64 ",%016" PRIx64 ",%016" PRIx64 " interp=%d wgs=%u ranges=%d nonlinear=%d unit=%d inexact=%d", digest(p.blob),
                digest(p.jit_source), digest(text), digest(overlay), (int)p.interpretable, p.jit_wgs, (int)(p.o_jit_ranges != 0), (int)nonlinear,
                (int)p.unit_weights, (int)(!p.jit_source.empty() && !nonlinear && !p.linear));
    dump(name, "comp.blob", p.blob);
    dump(name, "comp.hip", p.jit_source);
    dump(name, "comp.scalars", text);
    dump(name, "comp.overlay", overlay);
}

void lane_batch_case(const std::string& name, const std::vector<EzpzConstraint>& cs, size_t n_vars) {
    LanePlan l;
    if (lane_plan_build(cs.data(), cs.size(), n_vars, l)) {
        const std::string text = std::to_string(l.n_vars) + "\n" + std::to_string(l.n_cons) + "\n" + std::to_string(l.n_rows) + "\n" + std::to_string(l.unit_weights) + "\n";
        std::printf(" lane=%016" PRIx64 ",%016" PRIx64 ",%016" PRIx64 " wave=%s", digest(l.jit_source), digest(l.wave_source), digest(text),
                    l.wave_source.empty() ? "none" : has(l.wave_source, "HAS_TAIL_WAVE = true") ? "across" : "serial");
        dump(name, "lane.hip", l.jit_source);
        dump(name, "wave.hip", l.wave_source);
        dump(name, "lane.scalars", text);
    } else {
        std::printf(" lane=rejected");
    }
    BatchPlan b;
    if (batch_plan_build(cs.data(), cs.size(), n_vars, b)) {
        const uint64_t scalars[] = {b.nv, b.m, b.zj, b.zlo, b.ncons, b.n_ops, b.ops_off, b.cons_off, b.var_off, b.inv_off,
                                    b.o_d, b.o_r, b.o_rn, b.o_j, b.o_dg, b.o_l, b.rows, b.unit_weights};
        std::string text;
        for (uint64_t v : scalars) text += std::to_string(v) + "\n";
        std::printf(" batch=%016" PRIx64 ",%016" PRIx64, digest(b.blob), digest(text));
        dump(name, "batch.blob", b.blob);
        dump(name, "batch.scalars", text);
    } else {
        std::printf(" batch=rejected");
    }
}

EzpzConstraint make_con(uint16_t kind, uint32_t a, uint32_t b, double param, double weight) {
    EzpzConstraint c;
    std::memset(&c, 0, sizeof(c));
    c.kind = kind, c.ids[0] = a, c.ids[1] = b, c.param = param, c.weight = weight;
    return c;
}

// tools/asan_comp_plan.cpp's block systems, draw for draw
void random_cases(int trials) {
    std::mt19937_64 rng(777);
    const uint16_t linear_kinds[] = {0, 1, 2, 3, 4, 5, 7, 8};
    for (int trial = 0; trial < trials; ++trial) {
        const int n_topo = 1 + (int)(rng() % 3);
        struct Topo { int nv; std::vector<EzpzConstraint> cs; };
        std::vector<Topo> topo(n_topo);
        for (auto& t : topo) {
            t.nv = 1 + (int)(rng() % 6);
            const int nc = 1 + (int)(rng() % 6);
            const bool linear = rng() % 3 != 0;
            for (int i = 0; i < nc; ++i) {
                EzpzConstraint c;
                std::memset(&c, 0, sizeof(c));
                c.kind = linear ? linear_kinds[rng() % 8] : (uint16_t)(rng() % 25);
                for (int k = 0; k < 8; ++k) c.ids[k] = (uint32_t)(rng() % t.nv);
                c.param = 1.0 + (double)(rng() % 5);
                c.weight = (rng() % 5) ? 1.0 : 0.25;
                c.tag = (uint8_t)(rng() % 3);
                t.cs.push_back(c);
            }
        }
        const size_t blocks = trial % 7 == 0 ? 20000 + rng() % 40000 : 1 + rng() % 3000;
        std::vector<EzpzConstraint> cs;
        size_t n_vars = 0;
        for (size_t b = 0; b < blocks; ++b) {
            const Topo& t = topo[rng() % n_topo];
            for (EzpzConstraint c : t.cs) {
                for (int k = 0; k < 8; ++k) c.ids[k] += (uint32_t)n_vars;
                cs.push_back(c);
            }
            n_vars += t.nv;
        }
        if (trial % 3 == 0) std::shuffle(cs.begin(), cs.end(), rng);
        CompLimits lim;
        if (trial % 5 == 0) lim.lds_bytes = 64 * 1024;
        const std::string name = "random" + std::to_string(trial);
        std::printf("%s", name.c_str());
        comp_case(name, cs, n_vars, lim);
        lane_batch_case(name, topo[0].cs, (size_t)topo[0].nv);
        std::printf("\n");
    }
}

// 300 blocks of {Fixed x, weight 0.1; ScalarEqual x y, weight 0.3}: every class linear, constants not f32-exact
void inexact_case() {
    std::vector<EzpzConstraint> cs;
    for (uint32_t b = 0; b < 300; ++b) {
        cs.push_back(make_con(EZPZ_FIXED, 2 * b, 0, 1.0 + b, 0.1));
        cs.push_back(make_con(EZPZ_SCALAR_EQUAL, 2 * b, 2 * b + 1, 0.0, 0.3));
    }
    std::printf("inexact");
    comp_case("inexact", cs, 600, CompLimits());
    lane_batch_case("inexact", std::vector<EzpzConstraint>(cs.begin(), cs.begin() + 2), 2);
    std::printf("\n");
}

// a hub: 18 constraints on one variable -- a list too long for the wavefront form (lane plan with an empty wave source)
void hub_case() {
    std::vector<EzpzConstraint> cs;
    for (uint32_t i = 0; i < 18; ++i) cs.push_back(make_con(EZPZ_FIXED, 0, 0, 1.0 + i, 1.0));
    cs.push_back(make_con(EZPZ_SCALAR_EQUAL, 0, 1, 0.0, 1.0));
    std::printf("hub");
    comp_case("hub", cs, 2, CompLimits());
    lane_batch_case("hub", cs, 2);
    std::printf("\n");
}

struct FileCase {
    std::string name;
    std::vector<EzpzConstraint> cs;
    size_t n_vars = 0;
};
FileCase read_case(const std::string& arg) {
    FileCase c;
    const size_t a = arg.find(':'), b = arg.rfind(':');
    if (a == std::string::npos || a == b) std::fprintf(stderr, "expected NAME:FILE:N_VARS, got %s\n", arg.c_str()), std::exit(2);
    c.name = arg.substr(0, a);
    c.n_vars = (size_t)std::strtoull(arg.c_str() + b + 1, nullptr, 10);
    const std::string path = arg.substr(a + 1, b - a - 1);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) std::fprintf(stderr, "cannot read %s\n", path.c_str()), std::exit(2);
    EzpzConstraint rec;
    while (std::fread(&rec, sizeof(rec), 1, f) == 1) c.cs.push_back(rec);
    std::fclose(f);
    return c;
}

void time_case(const FileCase& c, int n) {
    CompPlan p;
    LanePlan l;
    const bool comp = comp_plan_build(c.cs.data(), c.cs.size(), c.n_vars, CompLimits(), p);  // (also the warm-up run)
    if (!comp && !lane_plan_build(c.cs.data(), c.cs.size(), c.n_vars, l)) std::fprintf(stderr, "%s has neither plan\n", c.name.c_str()), std::exit(2);
    std::vector<double> us;
    for (int i = 0; i < n; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        if (comp)
            comp_plan_build(c.cs.data(), c.cs.size(), c.n_vars, CompLimits(), p);
        else
            lane_plan_build(c.cs.data(), c.cs.size(), c.n_vars, l);
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(us.begin(), us.end());
    std::printf("%-14s %-16s runs %3zu  min %10.1f us  median %10.1f us  max %10.1f us\n", c.name.c_str(), comp ? "comp_plan_build" : "lane_plan_build",
                us.size(), us.front(), us[us.size() / 2], us.back());
}

}  // namespace

int main(int argc, char** argv) {
    int trials = 200, timed = 0;
    std::vector<FileCase> files;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--trials" && i + 1 < argc)
            trials = std::atoi(argv[++i]);
        else if (a == "--dump" && i + 1 < argc)
            g_dump = argv[++i];
        else if (a == "--time" && i + 1 < argc)
            timed = std::atoi(argv[++i]);
        else
            files.push_back(read_case(a));
    }
    if (timed > 0) {
        for (const FileCase& c : files) time_case(c, timed);
        return 0;
    }
    random_cases(trials);
    inexact_case();
    hub_case();
    for (const FileCase& c : files) {
        std::printf("%s", c.name.c_str());
        comp_case(c.name, c.cs, c.n_vars, CompLimits());
        lane_batch_case(c.name, c.cs, c.n_vars);
        std::printf("\n");
    }
    return 0;
}
