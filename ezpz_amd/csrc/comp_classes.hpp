// What the two halves of the component planner share: comp_program.cpp (the plans: components, classes, layouts, blobs, the lane
// and batch plans, the overlay) and comp_source.cpp (the HIP source text of the run-time compiled kernels).  Internal: the public
// declarations are comp_program.hpp's.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "comp_program.hpp"
#include "program.hpp"

namespace ezpz {

// (views into two arrays shared by all components: a request of 1500 components is analysed on the path of a solve() call)
struct Span {
    const uint32_t* b = nullptr;
    uint32_t n = 0;
    size_t size() const { return n; }
    const uint32_t* begin() const { return b; }
    const uint32_t* end() const { return b + n; }
    uint32_t operator[](size_t i) const { return b[i]; }
};
struct Component {
    Span verts;  // caller's variable ids, ascending
    Span cons;   // caller's constraint positions, ascending
};

struct ClassLayout {  // what every chunk of a class shares (copied into its CompChunk)
    uint32_t nv = 0, m = 0, zj = 0, ncons = 0, n_ops = 0, ops_off = 0, cons_off = 0;
    uint32_t rows_p = 0, o_d = 0, o_r0 = 0, o_r1 = 0, o_j = 0, o_wm = 0, s_l = 0;
    uint32_t ninst_pad = 0, ids_off = 0, par_off = 0, pos_off = 0, ovl_off = 0;
};

struct Class {
    ClassLayout H;
    uint32_t rep = 0;                 // representative component
    std::vector<uint32_t> instances;  // components of this class, in order of their first variable
    Program Q;                        // symbolic phase of the representative, class-internal numbering
    bool linear = true;
    bool consts_f32 = true;
    std::vector<double> jconst;       // linear classes: the (constant) Jacobian value of every slot
    uint32_t cost = 1;
};

inline std::string S(uint64_t v) { return std::to_string(v); }

// ---- comp_source.cpp ----
// What a wavefront runs in the class-specialised kernel of a component plan, as the slot choice left it (comp_program.cpp:
// CompPlanner): `waves` wavefronts per workgroup, `wgs` workgroups per system, slots_k[k] slots of class k on every wavefront
// (`vgprs` registers of state in all); `contiguous`: every wavefront's variables are one run of the caller's.
struct CompKernelShape {
    uint32_t waves = 0, wgs = 1;
    std::vector<uint32_t> slots_k;
    uint64_t vgprs = 0;
    bool unit_weights = true, contiguous = false;
};
// The whole source of that kernel: one struct per class (Cls<k>: its sweeps and its linear solve as straight-line code), then the entries (ezpz_jit_solve, _one, _fast, _fast_b, _list).
std::string comp_kernel_source(const std::vector<Class>& classes, const CompKernelShape& shape);
// One lane per system: the class (the prefix the wavefront form shares) and the source with its two entries (ezpz_jit_lane, _one).
std::string lane_class_source(const Class& cl, const EzpzConstraint* cs);
std::string lane_kernel_source(const std::string& cls, bool unit_weights);
// One wavefront per system (ezpz_jit_wave), or empty when the class does not fit that form.
std::string wave_kernel_source(const std::string& cls, const Class& cl, const EzpzConstraint* cs, bool unit_weights);

}  // namespace ezpz
