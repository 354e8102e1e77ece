// Plain-data types of the dimension sensitivities on the FRONTAL shape: the tables the host derives from a
// FrontPlan for a `positions` list (front_sens_plan.cpp) and the argument block of front_sens_kernel (front_sens_kernel.hip.hpp).
// Nothing of the plan blob changes; the tables live in a buffer of their own beside it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "front_types.hpp"

namespace ezpz {

// The tables: one array of 32-bit words, every offset a WORD index from its start.
//   [0 .. 3]          FrontSensHead
//   [4 + 4 g ..]      FrontSensWg of workgroup g
//   per workgroup     the RHS-ONLY ASSEMBLY STREAM: asm_trips word indices of its trips, then the trips -- the FASM_RHS entries of
//                     the plan's assembly stream alone, in its encoding (64 header words, w x 64 operand words, w = header >> 24,
//                     trips sorted by w, entries in the plan's order; padding entries are FASM_NOP with operands (zj, n_rows));
//                     the RHS-ONLY EXTEND-ADD: per front two words (first trip, trips), and the trips -- the entries of the
//                     front's source stream whose destination is row S of its panel or the last row of its update matrix, in
//                     that stream's order and encoding (64 header words, v x 64 source words, v = header >> 24; the sources are
//                     elements of the last rows of its local children's update matrices; padding sources are 0)
//   w_home            per listed position two words: the workgroup that evaluates the constraint, its index in that
//                     workgroup's constraint table
struct FrontSensHead {
    uint32_t n_wgs, n_param, w_home, n_words;
};
struct FrontSensWg {
    uint32_t w_asm_offs, asm_trips;  // the rhs-only assembly stream: word index of the list of its trips, how many
    uint32_t w_ext, n_fronts;        // the rhs-only extend-add: word index of the fronts' (first trip, trips) pairs
};
static_assert(sizeof(FrontSensHead) == 16 && sizeof(FrontSensWg) == 16, "front sens table layout");

struct FrontPlan;
// False when a listed constraint is not evaluated by exactly one workgroup of the plan (positions are checked by the caller).
bool front_sens_tables(const FrontPlan& plan, const uint32_t* positions, size_t n_param, std::vector<uint32_t>& out);

// The argument block of front_sens_kernel: FrontArgs (plan, n_wgs, n_vars, x0 = the values, batch = SYSTEMS, the LDS carve-up,
// the scratch) and the request.  A type of its own, like FrontParArgs: the builds of front.hip and front_params.hip never see it.
struct FrontSensArgs : FrontArgs {
    const double* params;      // [batch][n_param] or null: the system's own values
    const uint32_t* par_slot;  // per CALLER position: the place in the list, or kNoParamSlot
    const uint32_t* tabs;      // the tables above
    double* S;                 // [batch][n_param][n_vars], zero-filled by the host
    uint32_t* sens_status;     // [batch], zero-filled: 1 a pivot was not positive, 2 a wait between workgroups ran out
    uint32_t* deg;             // [batch], zero-filled, or null
    double lambda;
    uint32_t n_param;
    uint32_t rhs_per_item;      // right-hand sides of one work item (one factorisation)
    uint32_t items_per_system;  // ceil(n_param / rhs_per_item): item = system x items_per_system + chunk
    uint32_t pad;
};

}  // namespace ezpz
