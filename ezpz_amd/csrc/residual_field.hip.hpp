// Residual field: the residual magnitude of one constraint, or of a whole system, as a 2-D scalar field while two
// variables sweep a viewport (the reference's residual_viz module, ezpz/src/residual_viz.rs, evaluated on the device).
//
// Two launches.  field_prep_kernel (one workgroup) walks the system's constraint table once: the constraints that use a
// swept variable -- or the one selected constraint -- become a compact list in the caller's constraint order, their ids
// replaced by value SLOTS (0 = the lane's x, 1 = its y, 2 + 8 * record + k = a base value gathered beside the records),
// and every other constraint is evaluated at the base values and summed into C, which no pixel changes.
// field_kernel then puts one lane on each run of 4 consecutive pixels of a row: the list and its values are staged in
// LDS once per workgroup (every lane reads the same record: a broadcast), `con_residual` takes its values through the
// slot accessor, so no per-pixel value vector exists anywhere, and a lane's results leave as one 96-bit store of colour
// and two 128-bit stores of magnitude.
//
// Semantics (bit for bit reproducible; built with -ffp-contract=off like every evaluator):
//   pixel centre      x = x_min + (x_max - x_min) * (px + 0.5) / width, likewise y        residual_viz.rs:58-62
//   residuals         unweighted; a degenerate guard leaves 0 and the pixel counts as degenerate
//   one constraint    |r0|, or sqrt(r0*r0 + r1*r1) for a kind of two rows                 :240, :294
//   all constraints   sqrt(C + S), S = 0.0 + r0*r0 (+ r1*r1) ... over the listed constraints in the caller's order
//   colour            residual_colour below                                               :72-81
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "constraint_eval.hip.hpp"
#include "grid_ops.hip.hpp"
#include "kinds.hpp"
#include "lm_kernel.hip.hpp"

namespace ezpz {

// mag_to_pixel, residual_viz.rs:72-81: turquoise below the threshold, else rings of the fractional part.  The grey of a
// magnitude that is not finite is 0 (inf - inf = NaN, and Rust's `as u8` of NaN is 0); NaN < 0.08 is false.
__host__ __device__ inline void residual_colour(double mag, uint32_t& r, uint32_t& g, uint32_t& b) {
    if (mag < 0.08) {
        r = 64;
        g = 224;
        b = 208;
        return;
    }
    uint32_t grey = 0;
    if (mag <= 1.7976931348623157e308) {  // finite (NaN compares false)
        const double fractional = mag - trunc(mag);
        grey = (uint32_t)round(255.0 - fractional * 255.0);  // in (0, 255]: halves away from zero
    }
    r = g = b = grey;
}

struct FieldHeader {
    double c_sum;           // C: the constraints no swept variable touches, at the base values
    uint32_t n_list;        // constraints evaluated per pixel
    uint32_t heavy;         // one of them is not of a linear kind
    uint32_t c_degenerate;  // a guard fired among the constraints of C: every pixel counts as degenerate
    uint32_t pad;
};

constexpr uint32_t kFieldLdsCons = 96;  // records (and their 8 values each) staged in LDS; a longer list goes on in global memory

struct FieldArgs {
    ProgramView p;
    const double* x_base;  // caller's numbering
    uint32_t var_x, var_y;
    long long sel;  // position in the caller's constraint list, -1: all
    FieldHeader* hdr;
    DevCon* recs;            // [n_cons]
    double* vals;            // [n_cons][8]
    uint32_t* rank;          // [n_cons], by position
    uint32_t* ci_of_pos;     // [n_cons]
    unsigned long long* deg;  // degenerate pixels (zeroed by the first launch)
    EzpzViewport vp;
    double* mag;   // optional
    uint8_t* rgb;  // optional
    uint32_t wide;  // width % 4 == 0 and both outputs aligned for the vector stores
};

namespace dev {

constexpr uint64_t pack_n_ids(int from) {
    uint64_t v = 0;
    for (int k = 0; k < 16 && from + k < 25; ++k) v |= (uint64_t)kKinds[from + k].n_ids << (4 * k);
    return v;
}
constexpr uint64_t kNIdsLo = pack_n_ids(0), kNIdsHi = pack_n_ids(16);
__device__ __forceinline__ uint32_t field_n_ids(uint32_t kind) {
    return (uint32_t)(((kind < 16 ? kNIdsLo : kNIdsHi) >> (4 * (kind & 15u))) & 15u);
}
// kind_is_linear (kinds.hpp) for device code
constexpr uint32_t kLinearKinds = (1u << EZPZ_FIXED) | (1u << EZPZ_SCALAR_EQUAL) | (1u << EZPZ_VERTICAL) | (1u << EZPZ_HORIZONTAL) |
                                  (1u << EZPZ_VERTICAL_DISTANCE) | (1u << EZPZ_HORIZONTAL_DISTANCE) | (1u << EZPZ_CIRCLE_RADIUS) |
                                  (1u << EZPZ_POINTS_COINCIDENT) | (1u << EZPZ_MIDPOINT);

// values of the program's internal numbering out of the caller's vector
struct BaseValues {
    const double* x;
    const uint32_t* var_of;
    __device__ __forceinline__ double operator[](uint32_t id) const { return x[var_of[id]]; }
};

// values by slot: the lane's own point, else a base value (LDS for the staged records, global memory behind them)
struct SlotValues {
    double x, y;
    const double* staged;
    const double* rest;
    __device__ __forceinline__ double operator[](uint32_t slot) const {
        if (slot == 0) return x;
        if (slot == 1) return y;
        const uint32_t k = slot - 2;
        return k < kFieldLdsCons * 8 ? staged[k] : rest[k];
    }
};

}  // namespace dev

static __device__ __forceinline__ DevCon field_load(const ProgramView& v, const Prog<uint32_t>& P, uint32_t ci, uint32_t& pos) {
    DevCon c;
    if (v.packed) {
        c = load_packed(P.pcons, P.con_weight, ci, true);
        pos = P.con_pos[ci];
    } else {
        c = load_con(P.cons + ci);
        pos = c.pos;
    }
    return c;
}

static __global__ void __launch_bounds__(256) field_prep_kernel(const FieldArgs a) {
    using namespace dev;
    __shared__ double part[256];
    __shared__ uint32_t count[256];
    __shared__ uint32_t heavy, c_deg;
    const Prog<uint32_t> P = make_prog<uint32_t>(a.p, a.p.base, a.p.base);
    const uint32_t t = threadIdx.x, n = a.p.n_cons;
    if (t == 0) heavy = c_deg = 0;
    __syncthreads();
    const BaseValues base{a.x_base, P.var_of};
    double sum = 0.0;
    for (uint32_t ci = t; ci < n; ci += 256) {
        uint32_t pos;
        const DevCon c = field_load(a.p, P, ci, pos);
        bool listed;
        if (a.sel >= 0) {
            listed = pos == (uint32_t)a.sel;
        } else {
            listed = false;
            const uint32_t k_ids = field_n_ids(c.kind);
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                const uint32_t id = k < k_ids ? P.var_of[c.ids[k]] : 0xFFFFFFFFu;
                listed = listed || id == a.var_x || id == a.var_y;
            }
        }
        a.rank[pos] = listed ? 1u : 0u;
        a.ci_of_pos[pos] = ci;
        if (listed) {
            if (!((kLinearKinds >> c.kind) & 1u)) atomicOr(&heavy, 1u);
        } else if (a.sel < 0) {
            double r0, r1;
            if (con_residual<false>(c, base, r0, r1)) atomicOr(&c_deg, 1u);
            sum = sum + r0 * r0;
            if (c.nrows > 1) sum = sum + r1 * r1;
        }
    }
    // C: the lanes' sums folded in a fixed tree (the same bits for the same system and base values, whatever the viewport)
    part[t] = sum;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (t < s) part[t] = part[t] + part[t + s];
        __syncthreads();
    }
    // the list in the caller's order: lane t ranks positions [t * chunk, (t + 1) * chunk)
    const uint32_t chunk = (n + 255u) / 256u;
    const uint32_t p0 = min(t * chunk, n), p1 = min(p0 + chunk, n);
    uint32_t mine = 0;
    for (uint32_t p = p0; p < p1; ++p) mine += a.rank[p];
    count[t] = mine;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t k = 0; k < 256; ++k) {
        const uint32_t v = count[k];
        before += k < t ? v : 0u;
        total += v;
    }
    for (uint32_t p = p0; p < p1; ++p) {
        if (!a.rank[p]) continue;
        const uint32_t slot = before++;
        uint32_t pos;
        DevCon c = field_load(a.p, P, a.ci_of_pos[p], pos);
        const uint32_t k_ids = field_n_ids(c.kind);
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t id = k < k_ids ? P.var_of[c.ids[k]] : 0u;
            a.vals[(size_t)slot * 8 + k] = k < k_ids ? a.x_base[id] : 0.0;
            c.ids[k] = (k < k_ids && id == a.var_x) ? 0u : (k < k_ids && id == a.var_y) ? 1u : 2u + slot * 8u + k;
        }
        a.recs[slot] = c;
    }
    if (t == 0) {
        FieldHeader h;
        h.c_sum = part[0];
        h.n_list = total;
        h.heavy = heavy;
        h.c_degenerate = c_deg;
        h.pad = 0;
        *a.hdr = h;
        *a.deg = 0ull;
    }
}

struct __attribute__((packed, aligned(4))) FieldRgb4 {
    uint32_t w0, w1, w2;  // 4 pixels, 12 bytes
};

// LINEAR_ONLY: every listed constraint is of a linear kind (the evaluator is built without the other sixteen bodies and the
// four pixels of a lane are unrolled); the full evaluator keeps one copy of its switch and loops over the pixels.  The host
// enqueues both where it cannot know which applies; the one the list is not for returns at once.
template <bool LINEAR_ONLY>
static __global__ void __launch_bounds__(256) field_kernel(const FieldArgs a) {
    using namespace dev;
    __shared__ DevCon s_recs[kFieldLdsCons];
    __shared__ double s_vals[kFieldLdsCons * 8];
    const FieldHeader h = *a.hdr;
    if ((h.heavy != 0u) == LINEAR_ONLY) return;
    const uint32_t t = threadIdx.x;
    const uint32_t n_list = h.n_list, n_staged = min(n_list, kFieldLdsCons);
    for (uint32_t i = t; i < n_staged * 5; i += 256) reinterpret_cast<uint4*>(s_recs)[i] = reinterpret_cast<const uint4*>(a.recs)[i];
    for (uint32_t i = t; i < n_staged * 8; i += 256) s_vals[i] = a.vals[i];
    __syncthreads();

    const uint32_t W = a.vp.width, H = a.vp.height;
    const uint32_t runs_per_row = (W + 3u) / 4u, total = runs_per_row * H;
    const double span_x = a.vp.x_max - a.vp.x_min, span_y = a.vp.y_max - a.vp.y_min;
    const double wd = (double)W, hd = (double)H;
    const bool single = a.sel >= 0;
    uint32_t n_deg = 0;
    for (uint32_t run = blockIdx.x * 256u + t; run < total; run += gridDim.x * 256u) {
        const uint32_t row = run / runs_per_row, px0 = (run - row * runs_per_row) * 4u;
        SlotValues X;
        X.staged = s_vals;
        X.rest = a.vals;
        X.y = a.vp.y_min + span_y * ((double)row + 0.5) / hd;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
        constexpr int kUnroll = LINEAR_ONLY ? 4 : 1;
#pragma unroll kUnroll
        for (uint32_t j = 0; j < 4; ++j) {
            X.x = a.vp.x_min + span_x * ((double)(px0 + j) + 0.5) / wd;
            double s = 0.0, m = 0.0;
            bool deg = h.c_degenerate != 0u;
            for (uint32_t i = 0; i < n_list; ++i) {
                const DevCon c = i < kFieldLdsCons ? s_recs[i] : load_con(a.recs + i);
                double r0, r1;
                deg = con_residual<LINEAR_ONLY>(c, X, r0, r1) || deg;
                if (single) {
                    m = c.nrows > 1 ? sqrt(r0 * r0 + r1 * r1) : fabs(r0);
                } else {
                    s = s + r0 * r0;
                    if (c.nrows > 1) s = s + r1 * r1;
                }
            }
            if (!single) m = sqrt(h.c_sum + s);
            n_deg += (deg && px0 + j < W) ? 1u : 0u;
            m0 = j == 0 ? m : m0;
            m1 = j == 1 ? m : m1;
            m2 = j == 2 ? m : m2;
            m3 = j == 3 ? m : m3;
        }
        const size_t pix = (size_t)row * W + px0;
        if (a.wide) {
            if (a.mag) {
                double2* dst = reinterpret_cast<double2*>(a.mag + pix);
                dst[0] = make_double2(m0, m1);
                dst[1] = make_double2(m2, m3);
            }
            if (a.rgb) {
                uint32_t r0, g0, b0, r1, g1, b1, r2, g2, b2, r3, g3, b3;
                residual_colour(m0, r0, g0, b0);
                residual_colour(m1, r1, g1, b1);
                residual_colour(m2, r2, g2, b2);
                residual_colour(m3, r3, g3, b3);
                FieldRgb4 q;
                q.w0 = r0 | g0 << 8 | b0 << 16 | r1 << 24;
                q.w1 = g1 | b1 << 8 | r2 << 16 | g2 << 24;
                q.w2 = b2 | r3 << 8 | g3 << 16 | b3 << 24;
                *reinterpret_cast<FieldRgb4*>(a.rgb + pix * 3) = q;
            }
        } else {
            // a width that is no multiple of 4 (rows start on any byte), or outputs the caller did not align: pixel by pixel
            const double m[4] = {m0, m1, m2, m3};
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                if (px0 + j >= W) break;
                if (a.mag) a.mag[pix + j] = m[j];
                if (a.rgb) {
                    uint32_t r, g, b;
                    residual_colour(m[j], r, g, b);
                    uint8_t* dst = a.rgb + (pix + j) * 3;
                    dst[0] = (uint8_t)r;
                    dst[1] = (uint8_t)g;
                    dst[2] = (uint8_t)b;
                }
            }
        }
    }
    // one atomic per wavefront that saw a degenerate pixel
    for (int off = 32; off > 0; off >>= 1) n_deg += __shfl_down(n_deg, off, 64);
    if ((t & 63u) == 0 && n_deg) atomicAdd(a.deg, (unsigned long long)n_deg);
}

}  // namespace ezpz
