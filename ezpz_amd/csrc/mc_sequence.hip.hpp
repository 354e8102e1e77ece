// The low-discrepancy draws of the Monte-Carlo entries (include/ezpz_amd.h: THE DRAW, EZPZ_MC_SEQUENCE): the Sobol'
// point of (sample, dimension) from the Joe-Kuo direction numbers -- evaluated directly, or stepped from the sample before it --
// the seed-keyed digital shift, the 32-bit grid value u and Wichura's inverse of the normal distribution.  Every function is one
// __host__ __device__ body; the table is one list (mc_sequence_table.hpp) behind the host's array and the device's copy.
//
// Built without contraction, like everything around the sampler: the point, the shift, u and the central branch of the inverse are
// integer arithmetic and rounded + - * / alone, so they have the same bits on the host and on the device.  Only the inverse's two
// tail branches (log, sqrt) can differ in the last bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "mc_sequence_table.hpp"

namespace ezpz {
namespace mc {

#define EZPZ_SEQ_HD __host__ __device__ inline

constexpr uint32_t kSequenceDims = EZPZ_MC_SEQUENCE_DIMS, kSequenceBits = 32;
constexpr uint32_t kShiftAttempt = 0xFFFFFFFFu;  // the attempt word of the shift's counter: no plain draw reaches it

static const uint32_t kSequenceHost[kSequenceDims][kSequenceBits] = {EZPZ_MC_SEQUENCE_TABLE};
#ifdef __HIPCC__
static __constant__ const uint32_t kSequenceDevice[kSequenceDims][kSequenceBits] = {EZPZ_MC_SEQUENCE_TABLE};
#endif

// the 32 direction numbers of dimension j < kSequenceDims, on whichever side this is compiled for
EZPZ_SEQ_HD const uint32_t* sequence_row(uint32_t j) {
#ifdef __HIP_DEVICE_COMPILE__
    return kSequenceDevice[j];
#else
    return kSequenceHost[j];
#endif
}

// x(b): the XOR of v[c] over the set bits c of the Gray code of b
EZPZ_SEQ_HD uint32_t sequence_point(const uint32_t* v, uint32_t b) {
    uint32_t x = 0;
    for (uint32_t g = b ^ (b >> 1), c = 0; g; g >>= 1, ++c)
        if (g & 1u) x ^= v[c];
    return x;
}

// x(b) from x(b - 1), b >= 1: the Gray codes of b - 1 and b differ in the bit ctz(b)
EZPZ_SEQ_HD uint32_t sequence_step(const uint32_t* v, uint32_t x_before, uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return x_before ^ v[__builtin_ctz(b)];
#else
    uint32_t c = 0;
    while (!((b >> c) & 1u)) ++c;
    return x_before ^ v[c];
#endif
}

// u = (k + 0.5) * 2^-32 for the shifted point k: exact in a double, inside (0, 1)
EZPZ_SEQ_HD double sequence_unit(uint32_t k) { return ((double)k + 0.5) * 2.3283064365386962890625e-10; }

// Phi^-1(p), 0 < p < 1: M. J. Wichura, "Algorithm AS 241: the percentage points of the normal distribution", Applied Statistics 37
// (1988) 477-484, routine PPND16 (relative error about 1e-16).  |p - 0.5| <= 0.425 is a rational polynomial of + - * / alone.
EZPZ_SEQ_HD double normal_inverse(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                              1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                              4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    double r = q <= 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    double num, den;
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                   1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                   1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                 2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                   2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                   7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                 5.99832206555887937690e-1) * r + 1.0);
    }
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

}  // namespace mc
}  // namespace ezpz
