// Reference dimensions: the value m of `param` at which a record's unweighted residual vanishes at x (for the two kinds with two
// rows and one parameter: the param that minimises the sum of the squares of the rows), and its gradient by the record's ids
// (include/ezpz_amd.h: ezpz_constraint_measure).  Beside the evaluators of constraint_eval.hip.hpp and
// constraint_dparam.hip.hpp whose residuals it inverts -- same guards, same operand order, built with -ffp-contract=off.
// __host__ __device__: the measure kernels (measure.hip.hpp) and ezpz_constraint_measure (host only) share it.
//
//   Fixed, CircleRadius, the two axis distances: the residual without `- param`, constant gradient;
//   Distance, ArcRadius (the mean of its two magnitudes): the gradient has distance_jac's guard (dist < EPS), per row, flag bit 1;
//   the three point-line distances: the residual's expression and guard, the Jacobian's partials (con_jacobian);
//   LinesAtAngle, ArcAngle, PointsAtAngle: theta = atan2(cross(u, v), dot(u, v)) in (-pi, pi] with the residual's u and v, per
//   degree where the tag says so -- the branch cut at +-pi is documented, not smoothed;
//   ArcLength: |u| * rem_euclid(theta(u, w), 2 pi) in [0, 2 pi r), counter-clockwise from start to end (classify_pac) -- cut at 0.
//   (An arc whose end lies on its centre has no direction: its gradient is not finite.  The residual has no guard for it either.)
// Unweighted, in the units of EzpzConstraint::param.  Returns the flags: bit 0 the residual's degenerate guard fired (m = 0 and
// every gradient slot 0 then), bit 1 a gradient guard fired (m valid, the guarded row contributes zeros).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ezpz_amd.h"

namespace ezpz {
namespace measure {

constexpr double EPS = 1e-4;  // lib.rs:43
constexpr double PI = 3.14159265358979323846264338327950288;
constexpr uint32_t kDegenerate = 1u, kGradGuard = 2u;

// Not inlined on the device: hypot / atan2 / fmod bring large OCML bodies whose registers would otherwise be live across every
// branch of the switch (constraint_eval.hip.hpp: rot_for).
#ifdef __HIP_DEVICE_COMPILE__
#define EZPZ_MEASURE_LIBM __device__ __noinline__
#else
#define EZPZ_MEASURE_LIBM __host__ inline
#endif
EZPZ_MEASURE_LIBM double mag2d(double x, double y) { return hypot(x, y); }
// signed_angle (vector.rs:72-74) with a cross product of -0.0 taken as +0.0: opposite arms give +pi whatever their signs
EZPZ_MEASURE_LIBM double angle_between(double ux, double uy, double vx, double vy) {
    return atan2((ux * vy - uy * vx) + 0.0, ux * vx + uy * vy);
}
EZPZ_MEASURE_LIBM double rem_two_pi(double a) {
    const double r = fmod(a, 2.0 * PI);
    return r < 0.0 ? r + 2.0 * PI : r;
}
#undef EZPZ_MEASURE_LIBM

// one Distance row between the points at ids ia, ib into the gradient, scaled by k (distance_jac)
template <class XP>
__host__ __device__ inline double distance_row(const uint32_t* ids, XP xs, int ia, int ib, double k, double* grad, uint32_t& flags) {
    const double x0 = xs[ids[ia]], y0 = xs[ids[ia + 1]], x1 = xs[ids[ib]], y1 = xs[ids[ib + 1]];
    const double dist = mag2d(x0 - x1, y0 - y1);
    if (dist < EPS) {
        flags |= kGradGuard;
        return dist;
    }
    grad[ia] = grad[ia] + ((x0 - x1) / dist) * k;
    grad[ia + 1] = grad[ia + 1] + ((y0 - y1) / dist) * k;
    grad[ib] = grad[ib] + ((-x0 + x1) / dist) * k;
    grad[ib + 1] = grad[ib + 1] + ((-y0 + y1) / dist) * k;
    return dist;
}

// theta(u, v) and its gradient by u and v, times `unit`; true: the residual's guard (lines_at_angle_residual)
__host__ __device__ inline bool angle_of(double ux, double uy, double vx, double vy, double unit, double& m, double* du, double* dv) {
    const double len_u = mag2d(ux, uy), len_v = mag2d(vx, vy);
    if (len_u <= EPS || len_v <= EPS) return true;
    m = angle_between(ux, uy, vx, vy) * unit;
    const double uu = ux * ux + uy * uy, vv = vx * vx + vy * vy;
    du[0] = (uy / uu) * unit;
    du[1] = (-ux / uu) * unit;
    dv[0] = (-vy / vv) * unit;
    dv[1] = (vx / vv) * unit;
    return false;
}

#define XV(i) (xs[ids[(i)]])

template <class XP>
__host__ __device__ inline uint32_t con_measure(uint32_t kind, uint32_t tag, const uint32_t* ids, XP xs, double& m, double* grad) {
    m = 0.0;
#pragma unroll
    for (int s = 0; s < 8; ++s) grad[s] = 0.0;
    const double unit = (tag == EZPZ_ANGLE_OTHER_DEG) ? (180.0 / PI) : 1.0;
    uint32_t flags = 0;
    switch (kind) {
    case EZPZ_FIXED:
        m = XV(0);
        grad[0] = 1.0;
        return 0;
    case EZPZ_CIRCLE_RADIUS:
        m = XV(2);
        grad[2] = 1.0;
        return 0;
    case EZPZ_VERTICAL_DISTANCE:
        m = XV(1) - XV(3);
        grad[1] = 1.0;
        grad[3] = -1.0;
        return 0;
    case EZPZ_HORIZONTAL_DISTANCE:
        m = XV(0) - XV(2);
        grad[0] = 1.0;
        grad[2] = -1.0;
        return 0;
    case EZPZ_DISTANCE:
        m = distance_row(ids, xs, 0, 2, 1.0, grad, flags);
        return flags;
    case EZPZ_ARC_RADIUS: {
        const double d0 = distance_row(ids, xs, 0, 2, 0.5, grad, flags);
        const double d1 = distance_row(ids, xs, 0, 4, 0.5, grad, flags);
        m = (d0 + d1) / 2.0;
        return flags;
    }
    case EZPZ_POINT_LINE_DISTANCE: {
        const double px = XV(0), py = XV(1), lpx = XV(2), lpy = XV(3), lqx = XV(4), lqy = XV(5);
        const double a = lpy - lqy, b = lqx - lpx, cc = (lpx * lqy) - (lqx * lpy);
        const double den = mag2d(a, b);
        if (den < EPS) return kDegenerate;
        const double num = a * px + b * py + cc;
        m = num / den;
        const double t = num / (den * den * den);
        grad[0] = a / den;
        grad[1] = b / den;
        grad[2] = (b * t) + (lqy - py) / den;
        grad[3] = -(a * t) + (px - lqx) / den;
        grad[4] = -(b * t) + (py - lpy) / den;
        grad[5] = (a * t) + (lpx - px) / den;
        return 0;
    }
    case EZPZ_VERTICAL_POINT_LINE_DISTANCE: {
        const double ax = XV(0), ay = XV(1), px = XV(2), py = XV(3), qx = XV(4), qy = XV(5);
        const double dx = qx - px, dy = qy - py;
        if (fabs(dx) <= EPS || (dx * dx + dy * dy) <= EPS * EPS) return kDegenerate;
        m = ay - py - dy * (1.0 / dx) * (ax - px);
        const double pq = px - qx;
        const double inv2 = 1.0 / (pq * pq), inv = 1.0 / pq;
        grad[0] = (-py + qy) * inv;
        grad[1] = 1.0;
        grad[2] = (ax - qx) * (py - qy) * inv2;
        grad[3] = (-ax + qx) * inv;
        grad[4] = -(ax - px) * (py - qy) * inv2;
        grad[5] = (ax - px) * inv;
        return 0;
    }
    case EZPZ_HORIZONTAL_POINT_LINE_DISTANCE: {
        const double ax = XV(0), ay = XV(1), px = XV(2), py = XV(3), qx = XV(4), qy = XV(5);
        const double dx = qx - px, dy = qy - py;
        if (fabs(dy) <= EPS || (dx * dx + dy * dy) <= EPS * EPS) return kDegenerate;
        m = ax - px - dx * (1.0 / dy) * (ay - py);
        const double pq = py - qy;
        const double inv2 = 1.0 / (pq * pq), inv = 1.0 / pq;
        grad[0] = 1.0;
        grad[1] = (-px + qx) * inv;
        grad[2] = (-ay + qy) * inv;
        grad[3] = (ay - qy) * (px - qx) * inv2;
        grad[4] = (ay - py) * inv;
        grad[5] = -(ay - py) * (px - qx) * inv2;
        return 0;
    }
    case EZPZ_LINES_AT_ANGLE: {
        if (tag != EZPZ_ANGLE_OTHER_DEG && tag != EZPZ_ANGLE_OTHER_RAD) return 0;
        double du[2], dv[2];
        if (angle_of(XV(2) - XV(0), XV(3) - XV(1), XV(6) - XV(4), XV(7) - XV(5), unit, m, du, dv)) return kDegenerate;
        grad[0] = -du[0];
        grad[1] = -du[1];
        grad[2] = du[0];
        grad[3] = du[1];
        grad[4] = -dv[0];
        grad[5] = -dv[1];
        grad[6] = dv[0];
        grad[7] = dv[1];
        return 0;
    }
    case EZPZ_ARC_ANGLE:
    case EZPZ_POINTS_AT_ANGLE: {
        // both measure the turn from (ids 2, 3) to (ids 4, 5) about (ids 0, 1)
        if (tag != EZPZ_ANGLE_OTHER_DEG && tag != EZPZ_ANGLE_OTHER_RAD) return 0;
        const double cx = XV(0), cy = XV(1);
        double du[2], dv[2];
        if (angle_of(XV(2) - cx, XV(3) - cy, XV(4) - cx, XV(5) - cy, unit, m, du, dv)) return kDegenerate;
        grad[0] = -(du[0] + dv[0]);
        grad[1] = -(du[1] + dv[1]);
        grad[2] = du[0];
        grad[3] = du[1];
        grad[4] = dv[0];
        grad[5] = dv[1];
        return 0;
    }
    case EZPZ_ARC_LENGTH: {
        const double cx = XV(0), cy = XV(1);
        const double ux = XV(2) - cx, uy = XV(3) - cy, wx = XV(4) - cx, wy = XV(5) - cy;
        const double r2 = ux * ux + uy * uy;
        if (r2 <= EPS * EPS) return kDegenerate;
        const double r = sqrt(r2);
        const double phi = rem_two_pi(angle_between(ux, uy, wx, wy));
        m = r * phi;
        const double ww = wx * wx + wy * wy;
        // d(r phi) = phi u / r + r d(phi),  d(phi)/du = (uy, -ux) / |u|^2,  d(phi)/dw = (-wy, wx) / |w|^2
        const double dux = (phi * ux) / r + (uy / r2) * r, duy = (phi * uy) / r - (ux / r2) * r;
        const double dwx = (-wy / ww) * r, dwy = (wx / ww) * r;
        grad[0] = -(dux + dwx);
        grad[1] = -(duy + dwy);
        grad[2] = dux;
        grad[3] = duy;
        grad[4] = dwx;
        grad[5] = dwy;
        return 0;
    }
    default:
        return 0;
    }
}

#undef XV

}  // namespace measure
}  // namespace ezpz
