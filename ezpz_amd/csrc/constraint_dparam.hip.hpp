// d residual / d param for the 13 parametrised kinds (kinds.hpp: kind_has_param), beside the evaluators of
// constraint_eval.hip.hpp whose residuals it differentiates -- same guards, same operand order, built with -ffp-contract=off.
// __host__ __device__: the sensitivity kernels (sensitivity.hip.hpp) and ezpz_constraint_param_derivative (host only) share it.
//
//   nine kinds subtract the parameter (Distance, the two axis distances, Fixed, CircleRadius, ArcRadius -- two rows --, the three
//   point-line distances): -1 per row, 0 under the residual's guard;
//   ArcLength rotates the start by alpha = param / radius (constraint_eval.hip.hpp: EZPZ_ARC_LENGTH);
//   LinesAtAngle, ArcAngle, PointsAtAngle take their rotation from the parameter (rot_for), per degree where the tag says so.
// Unweighted, in the units of EzpzConstraint::param.  Returns the residual's degenerate flag (g0 = g1 = 0 then).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ezpz_amd.h"

namespace ezpz {
namespace dparam {

constexpr double EPS = 1e-4;  // lib.rs:43
constexpr double PI = 3.14159265358979323846264338327950288;

__host__ __device__ inline void sin_cos(double a, double& s, double& c) {
#ifdef __HIP_DEVICE_COMPILE__
    sincos(a, &s, &c);
#else
    s = std::sin(a);
    c = std::cos(a);
#endif
}

// d/dtheta of cross(u, R(-theta) v) / s  (lines_at_angle_residual)
__host__ __device__ inline bool lines_at_angle_dparam(double ux, double uy, double vx, double vy, double rad, double unit, double& g0) {
    const double len_u = hypot(ux, uy), len_v = hypot(vx, vy);
    if (len_u <= EPS || len_v <= EPS) return true;
    double s, c;
    sin_cos(rad, s, c);
    // R(-theta) v = (c vx + s vy, -s vx + c vy); its derivative by theta:
    const double dx = (c * vy) - (s * vx), dy = -(c * vx) - (s * vy);
    g0 = ((ux * dy - uy * dx) / ((len_u + len_v) * 0.5)) * unit;
    return false;
}

#define XV(i) (xs[ids[(i)]])

template <class XP>
__host__ __device__ inline bool con_dparam(uint32_t kind, uint32_t tag, const uint32_t* ids, double param, XP xs, double& g0, double& g1) {
    g0 = 0.0;
    g1 = 0.0;
    const double unit = (tag == EZPZ_ANGLE_OTHER_DEG) ? (PI / 180.0) : 1.0;
    switch (kind) {
    case EZPZ_DISTANCE:
    case EZPZ_VERTICAL_DISTANCE:
    case EZPZ_HORIZONTAL_DISTANCE:
    case EZPZ_FIXED:
    case EZPZ_CIRCLE_RADIUS:
        g0 = -1.0;
        return false;
    case EZPZ_ARC_RADIUS:
        g0 = -1.0;
        g1 = -1.0;
        return false;
    case EZPZ_POINT_LINE_DISTANCE: {
        const double a = XV(3) - XV(5), b = XV(4) - XV(2);
        if (hypot(a, b) < EPS) return true;
        g0 = -1.0;
        return false;
    }
    case EZPZ_VERTICAL_POINT_LINE_DISTANCE: {
        const double dx = XV(4) - XV(2), dy = XV(5) - XV(3);
        if (fabs(dx) <= EPS || (dx * dx + dy * dy) <= EPS * EPS) return true;
        g0 = -1.0;
        return false;
    }
    case EZPZ_HORIZONTAL_POINT_LINE_DISTANCE: {
        const double dx = XV(4) - XV(2), dy = XV(5) - XV(3);
        if (fabs(dy) <= EPS || (dx * dx + dy * dy) <= EPS * EPS) return true;
        g0 = -1.0;
        return false;
    }
    case EZPZ_ARC_LENGTH: {
        // r = (e - c) - R(alpha) u, alpha = param / |u|:  dr/dparam = -R'(alpha) u / |u|
        const double cx = XV(0), cy = XV(1);
        const double ux = XV(2) - cx, uy = XV(3) - cy;
        const double r2 = ux * ux + uy * uy;
        if (r2 <= EPS * EPS) return true;
        const double r = sqrt(r2);
        double sa, ca;
        sin_cos(param / r, sa, ca);
        g0 = (sa * ux + ca * uy) / r;
        g1 = -(ca * ux - sa * uy) / r;
        return false;
    }
    case EZPZ_LINES_AT_ANGLE:
        if (tag != EZPZ_ANGLE_OTHER_DEG && tag != EZPZ_ANGLE_OTHER_RAD) return false;
        return lines_at_angle_dparam(XV(2) - XV(0), XV(3) - XV(1), XV(6) - XV(4), XV(7) - XV(5), param * unit, unit, g0);
    case EZPZ_ARC_ANGLE: {
        if (tag != EZPZ_ANGLE_OTHER_DEG && tag != EZPZ_ANGLE_OTHER_RAD) return false;
        const double cx = XV(0), cy = XV(1);
        return lines_at_angle_dparam(XV(2) - cx, XV(3) - cy, XV(4) - cx, XV(5) - cy, param * unit, unit, g0);
    }
    case EZPZ_POINTS_AT_ANGLE: {
        // res = (v |u| - R(theta) u |v|) / s:  d res / d theta = -R'(theta) u |v| / s
        if (tag != EZPZ_ANGLE_OTHER_DEG && tag != EZPZ_ANGLE_OTHER_RAD) return false;
        const double px = XV(0), py = XV(1);
        const double ux = XV(2) - px, uy = XV(3) - py, vx = XV(4) - px, vy = XV(5) - py;
        const double len_u = hypot(ux, uy), len_v = hypot(vx, vy);
        if (len_u <= EPS || len_v <= EPS) return true;
        double s, c;
        sin_cos(param * unit, s, c);
        const double k = (len_v * (1.0 / ((len_u + len_v) * 0.5))) * unit;
        g0 = ((s * ux) + (c * uy)) * k;
        g1 = -((c * ux) - (s * uy)) * k;
        return false;
    }
    default:
        return false;
    }
}

#undef XV

}  // namespace dparam
}  // namespace ezpz
