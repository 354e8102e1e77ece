// Residual-field rendering (include/ezpz_amd.h: ezpz_system_residual_field*, ezpz_residual_colormap, ezpz_residual_overlay):
// the counterpart of the reference's residual_viz module (ezpz/src/residual_viz.rs).  The field is evaluated on the device
// (residual_field.hip.hpp); the colour map is the same function on both sides; the overlay of the example and solution
// points is a few hundred pixels and is drawn on the host, with no device needed.
#include "residual_field.hip.hpp"
#include "system.hpp"

using namespace ezpz;

namespace {

// (the caller holds sys->mu, the system's device is current and its program is there)
int field_enqueue(EzpzSystem* sys, const double* x_base_dev, uint32_t var_x, uint32_t var_y, int64_t constraint, const EzpzViewport& vp,
                  double* mag_dev, uint8_t* rgb_dev, unsigned long long* deg_dev, hipStream_t stream) {
    const size_t n = std::max<size_t>(sys->counts.n_cons, 1);
    // header | records | their values | rank and table index by position | the count of a caller who asked for none
    const size_t o_recs = 64, o_vals = o_recs + n * sizeof(DevCon), o_rank = o_vals + n * 8 * sizeof(double), o_ci = o_rank + n * 4,
                 o_deg = (o_ci + n * 4 + 7) & ~size_t(7);
    if (int rc = sys->field_scratch.ensure(o_deg + 8)) return rc;
    unsigned char* s = sys->field_scratch.p;
    FieldArgs a{};
    a.p = sys->view;
    a.x_base = x_base_dev;
    a.var_x = var_x;
    a.var_y = var_y;
    a.sel = constraint;
    a.hdr = reinterpret_cast<FieldHeader*>(s);
    a.recs = reinterpret_cast<DevCon*>(s + o_recs);
    a.vals = reinterpret_cast<double*>(s + o_vals);
    a.rank = reinterpret_cast<uint32_t*>(s + o_rank);
    a.ci_of_pos = reinterpret_cast<uint32_t*>(s + o_ci);
    a.deg = deg_dev ? deg_dev : reinterpret_cast<unsigned long long*>(s + o_deg);
    a.vp = vp;
    a.mag = mag_dev;
    a.rgb = rgb_dev;
    a.wide = (vp.width % 4 == 0 && (reinterpret_cast<uintptr_t>(mag_dev) & 15u) == 0 && (reinterpret_cast<uintptr_t>(rgb_dev) & 3u) == 0) ? 1u : 0u;
    const uint64_t runs = (uint64_t)((vp.width + 3u) / 4u) * vp.height;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((runs + 255) / 256, (uint64_t)sys->lim.cus * 16);
    hipLaunchKernelGGL(field_prep_kernel, dim3(1), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    // which evaluator the list needs is known on the device only: a system of linear kinds alone has no use for the full one
    hipLaunchKernelGGL(field_kernel<true>, dim3(grid), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    if (!sys->linear_only) {
        hipLaunchKernelGGL(field_kernel<false>, dim3(grid), dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return EZPZ_OK;
}

int field_check(EzpzSystem* sys, const double* x_base, uint32_t var_x, uint32_t var_y, int64_t constraint, const EzpzViewport* vp,
                const void* mag, const void* rgb) {
    if (!sys || !vp || !x_base || (!mag && !rgb)) return EZPZ_ERR_INVALID_ARGUMENT;
    if (vp->width == 0 || vp->height == 0 || var_x == var_y) return EZPZ_ERR_INVALID_ARGUMENT;
    if ((uint64_t)((vp->width + 3ull) / 4) * vp->height > 0xFFFFFFFFull) return EZPZ_ERR_TOO_LARGE;
    if (int rc = ensure_program(sys)) return rc;
    if (var_x >= sys->counts.n_vars || var_y >= sys->counts.n_vars) return EZPZ_ERR_INVALID_ARGUMENT;
    if (constraint < -1 || constraint >= (int64_t)sys->counts.n_cons) return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

inline int32_t to_i32(double v) {  // Rust's `as i32`: saturating, NaN -> 0
    if (!(v == v)) return 0;
    if (v <= -2147483648.0) return INT32_MIN;
    if (v >= 2147483647.0) return INT32_MAX;
    return (int32_t)v;
}

struct Canvas {
    uint8_t* rgb;
    int32_t w, h;
    void put(int64_t px, int64_t py, const uint8_t (&c)[3]) const {
        if (px < 0 || px >= w || py < 0 || py >= h) return;
        uint8_t* d = rgb + ((size_t)py * (size_t)w + (size_t)px) * 3;
        d[0] = c[0];
        d[1] = c[1];
        d[2] = c[2];
    }
    // draw_filled_circle, residual_viz.rs:83-97
    void disc(int32_t cx, int32_t cy, int32_t radius, const uint8_t (&c)[3]) const {
        for (int32_t dy = -radius; dy <= radius; ++dy)
            for (int32_t dx = -radius; dx <= radius; ++dx)
                if (dx * dx + dy * dy <= radius * radius) put((int64_t)cx + dx, (int64_t)cy + dy, c);
    }
    // draw_line_segment, :99-120
    void segment(int64_t x0, int64_t y0, int64_t x1, int64_t y1, const uint8_t (&c)[3]) const {
        const int64_t dx = std::llabs(x1 - x0), dy = std::llabs(y1 - y0);
        const int64_t steps = std::max<int64_t>(std::max(dx, dy), 1);
        for (int64_t i = 0; i <= steps; ++i) {
            const double t = (double)i / (double)steps;
            put(to_i32(std::round((double)x0 + (double)(x1 - x0) * t)), to_i32(std::round((double)y0 + (double)(y1 - y0) * t)), c);
        }
    }
    // draw_arrow, :122-167
    void arrow(int32_t from_x, int32_t from_y, int32_t to_x, int32_t to_y, const uint8_t (&c)[3], int32_t head, double fraction) const {
        const int64_t dx = (int64_t)to_x - from_x, dy = (int64_t)to_y - from_y;
        const double len = std::hypot((double)dx, (double)dy);
        if (len < 1.0) return;
        const double ux = (double)dx / len, uy = (double)dy / len;
        const double actual = len * fraction;
        const int64_t tip_x = (int64_t)from_x + to_i32(std::round(ux * actual)), tip_y = (int64_t)from_y + to_i32(std::round(uy * actual));
        const int32_t steps = std::max(to_i32(actual), 2);
        for (int32_t i = 0; i <= steps; ++i) {
            const double t = (double)i / (double)steps;
            put((int64_t)from_x + to_i32(std::round(ux * actual * t)), (int64_t)from_y + to_i32(std::round(uy * actual * t)), c);
        }
        const int64_t back_x = tip_x - to_i32(std::round(ux * (double)head)), back_y = tip_y - to_i32(std::round(uy * (double)head));
        const int64_t perp_x = to_i32(std::round(-uy * ((double)head * 0.6))), perp_y = to_i32(std::round(ux * ((double)head * 0.6)));
        segment(tip_x, tip_y, back_x + perp_x, back_y + perp_y, c);
        segment(tip_x, tip_y, back_x - perp_x, back_y - perp_y, c);
        segment(back_x + perp_x, back_y + perp_y, back_x - perp_x, back_y - perp_y, c);
    }
};

}  // namespace

extern "C" {

int ezpz_system_residual_field_device(EzpzSystem* sys, const double* x_base_dev, uint32_t var_x, uint32_t var_y, int64_t constraint,
                                      const EzpzViewport* viewport, double* mag_dev, uint8_t* rgb_dev, uint64_t* degenerate_pixels_dev,
                                      void* stream) {
    if (int rc = field_check(sys, x_base_dev, var_x, var_y, constraint, viewport, mag_dev, rgb_dev)) return rc;
    release_thread_kernel(sys->device);
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    return field_enqueue(sys, x_base_dev, var_x, var_y, constraint, *viewport, mag_dev, rgb_dev,
                         reinterpret_cast<unsigned long long*>(degenerate_pixels_dev), static_cast<hipStream_t>(stream));
}

int ezpz_system_residual_field(EzpzSystem* sys, const double* x_base, uint32_t var_x, uint32_t var_y, int64_t constraint,
                               const EzpzViewport* viewport, double* mag_out, uint8_t* rgb_out, uint64_t* degenerate_pixels_out) {
    if (int rc = field_check(sys, x_base, var_x, var_y, constraint, viewport, mag_out, rgb_out)) return rc;
    release_thread_kernel(sys->device);
    std::lock_guard<std::mutex> lock(sys->mu);
    EZPZ_ON_DEVICE(sys->device);
    const size_t pixels = (size_t)viewport->width * viewport->height, n = sys->counts.n_vars;
    int rc;
    if ((rc = sys->field_x.ensure(n + 1)) != EZPZ_OK) return rc;  // (+ 1: the degenerate count behind the values)
    if (mag_out && (rc = sys->field_mag.ensure(pixels)) != EZPZ_OK) return rc;
    if (rgb_out && (rc = sys->field_rgb.ensure(pixels * 3)) != EZPZ_OK) return rc;
    HIP_TRY(hipMemcpy(sys->field_x.p, x_base, n * sizeof(double), hipMemcpyHostToDevice));
    unsigned long long* deg_dev = reinterpret_cast<unsigned long long*>(sys->field_x.p + n);
    rc = field_enqueue(sys, sys->field_x.p, var_x, var_y, constraint, *viewport, mag_out ? sys->field_mag.p : nullptr,
                       rgb_out ? sys->field_rgb.p : nullptr, deg_dev, nullptr);
    if (rc != EZPZ_OK) return rc;
    if (mag_out) HIP_TRY(hipMemcpy(mag_out, sys->field_mag.p, pixels * sizeof(double), hipMemcpyDeviceToHost));
    if (rgb_out) HIP_TRY(hipMemcpy(rgb_out, sys->field_rgb.p, pixels * 3, hipMemcpyDeviceToHost));
    unsigned long long deg = 0;
    HIP_TRY(hipMemcpy(&deg, deg_dev, sizeof(deg), hipMemcpyDeviceToHost));
    if (degenerate_pixels_out) *degenerate_pixels_out = deg;
    return EZPZ_OK;
}

void ezpz_residual_colormap(const double* mag, size_t n, uint8_t* rgb) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t r, g, b;
        residual_colour(mag[i], r, g, b);
        rgb[3 * i + 0] = (uint8_t)r;
        rgb[3 * i + 1] = (uint8_t)g;
        rgb[3 * i + 2] = (uint8_t)b;
    }
}

// draw_solver_overlay, residual_viz.rs:186-200 (world_to_pixel :65-69): later drawing wins
int ezpz_residual_overlay(uint8_t* rgb, const EzpzViewport* vp, double example_x, double example_y, double solution_x, double solution_y) {
    if (!rgb || !vp || vp->width == 0 || vp->height == 0 || vp->width > 0x7FFFFFFFu || vp->height > 0x7FFFFFFFu) return EZPZ_ERR_INVALID_ARGUMENT;
    const Canvas canvas{rgb, (int32_t)vp->width, (int32_t)vp->height};
    auto to_pixel = [&](double x, double y, int32_t& px, int32_t& py) {
        px = to_i32(std::round((x - vp->x_min) / (vp->x_max - vp->x_min) * (double)vp->width));
        py = to_i32(std::round((y - vp->y_min) / (vp->y_max - vp->y_min) * (double)vp->height));
    };
    int32_t ex, ey, sx, sy;
    to_pixel(example_x, example_y, ex, ey);
    to_pixel(solution_x, solution_y, sx, sy);
    const uint8_t dark_red[3] = {200, 0, 0}, red[3] = {255, 0, 0}, green[3] = {0, 180, 0};
    canvas.arrow(ex, ey, sx, sy, dark_red, 6, 0.5);
    canvas.disc(ex, ey, 5, red);
    canvas.disc(sx, sy, 5, green);
    return EZPZ_OK;
}

}  // extern "C"
