// Sketch images (include/ezpz_amd.h: ezpz_sketch_image and its siblings): the rule, once, for the host and the
// device -- the pixel-space numbers of an item of a variant, "does it cover the pixel centre (X, Y)", a box that holds every pixel it
// can cover -- the host forms that need no device (the plain loops of ezpz_sketch_image_host, the compositor) and, for hipcc, the
// two kernels.  Only + - * /, fabs and comparisons decide a pixel, each rounded once in the order written: no unit is built with
// contraction, so the three sides agree bit for bit and the counts, integers, do not depend on the schedule.
// A host-only user (tools/asan_sketch_image.cpp, under EZPZ_SKIMG_HOST_ONLY) takes the rule and the host forms alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/ezpz_amd.h"

#if defined(__HIPCC__) && !defined(EZPZ_SKIMG_HOST_ONLY)
#include <hip/hip_runtime.h>
#define EZPZ_SKIMG_HD __host__ __device__ inline
#else
#define EZPZ_SKIMG_HD inline
#endif

namespace ezpz {
namespace skimg {

static_assert(sizeof(EzpzImageView) == 32 && sizeof(EzpzDrawItem) == 40 && sizeof(EzpzImageInfo) == 32 && sizeof(EzpzComposeLayer) == 12,
              "the layouts include/ezpz_amd.h documents");

constexpr double kMaxCoord = 1073741824.0;  // 2^30: the skip rule's bound
constexpr uint32_t kParams = 6;             // pixel-space numbers per (item, variant), at most

EZPZ_SKIMG_HD double absd(double v) { return v < 0.0 ? -v : v; }  // (fabs: the sign alone, exact on either side)
// finite and at most 2^30 in magnitude (false for a NaN)
EZPZ_SKIMG_HD bool usable(double v) { return absd(v) <= kMaxCoord; }

// ---- argument checks, shared by every entry ---------------------------------------------------------------------------------------
inline bool finite_host(double v) { return absd(v) <= 1.7976931348623157e308; }

inline uint32_t ids_used(uint32_t kind) { return kind == EZPZ_DRAW_POINT ? 2u : kind == EZPZ_DRAW_SEGMENT ? 4u : kind == EZPZ_DRAW_CIRCLE ? 3u : 6u; }

inline int check_view(const EzpzImageView* view, uint32_t n_layers) {
    if (!view || n_layers < 1 || n_layers > EZPZ_IMAGE_MAX_LAYERS) return EZPZ_ERR_INVALID_ARGUMENT;
    if (view->width < 1 || view->width > EZPZ_IMAGE_MAX_SIDE || view->height < 1 || view->height > EZPZ_IMAGE_MAX_SIDE) return EZPZ_ERR_INVALID_ARGUMENT;
    if (!finite_host(view->scale) || !(view->scale > 0.0) || !finite_host(view->x_min) || !finite_host(view->y_min)) return EZPZ_ERR_INVALID_ARGUMENT;
    return EZPZ_OK;
}

// Every argument error of a drawing request; the pointers x, counts and info are only compared with NULL.
inline int check_request(const void* x, size_t batch, size_t n_vars, const EzpzDrawItem* items, size_t n_items, const EzpzImageView* view,
                         uint32_t n_layers, const void* counts, const void* info) {
    if (int rc = check_view(view, n_layers)) return rc;
    if (!counts || !info || (n_items && !items) || (batch && n_items && !x)) return EZPZ_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n_items; ++i) {
        const EzpzDrawItem& it = items[i];
        if (it.kind > EZPZ_DRAW_ARC || it.layer >= n_layers) return EZPZ_ERR_INVALID_ARGUMENT;
        if (it.flags & ~EZPZ_DRAW_FILL || (it.flags && it.kind != EZPZ_DRAW_CIRCLE)) return EZPZ_ERR_INVALID_ARGUMENT;
        for (uint32_t k = 0; k < ids_used(it.kind); ++k)
            if (it.ids[k] >= n_vars) return EZPZ_ERR_INVALID_ARGUMENT;
        if (!finite_host(it.half_width) || !(it.half_width >= 0.0)) return EZPZ_ERR_INVALID_ARGUMENT;
    }
    if (n_items && batch >= (1ull << 32) / n_items + ((1ull << 32) % n_items ? 1 : 0)) return EZPZ_ERR_TOO_LARGE;
    return EZPZ_OK;
}

// ---- the rule ------------------------------------------------------------------------------------------------------------------------
// The pixel-space numbers p[0 .. 5] of item `it` for the variant whose values are x [n_vars]; false: the item is skipped.
//   POINT u v | SEGMENT au av bu bv | CIRCLE u v R | ARC cu cv au av bu bv
EZPZ_SKIMG_HD bool item_params(const EzpzDrawItem& it, const double* x, const EzpzImageView& vw, double* p) {
    const uint32_t kind = it.kind;
    const uint32_t pairs = kind == EZPZ_DRAW_POINT ? 1u : kind == EZPZ_DRAW_SEGMENT ? 2u : kind == EZPZ_DRAW_CIRCLE ? 1u : 3u;
    bool good = true;
    for (uint32_t k = 0; k < kParams; ++k) p[k] = 0.0;
    for (uint32_t k = 0; k < pairs; ++k) {
        p[2 * k] = (x[it.ids[2 * k]] - vw.x_min) * vw.scale;
        p[2 * k + 1] = (x[it.ids[2 * k + 1]] - vw.y_min) * vw.scale;
        good = good && usable(p[2 * k]) && usable(p[2 * k + 1]);
    }
    if (kind == EZPZ_DRAW_CIRCLE) {
        p[2] = absd(x[it.ids[2]]) * vw.scale;
        good = good && usable(p[2]);
    }
    return good;
}

// the ring | |w| - R | <= h without a root
EZPZ_SKIMG_HD bool in_ring(double d2, double R2, double h) {
    const double q = (d2 + R2) - h * h;
    return q <= 0.0 || q * q <= (4.0 * d2) * R2;
}

// Does the item with the numbers p cover the pixel centre (X, Y)?
EZPZ_SKIMG_HD bool covers(uint32_t kind, uint32_t flags, const double* p, double h, double X, double Y) {
    if (kind == EZPZ_DRAW_POINT) {
        const double dx = X - p[0], dy = Y - p[1];
        const double d2 = dx * dx + dy * dy;
        return d2 <= h * h;
    }
    if (kind == EZPZ_DRAW_SEGMENT) {
        const double ex = p[2] - p[0], ey = p[3] - p[1];
        const double L2 = ex * ex + ey * ey;
        const double wx = X - p[0], wy = Y - p[1];
        const double t = wx * ex + wy * ey;
        if (L2 == 0.0 || t <= 0.0) return wx * wx + wy * wy <= h * h;
        if (t >= L2) {
            const double zx = X - p[2], zy = Y - p[3];
            return zx * zx + zy * zy <= h * h;
        }
        const double cr = wx * ey - wy * ex;
        return cr * cr <= (h * h) * L2;
    }
    if (kind == EZPZ_DRAW_CIRCLE) {
        const double wx = X - p[0], wy = Y - p[1];
        const double d2 = wx * wx + wy * wy;
        const double R = p[2];
        const double R2 = R * R;
        if (flags & EZPZ_DRAW_FILL) {
            const double hi = R + h;
            return d2 <= hi * hi;
        }
        return in_ring(d2, R2, h);
    }
    // ARC: centre p[0 .. 1], a p[2 .. 3], b p[4 .. 5]
    const double px = p[2] - p[0], py = p[3] - p[1], qx = p[4] - p[0], qy = p[5] - p[1];
    const double R2 = px * px + py * py;
    const double wx = X - p[0], wy = Y - p[1];
    const double d2 = wx * wx + wy * wy;
    if (!in_ring(d2, R2, h)) return false;
    const double s = px * qy - py * qx;
    const double c1 = px * wy - py * wx;
    const double c2 = wx * qy - wy * qx;
    if (s > 0.0) return c1 >= 0.0 && c2 >= 0.0;
    if (s < 0.0) return c1 <= 0.0 && c2 <= 0.0;
    if (px * qx + py * qy > 0.0) return false;
    return c1 >= 0.0;
}

// A box of pixels [x0, x1] x [y0, y1], clipped to the view, outside which the item covers nothing: the extent of its points grown by
// its reach -- h, and a circle's or an arc's radius -- and by a pixel on every side for the rounding of the tests above.  Empty: x0 > x1.
// (Culling only: whatever the box, the pixels inside it are decided by covers().  The root and the box's own rounding are taken up by
// the pixel of growth: every number is at most 2^30 + h, and a reach above 2^31 covers the whole view.)
struct Box {
    int x0, y0, x1, y1;
};

EZPZ_SKIMG_HD Box item_box(uint32_t kind, uint32_t flags, const double* p, double h, uint32_t width, uint32_t height) {
    (void)flags;
    double lo_x = p[0], hi_x = p[0], lo_y = p[1], hi_y = p[1], reach = h;
    if (kind == EZPZ_DRAW_SEGMENT) {
        lo_x = p[2] < lo_x ? p[2] : lo_x, hi_x = p[2] > hi_x ? p[2] : hi_x;
        lo_y = p[3] < lo_y ? p[3] : lo_y, hi_y = p[3] > hi_y ? p[3] : hi_y;
    } else if (kind == EZPZ_DRAW_CIRCLE) {
        reach = p[2] + h;
    } else if (kind == EZPZ_DRAW_ARC) {
        const double px = p[2] - p[0], py = p[3] - p[1];
        reach = __builtin_sqrt(px * px + py * py) * 1.0000001 + h;  // (the root serves the box alone)
    }
    // (reach can be huge, h being any finite number: clamp in doubles before the conversion)
    const double W = (double)width, H = (double)height;
    double a = lo_x - reach - 1.5, b = hi_x + reach + 1.5, c = lo_y - reach - 1.5, d = hi_y + reach + 1.5;
    Box box;
    if (!(a < W) || !(b >= 0.0) || !(c < H) || !(d >= 0.0)) {
        box.x0 = 1, box.y0 = 1, box.x1 = 0, box.y1 = 0;
        return box;
    }
    a = a < 0.0 ? 0.0 : a, c = c < 0.0 ? 0.0 : c;
    b = b > W - 1.0 ? W - 1.0 : b, d = d > H - 1.0 ? H - 1.0 : d;
    box.x0 = (int)a, box.y0 = (int)c, box.x1 = (int)b, box.y1 = (int)d;  // (truncation: downwards for these non-negative numbers)
    return box;
}

// ---- the host forms that need no device --------------------------------------------------------------------------------------------
// The rule alone: every pixel of the view for every item of every variant.  The request is checked.
inline void image_host(const double* x, const uint8_t* ok, size_t batch, size_t n_vars, const EzpzDrawItem* items, size_t n_items,
                       const EzpzImageView& vw, uint32_t n_layers, bool accumulate, uint32_t* counts, EzpzImageInfo* info) {
    const size_t plane = (size_t)vw.width * vw.height;
    if (!accumulate) {
        std::memset(counts, 0, plane * n_layers * sizeof(uint32_t));
        std::memset(info, 0, sizeof *info);
    }
    info->variants += batch;
    for (size_t b = 0; b < batch; ++b) {
        if (ok && !ok[b]) {
            info->masked += 1;
            continue;
        }
        for (size_t i = 0; i < n_items; ++i) {
            const EzpzDrawItem& it = items[i];
            double p[kParams];
            if (!item_params(it, x + b * n_vars, vw, p)) {
                info->items_skipped += 1;
                continue;
            }
            uint32_t* layer = counts + plane * it.layer;
            for (uint32_t py = 0; py < vw.height; ++py)
                for (uint32_t px = 0; px < vw.width; ++px)
                    if (covers(it.kind, it.flags, p, it.half_width, (double)px + 0.5, (double)py + 0.5)) {
                        layer[(size_t)py * vw.width + px] += 1;
                        info->increments += 1;
                    }
        }
    }
}

// The compositor: integers only.  The request is checked.
inline void compose_host(const uint32_t* counts, const EzpzImageView& vw, uint32_t n_layers, const EzpzComposeLayer* layers,
                         const uint8_t background[3], uint8_t* rgb_out) {
    const size_t plane = (size_t)vw.width * vw.height;
    for (size_t i = 0; i < plane; ++i)
        for (int c = 0; c < 3; ++c) rgb_out[3 * i + c] = background[c];
    for (uint32_t l = 0; l < n_layers; ++l) {
        const EzpzComposeLayer& L = layers[l];
        const uint32_t* cnt = counts + plane * l;
        uint64_t F = L.full_at;
        if (F == 0)
            for (size_t i = 0; i < plane; ++i) F = cnt[i] > F ? cnt[i] : F;
        if (F == 0) F = 1;
        for (size_t i = 0; i < plane; ++i) {
            if (cnt[i] == 0) continue;
            uint64_t a = (cnt[i] < F ? (uint64_t)cnt[i] : F) * 255u / F;
            if (a < L.a_min) a = L.a_min;
            a = a * L.opacity / 255u;
            for (int c = 0; c < 3; ++c) rgb_out[3 * i + c] = (uint8_t)((rgb_out[3 * i + c] * (255u - a) + L.rgb[c] * a + 127u) / 255u);
        }
    }
}

#if defined(__HIPCC__) && defined(EZPZ_SKIMG_KERNELS)

// ---- the kernels (sketch_image.hip alone defines EZPZ_SKIMG_KERNELS) -------------------------------------------------------------------------------------------------------------------
// Pass 1 packs, pass 2 rasterises.  A round is `count` variants (the host side cuts a call into rounds so that the packed numbers stay
// bounded); everything a round shares is in RoundArgs.
constexpr uint32_t kTile = 64;  // a tile is kTile x kTile pixels: a row is a wavefront wide, its counts 16 KiB of LDS

struct ItemBox {  // the union over a round's variants, by unsigned minima from 0xFFFFFFFF: x0, y0, 0xFFFF - x1, 0xFFFF - y1
    uint32_t m[4];
};

struct RoundArgs {
    const double* x;        // [count][n_vars]
    const uint8_t* ok;      // [count] or NULL
    const EzpzDrawItem* items;  // device copy
    uint32_t count, n_vars, n_items;
    EzpzImageView view;
    double* packed;         // [n_items][count][kParams]
    uint16_t* boxes;        // [n_items][count][4]: x0, y0, x1, y1; x0 > x1: nothing to draw
    ItemBox* item_box;      // [n_items]
    uint32_t* counts;
    EzpzImageInfo* info;
    uint32_t per_slice;     // pass 2: variants per workgroup
    uint32_t count_info;    // pass 1: this launch counts the round's variants and masked ones (the first of a round's launches)
};

// Pass 1: thread = (variant, item).  The gather from the variant's row happens here once; pass 2 streams.  blockIdx.y == 0 also counts
// the round's variants and the masked ones (the grid has one row of blocks at least, whatever n_items is).
__global__ __launch_bounds__(256) void pack_kernel(RoundArgs a) {
    __shared__ uint32_t s_box[4];
    __shared__ uint32_t s_masked, s_skipped;
    const uint32_t item = blockIdx.y, v = blockIdx.x * 256u + threadIdx.x;
    if (threadIdx.x < 4) s_box[threadIdx.x] = 0xFFFFFFFFu;
    if (threadIdx.x == 0) s_masked = 0, s_skipped = 0;
    __syncthreads();
    if (v < a.count) {
        const bool masked = a.ok && !a.ok[v];
        if (masked && item == 0 && a.count_info) atomicAdd(&s_masked, 1u);
        if (item < a.n_items) {
            const EzpzDrawItem it = a.items[item];
            double p[kParams] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            Box box{1, 1, 0, 0};
            if (!masked) {
                if (item_params(it, a.x + (size_t)v * a.n_vars, a.view, p))
                    box = item_box(it.kind, it.flags, p, it.half_width, a.view.width, a.view.height);
                else
                    atomicAdd(&s_skipped, 1u);
            }
            const size_t at = (size_t)item * a.count + v;
            double* out = a.packed + at * kParams;
#pragma unroll
            for (uint32_t k = 0; k < kParams; ++k) out[k] = p[k];
            ushort4 packed_box;
            packed_box.x = (uint16_t)box.x0, packed_box.y = (uint16_t)box.y0, packed_box.z = (uint16_t)box.x1, packed_box.w = (uint16_t)box.y1;
            reinterpret_cast<ushort4*>(a.boxes)[at] = packed_box;
            if (box.x0 <= box.x1) {
                atomicMin(&s_box[0], (uint32_t)box.x0), atomicMin(&s_box[1], (uint32_t)box.y0);
                atomicMin(&s_box[2], 0xFFFFu - (uint32_t)box.x1), atomicMin(&s_box[3], 0xFFFFu - (uint32_t)box.y1);
            }
        }
    }
    __syncthreads();
    if (item < a.n_items && threadIdx.x < 4 && s_box[0] != 0xFFFFFFFFu) atomicMin(&a.item_box[item].m[threadIdx.x], s_box[threadIdx.x]);
    if (threadIdx.x == 0) {
        if (item == 0 && blockIdx.x == 0 && a.count_info) atomicAdd((unsigned long long*)&a.info->variants, (unsigned long long)a.count);
        if (s_masked) atomicAdd((unsigned long long*)&a.info->masked, (unsigned long long)s_masked);
        if (s_skipped) atomicAdd((unsigned long long*)&a.info->items_skipped, (unsigned long long)s_skipped);
    }
}

// Pass 2: workgroup = (tile, item, slice of the round's variants).  One whose tile misses the item's box leaves at once.  Otherwise
// the tile's counts live in LDS; a wavefront takes a variant at a time -- its box against the tile is wave-uniform -- and walks the
// clipped box with the lanes across a row's pixels (several rows at once where the box is narrow), adding with LDS atomics; at the end
// the cells that are not zero go out by global integer adds.  No workgroup waits for another.
__global__ __launch_bounds__(256) void raster_kernel(RoundArgs a) {
    __shared__ uint32_t s_tile[kTile * kTile];
    __shared__ unsigned long long s_sum;
    const uint32_t tiles_x = (a.view.width + kTile - 1) / kTile;
    const int tx0 = (int)((blockIdx.x % tiles_x) * kTile), ty0 = (int)((blockIdx.x / tiles_x) * kTile);
    const uint32_t item = blockIdx.y;
    const ItemBox ib = a.item_box[item];
    if (ib.m[0] == 0xFFFFFFFFu) return;
    if ((int)ib.m[0] > tx0 + (int)kTile - 1 || (int)(0xFFFFu - ib.m[2]) < tx0 || (int)ib.m[1] > ty0 + (int)kTile - 1 || (int)(0xFFFFu - ib.m[3]) < ty0) return;
    const uint32_t first = blockIdx.z * a.per_slice;
    if (first >= a.count) return;
    const uint32_t last = first + a.per_slice < a.count ? first + a.per_slice : a.count;
    for (uint32_t i = threadIdx.x; i < kTile * kTile; i += 256) s_tile[i] = 0;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const EzpzDrawItem it = a.items[item];
    const uint32_t kind = it.kind, flags = it.flags;
    const double h = it.half_width;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const ushort4* boxes = reinterpret_cast<const ushort4*>(a.boxes) + (size_t)item * a.count;
    const double* packed = a.packed + (size_t)item * a.count * kParams;
    for (uint32_t v = first + wave; v < last; v += 4) {
        const ushort4 b = boxes[v];
        int x0 = b.x, y0 = b.y, x1 = b.z, y1 = b.w;
        if (x0 > x1) continue;
        x0 = x0 < tx0 ? tx0 : x0, y0 = y0 < ty0 ? ty0 : y0;
        x1 = x1 > tx0 + (int)kTile - 1 ? tx0 + (int)kTile - 1 : x1, y1 = y1 > ty0 + (int)kTile - 1 ? ty0 + (int)kTile - 1 : y1;
        if (x0 > x1 || y0 > y1) continue;
        double p[kParams];
#pragma unroll
        for (uint32_t k = 0; k < kParams; ++k) p[k] = packed[(size_t)v * kParams + k];
        // lanes: `cols` (a power of two >= the box's width) across, 64 / cols rows at once
        const uint32_t bw = (uint32_t)(x1 - x0 + 1);
        uint32_t shift = 0;
        while ((1u << shift) < bw) ++shift;
        const uint32_t col = lane & ((1u << shift) - 1u), row_of_lane = lane >> shift, rows_at_once = 64u >> shift;
        const int px = x0 + (int)col;
        const double X = (double)px + 0.5;
        for (int py = y0 + (int)row_of_lane; py <= y1; py += (int)rows_at_once) {
            if (col < bw && covers(kind, flags, p, h, X, (double)py + 0.5))
                atomicAdd(&s_tile[(uint32_t)(py - ty0) * kTile + (uint32_t)(px - tx0)], 1u);
        }
    }
    __syncthreads();
    uint32_t* layer = a.counts + (size_t)it.layer * a.view.width * a.view.height;
    unsigned long long mine = 0;
    for (uint32_t i = threadIdx.x; i < kTile * kTile; i += 256) {
        const uint32_t c = s_tile[i];
        const uint32_t gx = (uint32_t)tx0 + (i & (kTile - 1)), gy = (uint32_t)ty0 + i / kTile;
        if (c && gx < a.view.width && gy < a.view.height) {
            atomicAdd(&layer[(size_t)gy * a.view.width + gx], c);
            mine += c;
        }
    }
    if (mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd((unsigned long long*)&a.info->increments, s_sum);
}

#endif  // __HIPCC__ && EZPZ_SKIMG_KERNELS

}  // namespace skimg
}  // namespace ezpz
