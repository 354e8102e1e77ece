// ASan / UBSan driver for the host side of the sketch images (ezpz_amd/csrc/sketch_image.hip.hpp: skimg::check_request, skimg::image_host
// and skimg::compose_host, the whole of ezpz_sketch_image_host and ezpz_sketch_compose -- the entries forward to them -- and skimg::item_box,
// the culling both passes of the kernel rely on; ezpz_amd/csrc/png_write.hpp, the CLI's writer).  Host code only, run on the CPU: no
// device, no library --
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Iezpz_amd/csrc -Iinclude tools/asan_sketch_image.cpp -o /tmp/asan_sketch_image && /tmp/asan_sketch_image
// Every array is an allocation of exactly its size (so a read or write past its end is seen).  The cases of the CPU tests that have
// a known answer -- the ring of 376 pixels, the quarter arc of 94 either way round, the half-turn of 188, the ties -- then random
// lists of every kind on views whose sides are no multiple of anything, with values far outside the view, NaN, infinities and
// magnitudes above 2^30, half-widths from 0 to 1e300, masked variants.  Every answer is checked for what the interface promises
// whatever the numbers: increments is the sum of the counts, a pixel an item covers lies inside the box the kernel would walk for
// it, a skipped or masked item adds nothing.  The compositor runs on the counts with every corner of its arithmetic (full_at 0,
// a_min, opacity) and the picture is written as a PNG whose stream is decoded again here.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#define EZPZ_SKIMG_HOST_ONLY
#include "png_write.hpp"
#include "sketch_image.hip.hpp"

using namespace ezpz;
using namespace ezpz::skimg;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

template <class T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

static EzpzDrawItem item(uint16_t kind, uint8_t layer, uint8_t flags, std::initializer_list<uint32_t> ids, double h) {
    EzpzDrawItem it;
    std::memset(&it, 0, sizeof it);
    it.kind = kind, it.layer = layer, it.flags = flags, it.half_width = h;
    int k = 0;
    for (uint32_t id : ids) it.ids[k++] = id;
    return it;
}

static uint64_t draw_one(const std::vector<double>& values, const EzpzDrawItem& it, const EzpzImageView& vw, std::vector<uint32_t>* keep = nullptr) {
    auto x = exact<double>(values.size());
    std::memcpy(x.get(), values.data(), values.size() * sizeof(double));
    auto items = exact<EzpzDrawItem>(1);
    items[0] = it;
    const size_t cells = (size_t)vw.width * vw.height;
    auto counts = exact<uint32_t>(cells);
    auto info = exact<EzpzImageInfo>(1);
    CHECK(check_request(x.get(), 1, values.size(), items.get(), 1, &vw, 1, counts.get(), info.get()) == EZPZ_OK);
    image_host(x.get(), nullptr, 1, values.size(), items.get(), 1, vw, 1, false, counts.get(), info.get());
    uint64_t sum = 0;
    for (size_t i = 0; i < cells; ++i) sum += counts[i];
    CHECK(sum == info[0].increments && info[0].variants == 1);
    if (keep) keep->assign(counts.get(), counts.get() + cells);
    return sum;
}

// a stored-deflate zlib stream back into its bytes, with both checksums verified
static std::vector<uint8_t> inflate_stored(const uint8_t* z, size_t n) {
    CHECK(n >= 6 && z[0] == 0x78 && (z[0] * 256 + z[1]) % 31 == 0);
    std::vector<uint8_t> out;
    size_t at = 2;
    for (;;) {
        CHECK(at + 5 <= n && (z[at] & 6) == 0);
        const bool last = z[at] & 1;
        const uint32_t len = z[at + 1] | (z[at + 2] << 8), nlen = z[at + 3] | (z[at + 4] << 8);
        CHECK((len ^ nlen) == 0xFFFFu && at + 5 + len <= n);
        out.insert(out.end(), z + at + 5, z + at + 5 + len);
        at += 5 + len;
        if (last) break;
    }
    CHECK(at + 4 == n);
    const uint32_t adler = ((uint32_t)z[at] << 24) | (z[at + 1] << 16) | (z[at + 2] << 8) | z[at + 3];
    CHECK(adler == png::adler32(out.data(), out.size()));
    return out;
}

static void check_png(const uint8_t* rgb, uint32_t w, uint32_t h) {
    const std::vector<uint8_t> file = png::encode(rgb, w, h);
    auto data = exact<uint8_t>(file.size());  // (an exact allocation: the walk below must stay inside the file)
    std::memcpy(data.get(), file.data(), file.size());
    CHECK(file.size() > 8 + 25 + 12 + 12 && data[1] == 'P');
    size_t at = 8;
    std::vector<uint8_t> idat;
    int chunks = 0;
    while (at < file.size()) {
        CHECK(at + 12 <= file.size());
        const uint32_t len = ((uint32_t)data[at] << 24) | (data[at + 1] << 16) | (data[at + 2] << 8) | data[at + 3];
        CHECK(at + 12 + len <= file.size());
        const uint32_t crc = ((uint32_t)data[at + 8 + len] << 24) | (data[at + 9 + len] << 16) | (data[at + 10 + len] << 8) | data[at + 11 + len];
        CHECK(crc == png::crc32(data.get() + at + 4, len + 4));
        if (!std::memcmp(data.get() + at + 4, "IDAT", 4)) idat.assign(data.get() + at + 8, data.get() + at + 8 + len);
        if (!std::memcmp(data.get() + at + 4, "IHDR", 4)) CHECK(len == 13 && data[at + 11] == (w & 0xFF) && data[at + 15] == (h & 0xFF) && data[at + 16] == 8 && data[at + 17] == 2);
        at += 12 + len;
        ++chunks;
    }
    CHECK(chunks == 3 && at == file.size());
    const std::vector<uint8_t> raw = inflate_stored(idat.data(), idat.size());
    CHECK(raw.size() == (size_t)h * (3 * (size_t)w + 1));
    for (uint32_t y = 0; y < h; ++y) {
        CHECK(raw[(size_t)y * (3 * w + 1)] == 0);
        CHECK(!std::memcmp(&raw[(size_t)y * (3 * w + 1) + 1], rgb + (size_t)y * w * 3, 3 * (size_t)w));
    }
}

int main() {
    CHECK(png::crc32((const uint8_t*)"123456789", 9) == 0xCBF43926u && png::adler32((const uint8_t*)"Wikipedia", 9) == 0x11E60398u);
    // ---- known answers --------------------------------------------------------------------------------------------------------------
    const EzpzImageView unit{0.0, 0.0, 1.0, 200, 136};
    CHECK(draw_one({60.0, 60.0, 20.0}, item(EZPZ_DRAW_CIRCLE, 0, 0, {0, 1, 2}, 1.5), unit) == 376);
    CHECK(draw_one({60.0, 60.0, -20.0}, item(EZPZ_DRAW_CIRCLE, 0, 0, {0, 1, 2}, 1.5), unit) == 376);
    const std::vector<double> quarter{60.0, 60.0, 80.0, 60.0, 60.0, 80.0};
    CHECK(draw_one(quarter, item(EZPZ_DRAW_ARC, 0, 0, {0, 1, 2, 3, 4, 5}, 1.5), unit) == 94);
    CHECK(draw_one(quarter, item(EZPZ_DRAW_ARC, 0, 0, {0, 1, 4, 5, 2, 3}, 1.5), unit) == 94);
    CHECK(draw_one({60.0, 60.0, 80.0, 60.0, 40.0, 60.0}, item(EZPZ_DRAW_ARC, 0, 0, {0, 1, 2, 3, 4, 5}, 1.5), unit) == 188);
    CHECK(draw_one({60.0, 60.0, 80.0, 60.0, 80.0, 60.0}, item(EZPZ_DRAW_ARC, 0, 0, {0, 1, 2, 3, 4, 5}, 1.5), unit) == 0);  // a == b
    std::vector<uint32_t> c;
    draw_one({10.5, 10.5}, item(EZPZ_DRAW_POINT, 0, 0, {0, 1}, 3.0), unit, &c);  // the tie at exactly the radius
    CHECK(c[10 * 200 + 13] == 1 && c[10 * 200 + 14] == 0 && c[13 * 200 + 10] == 1 && c[7 * 200 + 10] == 1);
    draw_one({5.0, 20.0, 30.0, 20.0}, item(EZPZ_DRAW_SEGMENT, 0, 0, {0, 1, 2, 3}, 1.5), unit, &c);
    CHECK(c[18 * 200 + 10] == 1 && c[17 * 200 + 10] == 0 && c[21 * 200 + 10] == 1 && c[22 * 200 + 10] == 0);
    CHECK(draw_one({20.5, 30.5}, item(EZPZ_DRAW_POINT, 0, 0, {0, 1}, 0.0), unit) == 1);
    CHECK(draw_one({20.0, 30.5}, item(EZPZ_DRAW_POINT, 0, 0, {0, 1}, 0.0), unit) == 0);
    CHECK(draw_one({20.0, 30.5}, item(EZPZ_DRAW_POINT, 0, 0, {0, 1}, 1e300), unit) == 200 * 136);

    // ---- argument errors ------------------------------------------------------------------------------------------------------------
    {
        double x[3] = {1.0, 2.0, 3.0};
        uint32_t counts[4];
        EzpzImageInfo info;
        EzpzImageView vw{0.0, 0.0, 1.0, 2, 2};
        EzpzDrawItem good = item(EZPZ_DRAW_CIRCLE, 0, EZPZ_DRAW_FILL, {0, 1, 2}, 1.0);
        CHECK(check_request(x, 1, 3, &good, 1, &vw, 1, counts, &info) == EZPZ_OK);
        EzpzDrawItem bad = good;
        bad.ids[2] = 3;
        CHECK(check_request(x, 1, 3, &bad, 1, &vw, 1, counts, &info) == EZPZ_ERR_INVALID_ARGUMENT);
        bad = good, bad.kind = 4;
        CHECK(check_request(x, 1, 3, &bad, 1, &vw, 1, counts, &info) == EZPZ_ERR_INVALID_ARGUMENT);
        bad = good, bad.layer = 1;
        CHECK(check_request(x, 1, 3, &bad, 1, &vw, 1, counts, &info) == EZPZ_ERR_INVALID_ARGUMENT);
        bad = good, bad.kind = EZPZ_DRAW_POINT;
        CHECK(check_request(x, 1, 3, &bad, 1, &vw, 1, counts, &info) == EZPZ_ERR_INVALID_ARGUMENT);
        bad = good, bad.half_width = std::numeric_limits<double>::quiet_NaN();
        CHECK(check_request(x, 1, 3, &bad, 1, &vw, 1, counts, &info) == EZPZ_ERR_INVALID_ARGUMENT);
        bad = good, bad.half_width = -1.0;
        CHECK(check_request(x, 1, 3, &bad, 1, &vw, 1, counts, &info) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(check_request(x, 1, 3, &good, 1, &vw, 0, counts, &info) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(check_request(x, 1, 3, &good, 1, &vw, 9, counts, &info) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(check_request(nullptr, 1, 3, &good, 1, &vw, 1, counts, &info) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(check_request(x, (size_t)1 << 32, 3, &good, 1, &vw, 1, counts, &info) == EZPZ_ERR_TOO_LARGE);
        CHECK(check_request(x, ((size_t)1 << 32) - 1, 3, &good, 1, &vw, 1, counts, &info) == EZPZ_OK);
        for (double scale : {0.0, -1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
            EzpzImageView v2 = vw;
            v2.scale = scale;
            CHECK(check_view(&v2, 1) == EZPZ_ERR_INVALID_ARGUMENT);
        }
        EzpzImageView v2 = vw;
        v2.width = 16385;
        CHECK(check_view(&v2, 1) == EZPZ_ERR_INVALID_ARGUMENT && check_view(nullptr, 1) == EZPZ_ERR_INVALID_ARGUMENT);
    }

    // ---- random lists ---------------------------------------------------------------------------------------------------------------
    std::mt19937_64 rng(20251);
    std::uniform_real_distribution<double> unit01(0.0, 1.0);
    const double odd[] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                          3e9, -3e9, 1073741824.0, 1e300, -1e-300, 0.0};
    const double widths[] = {0.0, 0.5, 1.5, 3.0, 40.0, 1e9, 1e300};
    for (int trial = 0; trial < 60; ++trial) {
        EzpzImageView vw;
        vw.width = 1 + (uint32_t)(rng() % 97), vw.height = 1 + (uint32_t)(rng() % 71);
        vw.scale = trial % 3 == 0 ? 1.0 : 0.25 + 9.0 * unit01(rng);
        vw.x_min = -5.0 + 10.0 * unit01(rng), vw.y_min = -5.0 + 10.0 * unit01(rng);
        const uint32_t n_layers = 1 + (uint32_t)(rng() % 8);
        const size_t n_vars = 6 + rng() % 10, n_items = rng() % 9, batch = rng() % 6;
        auto x = exact<double>(batch * n_vars);
        auto ok = exact<uint8_t>(batch);
        for (size_t i = 0; i < batch * n_vars; ++i) {
            const double span = (double)(vw.width > vw.height ? vw.width : vw.height) / vw.scale;
            x[i] = rng() % 13 == 0 ? odd[rng() % 9] : rng() % 5 == 0 ? (unit01(rng) - 0.5) * 40.0 * span : vw.x_min + (unit01(rng) * 1.4 - 0.2) * span;
        }
        for (size_t b = 0; b < batch; ++b) ok[b] = rng() % 4 ? 1 : 0;
        auto items = exact<EzpzDrawItem>(n_items);
        for (size_t i = 0; i < n_items; ++i) {
            const uint16_t kind = (uint16_t)(rng() % 4);
            items[i] = item(kind, (uint8_t)(rng() % n_layers), kind == EZPZ_DRAW_CIRCLE && rng() % 2 ? EZPZ_DRAW_FILL : 0, {}, widths[rng() % 7]);
            for (uint32_t k = 0; k < ids_used(kind); ++k) items[i].ids[k] = (uint32_t)(rng() % n_vars);
        }
        const size_t plane = (size_t)vw.width * vw.height, cells = plane * n_layers;
        auto counts = exact<uint32_t>(cells);
        auto info = exact<EzpzImageInfo>(1);
        const uint8_t* mask = trial % 2 ? ok.get() : nullptr;
        CHECK(check_request(x.get(), batch, n_vars, items.get(), n_items, &vw, n_layers, counts.get(), info.get()) == EZPZ_OK);
        image_host(x.get(), mask, batch, n_vars, items.get(), n_items, vw, n_layers, false, counts.get(), info.get());
        uint64_t sum = 0, masked = 0;
        for (size_t i = 0; i < cells; ++i) sum += counts[i];
        for (size_t b = 0; b < batch; ++b) masked += mask && !mask[b];
        CHECK(sum == info[0].increments && info[0].variants == batch && info[0].masked == masked);
        CHECK(info[0].items_skipped <= (batch - masked) * n_items);
        // accumulating once more doubles everything
        image_host(x.get(), mask, batch, n_vars, items.get(), n_items, vw, n_layers, true, counts.get(), info.get());
        CHECK(info[0].increments == 2 * sum && info[0].variants == 2 * batch);
        // every covered pixel lies inside the box the kernel would walk
        uint64_t covered = 0;
        for (size_t b = 0; b < batch; ++b) {
            if (mask && !mask[b]) continue;
            for (size_t i = 0; i < n_items; ++i) {
                double p[kParams];
                if (!item_params(items[i], x.get() + b * n_vars, vw, p)) continue;
                const Box box = item_box(items[i].kind, items[i].flags, p, items[i].half_width, vw.width, vw.height);
                CHECK(box.x0 > box.x1 || (box.x0 >= 0 && box.y0 >= 0 && box.x1 < (int)vw.width && box.y1 < (int)vw.height && box.y0 <= box.y1));
                for (uint32_t py = 0; py < vw.height; ++py)
                    for (uint32_t px = 0; px < vw.width; ++px)
                        if (covers(items[i].kind, items[i].flags, p, items[i].half_width, px + 0.5, py + 0.5)) {
                            CHECK(box.x0 <= (int)px && (int)px <= box.x1 && box.y0 <= (int)py && (int)py <= box.y1);
                            ++covered;
                        }
            }
        }
        CHECK(covered == sum);
        // the compositor and the writer on these counts
        auto layers = exact<EzpzComposeLayer>(n_layers);
        for (uint32_t l = 0; l < n_layers; ++l) {
            layers[l] = EzpzComposeLayer{{(uint8_t)rng(), (uint8_t)rng(), (uint8_t)rng()}, (uint8_t)(l % 3 == 0 ? 255 : rng()), (uint8_t)(l % 2 ? rng() : 0),
                                         (uint32_t)(l % 4 == 0 ? 0 : rng() % 5)};
        }
        const uint8_t background[3] = {(uint8_t)rng(), 255, 0};
        auto rgb = exact<uint8_t>(plane * 3);
        compose_host(counts.get(), vw, n_layers, layers.get(), background, rgb.get());
        for (size_t i = 0; i < plane; ++i) {
            bool any = false;
            for (uint32_t l = 0; l < n_layers; ++l) any = any || counts[l * plane + i];
            if (!any) CHECK(!std::memcmp(&rgb[3 * i], background, 3));
        }
        check_png(rgb.get(), vw.width, vw.height);
    }
    // a picture whose rows do not fit one stored block
    {
        const uint32_t w = 301, h = 257;
        auto rgb = exact<uint8_t>((size_t)w * h * 3);
        for (size_t i = 0; i < (size_t)w * h * 3; ++i) rgb[i] = (uint8_t)(i * 2654435761u >> 13);
        check_png(rgb.get(), w, h);
    }
    std::printf("asan_sketch_image: ok\n");
    return 0;
}
