// Sketch images (include/ezpz_amd.h: ezpz_sketch_image, its _device and _host forms, ezpz_sketch_compose): the host
// side of sketch_image.hip.hpp -- the check of a request, the workspace the process keeps per device (the packed numbers and boxes
// of a round, the device copy of the item list) and the rounds.  A call is cut into rounds of variants so that the packed numbers
// stay below kRoundBytes; a round is the reset of the items' boxes, pass 1 and pass 2, all on the caller's stream.  The run with an
// image, ezpz_system_tolerance_mc_image in tolerance_mc.hip, enqueues the device form behind each of its rounds.
#define EZPZ_SKIMG_KERNELS
#include "sketch_image.hip.hpp"

#include "host_stage.hpp"
#include "mc_block_sum.hip.hpp"
#include "one_call.hpp"

using namespace ezpz;
using namespace ezpz::skimg;

namespace {

constexpr uint64_t kRoundBytes = 128ull << 20;  // of packed numbers and boxes per round
constexpr uint32_t kRoundMax = 1u << 20;        // variants per round at most
constexpr uint32_t kItemsPerLaunch = 32768;     // a launch's grid has an item per block row
constexpr uint32_t kSliceVariants = 1024;       // pass 2: variants per workgroup (256 a wavefront)
constexpr uint32_t kMaxSlices = 1024;
constexpr size_t kHostRound = 65536;            // the host form: variants staged at once

// the process's workspace, one per device (system.hpp: plan_of_device)
struct ImageWork {
    DevBuf<double> packed;
    DevBuf<uint16_t> boxes;
    DevBuf<ItemBox> item_box;
    DevBuf<EzpzDrawItem> items;
    std::vector<unsigned char> items_kept;  // what `items` holds
    std::mutex host_mu;                     // a host form holds it from its upload to its copies back
    DevBuf<unsigned char> host_stage;       // the host form's x, ok, counts and info (host_stage.hpp)
};
using ImagePlan = mcb::ProcessPlan<ImageWork>;

uint32_t round_of(size_t batch, size_t n_items) {
    const uint64_t per_variant = std::max<uint64_t>(n_items, 1) * (kParams * sizeof(double) + 4 * sizeof(uint16_t));
    uint64_t round = std::max<uint64_t>(kRoundBytes / per_variant / 256 * 256, 256);
    round = std::min<uint64_t>(round, kRoundMax);
    return (uint32_t)std::min<uint64_t>(round, std::max<size_t>(batch, 1));
}

// The checked request on the process's plan: everything on `stream`, behind the last call's launches.
int enqueue_image(const double* x_dev, const uint8_t* ok_dev, size_t batch, size_t n_vars, const EzpzDrawItem* items, size_t n_items,
                  const EzpzImageView& view, uint32_t n_layers, bool accumulate, uint32_t* counts_dev, EzpzImageInfo* info_dev,
                  hipStream_t stream) {
    ImagePlan* P = nullptr;
    int device = -1;
    if (int rc = plan_of_device(P, device)) return rc;
    release_thread_kernel(device);
    std::lock_guard<std::mutex> lock(P->mu);
    P->device = device;
    ImageWork& W = P->work;
    int rc;
    const uint32_t round = round_of(batch, n_items);
    const size_t slots = (size_t)round * n_items, item_bytes = n_items * sizeof(EzpzDrawItem);
    const bool same_items = W.items_kept.size() == item_bytes && (!item_bytes || (W.items.p && !std::memcmp(W.items_kept.data(), items, item_bytes)));
    if (!same_items || slots * kParams > W.packed.cap || slots * 4 > W.boxes.cap || n_items > W.item_box.cap) {
        // another list, or a buffer that has to grow: the last call's launches first
        if ((rc = P->order.before_overwrite()) != EZPZ_OK) return rc;
        W.items_kept.clear();
        if ((rc = W.packed.ensure(slots * kParams)) != EZPZ_OK || (rc = W.boxes.ensure(slots * 4)) != EZPZ_OK ||
            (rc = W.item_box.ensure(n_items)) != EZPZ_OK || (rc = W.items.ensure(n_items)) != EZPZ_OK)
            return rc;
        if (item_bytes) HIP_TRY(hipMemcpy(W.items.p, items, item_bytes, hipMemcpyHostToDevice));
        W.items_kept.assign((const unsigned char*)items, (const unsigned char*)items + item_bytes);
        call_stamp(IMAGE_WORKSPACE_GROWN);
    }
    if ((rc = P->order.order_behind(stream)) != EZPZ_OK) return rc;
    if (!accumulate) {
        HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)n_layers * view.width * view.height * sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(info_dev, 0, sizeof(EzpzImageInfo), stream));
    }
    const uint32_t tiles = ((view.width + kTile - 1) / kTile) * ((view.height + kTile - 1) / kTile);
    for (size_t first = 0; first < batch; first += round) {
        RoundArgs a{};
        a.x = x_dev ? x_dev + first * n_vars : nullptr;
        a.ok = ok_dev ? ok_dev + first : nullptr;
        a.count = (uint32_t)std::min<size_t>(round, batch - first);
        a.n_vars = (uint32_t)n_vars;
        a.view = view;
        a.counts = counts_dev;
        a.info = info_dev;
        const uint32_t slices = std::min<uint32_t>((a.count + kSliceVariants - 1) / kSliceVariants, kMaxSlices);
        a.per_slice = (a.count + slices - 1) / slices;
        // (an empty list still has its variants and its masked ones counted: one launch of pass 1 with no items)
        for (size_t item0 = 0; item0 == 0 || item0 < n_items; item0 += kItemsPerLaunch) {
            a.n_items = (uint32_t)std::min<size_t>(kItemsPerLaunch, n_items - item0);
            a.count_info = item0 == 0;
            a.items = W.items.p + item0;
            a.packed = W.packed.p + item0 * a.count * kParams;
            a.boxes = W.boxes.p + item0 * a.count * 4;
            a.item_box = W.item_box.p + item0;
            if (a.n_items) HIP_TRY(hipMemsetAsync(a.item_box, 0xFF, a.n_items * sizeof(ItemBox), stream));
            hipLaunchKernelGGL(pack_kernel, dim3((a.count + 255) / 256, std::max<uint32_t>(a.n_items, 1)), dim3(256), 0, stream, a);
            if (a.n_items) hipLaunchKernelGGL(raster_kernel, dim3(tiles, a.n_items, slices), dim3(256), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
    }
    call_stamp(IMAGE_LAUNCHED);
    return P->order.record(stream);
}

}  // namespace

extern "C" {

int ezpz_sketch_image_device(const double* x_dev, const uint8_t* ok_dev, size_t batch, size_t n_vars, const EzpzDrawItem* items,
                             size_t n_items, const EzpzImageView* view, uint32_t n_layers, int accumulate, uint32_t* counts_dev,
                             EzpzImageInfo* info_dev, void* stream) {
    if (int rc = check_request(x_dev, batch, n_vars, items, n_items, view, n_layers, counts_dev, info_dev)) return rc;
    return enqueue_image(x_dev, ok_dev, batch, n_vars, items, n_items, *view, n_layers, accumulate != 0, counts_dev, info_dev, (hipStream_t)stream);
}

int ezpz_sketch_image(const double* x, const uint8_t* ok, size_t batch, size_t n_vars, const EzpzDrawItem* items, size_t n_items,
                      const EzpzImageView* view, uint32_t n_layers, int accumulate, uint32_t* counts, EzpzImageInfo* info) {
    if (int rc = check_request(x, batch, n_vars, items, n_items, view, n_layers, counts, info)) return rc;
    ImagePlan* P = nullptr;
    int device = -1;
    if (int rc = plan_of_device(P, device)) return rc;
    ImageWork& W = P->work;
    std::lock_guard<std::mutex> lock(W.host_mu);
    const hipStream_t stream = hipStreamPerThread;
    const size_t cells = (size_t)n_layers * view->width * view->height;
    const bool draws = batch && n_items;  // (without items the variants are only counted: nothing of x is read)
    int rc;
    Staged io;
    uint32_t* counts_dev = nullptr;
    EzpzImageInfo* info_dev = nullptr;
    // The outputs stand in front of the round's variants, so that every round finds them at the same place; round 0 uploads them
    // where the call accumulates, the others keep their room.
    size_t first = 0;
    do {
        const size_t count = std::min(kHostRound, batch - first);
        if (first) HIP_TRY(hipStreamSynchronize(stream));  // (the last round has read the buffers)
        const double* x_dev = nullptr;
        const uint8_t* ok_dev = nullptr;
        io = Staged{};
        io.inout(!first && accumulate ? counts : (const uint32_t*)nullptr, cells, counts, cells, counts_dev);
        io.inout(!first && accumulate ? info : (const EzpzImageInfo*)nullptr, 1, info, 1, info_dev);
        io.in(draws ? x + first * n_vars : nullptr, count * n_vars, x_dev, draws ? Staged::kPlaced : Staged::kAbsent);
        io.in(ok ? ok + first : nullptr, count, ok_dev);
        if ((rc = io.reserve(W.host_stage)) != EZPZ_OK || (rc = io.upload(W.host_stage)) != EZPZ_OK) return rc;
        if ((rc = enqueue_image(x_dev, ok_dev, count, n_vars, items, n_items, *view, n_layers, first || accumulate, counts_dev, info_dev, stream)) != EZPZ_OK)
            return rc;
        first += count;
    } while (first < batch);
    HIP_TRY(hipStreamSynchronize(stream));
    return io.copy_back(W.host_stage);
}

int ezpz_sketch_image_host(const double* x, const uint8_t* ok, size_t batch, size_t n_vars, const EzpzDrawItem* items, size_t n_items,
                           const EzpzImageView* view, uint32_t n_layers, int accumulate, uint32_t* counts, EzpzImageInfo* info) {
    if (int rc = check_request(x, batch, n_vars, items, n_items, view, n_layers, counts, info)) return rc;
    image_host(x, ok, batch, n_vars, items, n_items, *view, n_layers, accumulate != 0, counts, info);
    return EZPZ_OK;
}

int ezpz_sketch_compose(const uint32_t* counts, const EzpzImageView* view, uint32_t n_layers, const EzpzComposeLayer* layers,
                        const uint8_t background[3], uint8_t* rgb_out) {
    if (int rc = check_view(view, n_layers)) return rc;
    if (!counts || !layers || !background || !rgb_out) return EZPZ_ERR_INVALID_ARGUMENT;
    compose_host(counts, *view, n_layers, layers, background, rgb_out);
    return EZPZ_OK;
}

}  // extern "C"
