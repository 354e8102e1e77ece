// ASan / UBSan driver for the layout of the host forms' staging list (ezpz_amd/csrc/host_stage.hpp: Staged::layout, place, each_in,
// each_out).  Host code only, run on the CPU: no device, no library --
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Iezpz_amd/csrc -Iinclude tools/asan_host_stage.cpp -o /tmp/asan_host_stage && /tmp/asan_host_stage
// Random lists of inputs, outputs, shared places and bare rooms over every element size the host forms stage -- 1, 4 and 8 bytes,
// EzpzStatus, EzpzGuardStep, the seek, moments' and branch structs -- with absent arrays, zero counts, either side of a shared place
// the larger, and places kept although empty.  The buffer is an allocation of exactly the reported size (so a copy past its end is
// seen); every input is copied in and every output out of its place.  Checked: a place is 256-byte aligned, no two overlap, NULL
// stands exactly for the absent entries, the total is the sum of the rounded sizes, what went in at a shared place comes out of it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

#include "ezpz_amd.h"
#define EZPZ_HOST_STAGE_LAYOUT_ONLY
#include "host_stage.hpp"

using namespace ezpz;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

namespace {

std::mt19937_64 rng(20261021);

enum Kind { IN, OUT, INOUT, ROOM };

// One entry of a random list with everything the checks need: host arrays of exactly their size, the caller's device pointer.
struct Item {
    virtual ~Item() = default;
    Kind kind = IN;
    bool kept = false;             // a place although empty
    size_t size = 0;               // of an element
    size_t count_in = 0, count_out = 0, count_room = 0;
    std::unique_ptr<unsigned char[]> host_in, host_out;  // (null: the array is absent)
    virtual const unsigned char* dev() const = 0;
    virtual void add(Staged& io) = 0;
    size_t bytes() const {  // what the place has to hold
        const size_t a = host_in ? count_in * size : 0, b = host_out ? count_out * size : 0;
        return kind == ROOM ? count_room * size : a > b ? a : b;
    }
    bool absent() const { return !kept && bytes() == 0; }
};

template <class T>
struct ItemOf : Item {
    T* dev_out = reinterpret_cast<T*>(16);  // (neither NULL nor a place: place() has to set it)
    const T* dev_in = reinterpret_cast<const T*>(16);
    const unsigned char* dev() const override { return reinterpret_cast<const unsigned char*>(kind == IN ? dev_in : dev_out); }
    void add(Staged& io) override {
        const Staged::Empty e = kept ? Staged::kPlaced : Staged::kAbsent;
        const T* in = reinterpret_cast<const T*>(host_in.get());
        T* out = reinterpret_cast<T*>(host_out.get());
        if (kind == IN) io.in(in, count_in, dev_in, e);
        if (kind == OUT) io.out(out, count_out, dev_out, e);
        if (kind == INOUT) io.inout(in, count_in, out, count_out, dev_out, e);
        if (kind == ROOM) io.room(count_room, dev_out);
    }
};

size_t some_count() {
    const unsigned pick = rng() % 8;
    return pick == 0 ? 0 : pick == 1 ? 1 : pick < 6 ? 1 + rng() % 70 : 1 + rng() % 3000;
}

template <class T>
std::unique_ptr<Item> make_item() {
    auto it = std::make_unique<ItemOf<T>>();
    it->size = sizeof(T);
    it->kind = (Kind)(rng() % 4);
    it->kept = it->kind != ROOM && rng() % 4 == 0;
    it->count_in = some_count(), it->count_out = some_count(), it->count_room = some_count();
    if (it->kind == INOUT && rng() % 3 == 0) it->count_out = it->count_in;
    const bool has_in = it->kind == IN || it->kind == INOUT, has_out = it->kind == OUT || it->kind == INOUT;
    // (an absent array now and then; new[0] is an array too: present, with no elements)
    if (has_in && rng() % 5) it->host_in.reset(new unsigned char[it->count_in * sizeof(T)]);
    if (has_out && rng() % 5) it->host_out.reset(new unsigned char[it->count_out * sizeof(T)]);
    if (it->host_in)
        for (size_t k = 0; k < it->count_in * sizeof(T); ++k) it->host_in[k] = (unsigned char)rng();
    return it;
}

std::unique_ptr<Item> random_item() {
    switch (rng() % 9) {
        case 0: return make_item<uint8_t>();
        case 1: return make_item<uint32_t>();
        case 2: return make_item<int32_t>();
        case 3: return make_item<double>();
        case 4: return make_item<uint64_t>();
        case 5: return make_item<EzpzStatus>();
        case 6: return make_item<EzpzGuardStep>();
        case 7: return make_item<EzpzSeekInfo>();
        default: return rng() % 2 ? make_item<EzpzBranch>() : rng() % 2 ? make_item<EzpzBranchInfo>() : make_item<EzpzMcMomentsInfo>();
    }
}

}  // namespace

int main() {
    size_t lists = 0, placed = 0, absent = 0, kept_empty = 0, shared = 0;
    for (int round = 0; round < 4000; ++round) {
        std::vector<std::unique_ptr<Item>> items;
        const size_t n_items = round % 50 == 0 ? 0 : 1 + rng() % 12;
        for (size_t k = 0; k < n_items; ++k) items.push_back(random_item());
        Staged io;
        for (auto& it : items) it->add(io);
        const size_t total = io.layout();
        size_t want_total = 0;
        for (auto& it : items) want_total += it->absent() ? 0 : ((it->bytes() ? it->bytes() : 1) + 255) / 256 * 256;
        CHECK(total == want_total);
        CHECK(total % 256 == 0);
        // an allocation of exactly `total` bytes, as aligned as the device's
        unsigned char* base = total ? static_cast<unsigned char*>(std::aligned_alloc(256, total)) : nullptr;
        CHECK(!total || base);
        if (total) std::memset(base, 0xEE, total);
        io.place(base);
        for (size_t a = 0; a < items.size(); ++a) {
            const Item& A = *items[a];
            CHECK((A.dev() == nullptr) == A.absent());
            if (A.absent()) {
                ++absent;
                continue;
            }
            ++placed;
            if (!A.bytes()) ++kept_empty;
            CHECK(reinterpret_cast<uintptr_t>(A.dev()) % 256 == 0);
            CHECK(A.dev() >= base && A.dev() + A.bytes() <= base + total);
            for (size_t b = 0; b < a; ++b) {
                const Item& B = *items[b];
                if (B.absent()) continue;
                const size_t room_a = A.bytes() ? A.bytes() : 1, room_b = B.bytes() ? B.bytes() : 1;
                CHECK(A.dev() + room_a <= B.dev() || B.dev() + room_b <= A.dev());
            }
        }
        size_t copied_in = 0, copied_out = 0, want_in = 0, want_out = 0;
        CHECK(io.each_in(base, [&](void* dst, const void* src, size_t bytes) {
            std::memcpy(dst, src, bytes);
            copied_in += bytes;
            return 0;
        }) == 0);
        for (auto& it : items)
            if (it->host_in && it->count_in) CHECK(std::memcmp(it->dev(), it->host_in.get(), it->count_in * it->size) == 0);
        CHECK(io.each_out(base, [&](void* dst, const void* src, size_t bytes) {
            std::memcpy(dst, src, bytes);
            copied_out += bytes;
            return 0;
        }) == 0);
        for (auto& it : items) {
            want_in += it->host_in ? it->count_in * it->size : 0;
            want_out += it->host_out ? it->count_out * it->size : 0;
            if (it->host_out && it->count_out) CHECK(std::memcmp(it->host_out.get(), it->dev(), it->count_out * it->size) == 0);
            if (it->kind == INOUT && it->host_in && it->host_out) {  // what went in comes out, as far as both reach
                const size_t both = (it->count_in < it->count_out ? it->count_in : it->count_out) * it->size;
                CHECK(std::memcmp(it->host_out.get(), it->host_in.get(), both) == 0);
                ++shared;
            }
        }
        CHECK(copied_in == want_in && copied_out == want_out);
        std::free(base);
        ++lists;
    }
    CHECK(placed > 1000 && absent > 1000 && kept_empty > 100 && shared > 100);
    std::printf("asan_host_stage: %zu lists, %zu places (%zu kept although empty), %zu absent entries, %zu shared places: ok\n", lists, placed,
                kept_empty, absent, shared);
    return 0;
}
