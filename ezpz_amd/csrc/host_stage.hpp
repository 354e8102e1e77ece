// The staging list behind every host form: which host array goes with which device argument.  in(),
// out() and inout() give each a place, in order, in one device buffer; reserve() makes the buffer hold them and hands out the
// places; upload() brings the inputs there and copy_back() every output home.  An absent entry -- no host array, or no elements --
// takes no room, has no place (NULL) and is not copied; kPlaced gives an entry a place although it is empty, for the device forms
// whose argument check wants a pointer there.  The list does not wait: the caller synchronises, on the stream it uses, between its
// launches and copy_back().  The layout -- layout(), place(), each_in(), each_out() -- touches no runtime (EZPZ_HOST_STAGE_LAYOUT_ONLY:
// a host program that wants it alone, tools/asan_host_stage.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#ifndef EZPZ_HOST_STAGE_LAYOUT_ONLY
#include "system.hpp"
#endif

namespace ezpz {

struct Staged {
    enum Empty { kAbsent, kPlaced };
    static constexpr size_t kAlign = 256;  // every place as aligned as an allocation of its own
    struct Entry {
        const void* host_in;
        size_t count_in;
        void* host_out;
        size_t count_out;
        size_t count, size;                  // the place's elements (the larger of the two sides that are there), and an element's bytes
        Empty empty;
        void* dev;                           // the caller's device pointer for this entry: a T** or const T**
        void (*set)(void*, unsigned char*);  // ... and how to set it
        size_t offset;

        size_t bytes_in() const { return host_in ? count_in * size : 0; }
        size_t bytes_out() const { return host_out ? count_out * size : 0; }
        bool placed() const { return empty == kPlaced || count * size; }
        size_t room() const { return placed() ? (std::max<size_t>(count * size, 1) + kAlign - 1) / kAlign * kAlign : 0; }
    };
    std::vector<Entry> entries;
    Staged() { entries.reserve(12); }  // (one allocation a list: no host form has more entries)

    template <class T>
    void in(const T* host, size_t count, const T*& dev, Empty empty = kAbsent) {
        entries.push_back(Entry{host, count, nullptr, 0, host ? count : 0, sizeof(T), empty, &dev, &set_as<const T>, 0});
    }
    template <class T>
    void out(T* host, size_t count, T*& dev, Empty empty = kAbsent) {
        entries.push_back(Entry{nullptr, 0, host, count, host ? count : 0, sizeof(T), empty, &dev, &set_as<T>, 0});
    }
    // one place that is uploaded into and copied back from: its room is the larger of the two
    template <class T>
    void inout(const T* host_in, size_t count_in, T* host_out, size_t count_out, T*& dev, Empty empty = kAbsent) {
        const size_t count = std::max(host_in ? count_in : 0, host_out ? count_out : 0);
        entries.push_back(Entry{host_in, count_in, host_out, count_out, count, sizeof(T), empty, &dev, &set_as<T>, 0});
    }
    // a place the list does not copy: its caller brings it home in a form of its own (copy_back_warn_log)
    template <class T>
    void room(size_t count, T*& dev) {
        entries.push_back(Entry{nullptr, 0, nullptr, 0, count, sizeof(T), kAbsent, &dev, &set_as<T>, 0});
    }

    // ---- the layout: no runtime call ----------------------------------------------------------------------------------------------
    size_t layout() {  // the buffer's bytes
        size_t bytes = 0;
        for (Entry& e : entries) {
            e.offset = bytes;
            bytes += e.room();
        }
        return bytes;
    }
    void place(unsigned char* base) const {
        for (const Entry& e : entries) e.set(e.dev, e.placed() ? base + e.offset : nullptr);
    }
    // copy(place, host, bytes) for every input / copy(host, place, bytes) for every output that has elements; the first error ends it
    template <class Copy>
    int each_in(unsigned char* base, Copy&& copy) const {
        for (const Entry& e : entries)
            if (e.bytes_in())
                if (int rc = copy(base + e.offset, e.host_in, e.bytes_in())) return rc;
        return 0;
    }
    template <class Copy>
    int each_out(const unsigned char* base, Copy&& copy) const {
        for (const Entry& e : entries)
            if (e.bytes_out())
                if (int rc = copy(e.host_out, base + e.offset, e.bytes_out())) return rc;
        return 0;
    }

#ifndef EZPZ_HOST_STAGE_LAYOUT_ONLY
    // ---- on the device (the buffer of an earlier host call is idle: it waited for its launches) -----------------------------------
    int reserve(DevBuf<unsigned char>& buf) {
        if (int rc = buf.ensure(layout())) return rc;
        place(buf.p);
        return EZPZ_OK;
    }
    int upload(const DevBuf<unsigned char>& buf) const {
        return each_in(buf.p, [](void* dst, const void* src, size_t bytes) -> int {
            HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
            return EZPZ_OK;
        });
    }
    int copy_back(const DevBuf<unsigned char>& buf) const {
        return each_out(buf.p, [](void* dst, const void* src, size_t bytes) -> int {
            HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
            return EZPZ_OK;
        });
    }
#endif

private:
    template <class T>
    static void set_as(void* slot, unsigned char* p) {
        *static_cast<T**>(slot) = reinterpret_cast<T*>(p);
    }
};

#ifndef EZPZ_HOST_STAGE_LAYOUT_ONLY
// A driven call's warning log home: of `warn_cap` entries a row only those the kernel wrote are meaningful -- n_warnings per row,
// capped -- and only they reach the caller's array.  `status`: the rows' statuses, already on the host.
inline int copy_back_warn_log(uint64_t* warn_log, const uint64_t* log_dev, const EzpzStatus* status, size_t rows, uint32_t warn_cap) {
    std::vector<uint64_t> log(rows * (size_t)warn_cap);
    HIP_TRY(hipMemcpy(log.data(), log_dev, log.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < rows; ++b)
        std::memcpy(warn_log + b * warn_cap, log.data() + b * warn_cap, std::min<size_t>(status[b].n_warnings, warn_cap) * sizeof(uint64_t));
    return EZPZ_OK;
}
#endif

}  // namespace ezpz
