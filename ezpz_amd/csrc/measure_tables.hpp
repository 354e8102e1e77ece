// Reference dimensions, the host side that needs no device (measure.hip uses it under the system's lock, tools/asan_measure.cpp
// drives it under the sanitizers): the check of a record list, the packed table the kernels read, the variable -> (record, slot)
// CSR of the vector-Jacobian product, and ezpz_constraint_measure's body.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "constraint_measure.hip.hpp"
#include "kinds.hpp"

namespace ezpz {

constexpr uint32_t kMeasureRecWords = 9;        // kind | tag << 16 | n_ids << 24, then ids[8] with the unused ones 0
constexpr size_t kMeasureMaxRecords = 1u << 20;  // (record * 9 + word, record * 8 + slot and 256 systems' records stay inside 32 bits)

struct MeasureHostXs {
    const double* x;
    double operator[](uint32_t id) const { return x[id]; }
};

inline bool measurable(const EzpzConstraint& c) { return c.kind < 25 && kind_has_param(c.kind, c.tag); }

// The argument errors of a list, and the packed records: only kind, tag and the kind's ids are read (and compared, by a caller
// that repeats a list).  EZPZ_ERR_INVALID_ARGUMENT: records NULL with n_meas > 0, a record that is not measurable, an id >= n_vars.
inline int measure_pack_records(const EzpzConstraint* records, size_t n_meas, size_t n_vars, std::vector<uint32_t>& words) {
    words.clear();
    if (n_meas == 0) return EZPZ_OK;
    if (!records) return EZPZ_ERR_INVALID_ARGUMENT;
    if (n_meas > kMeasureMaxRecords) return EZPZ_ERR_TOO_LARGE;
    words.assign(n_meas * kMeasureRecWords, 0u);
    for (size_t i = 0; i < n_meas; ++i) {
        const EzpzConstraint& c = records[i];
        if (!measurable(c)) return EZPZ_ERR_INVALID_ARGUMENT;
        const uint32_t n_ids = kKinds[c.kind].n_ids;
        uint32_t* w = words.data() + i * kMeasureRecWords;
        w[0] = (uint32_t)c.kind | ((uint32_t)c.tag << 16) | (n_ids << 24);
        for (uint32_t s = 0; s < n_ids; ++s) {
            if (c.ids[s] >= n_vars) return EZPZ_ERR_INVALID_ARGUMENT;
            w[1 + s] = c.ids[s];
        }
    }
    return EZPZ_OK;
}

// csr[0 .. n_vars] offsets, then for every variable the pairs record * 8 + slot that name it, ascending (record, slot)
inline void measure_build_csr(const std::vector<uint32_t>& words, size_t n_vars, std::vector<uint32_t>& csr) {
    const size_t n_meas = words.size() / kMeasureRecWords;
    csr.assign(n_vars + 1, 0u);
    for (size_t i = 0; i < n_meas; ++i) {
        const uint32_t* w = words.data() + i * kMeasureRecWords;
        for (uint32_t s = 0; s < (w[0] >> 24); ++s) ++csr[w[1 + s] + 1];
    }
    for (size_t v = 0; v < n_vars; ++v) csr[v + 1] += csr[v];
    const size_t total = csr[n_vars];
    csr.resize(n_vars + 1 + total);
    std::vector<uint32_t> fill(csr.begin(), csr.begin() + n_vars);
    for (size_t i = 0; i < n_meas; ++i) {
        const uint32_t* w = words.data() + i * kMeasureRecWords;
        for (uint32_t s = 0; s < (w[0] >> 24); ++s) csr[n_vars + 1 + fill[w[1 + s]]++] = (uint32_t)(i * 8 + s);
    }
}

// ezpz_constraint_measure (include/ezpz_amd.h)
inline int constraint_measure_host(const EzpzConstraint* c, const double* x, double* m_out, double* grad_out, int* flags) {
    if (flags) *flags = 0;
    if (!c || !x || !measurable(*c)) return 0;
    double m, g[8];
    const uint32_t fl = measure::con_measure(c->kind, c->tag, c->ids, MeasureHostXs{x}, m, g);
    if (m_out) *m_out = m;
    if (grad_out)
        for (int s = 0; s < 8; ++s) grad_out[s] = g[s];
    if (flags) *flags = (int)fl;
    return kKinds[c->kind].n_ids;
}

}  // namespace ezpz
