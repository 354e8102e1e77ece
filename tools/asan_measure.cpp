// ASan / UBSan driver for the host side of the reference dimensions (ezpz_amd/csrc/measure_tables.hpp): random record lists,
// invalid ones among them, through the list check and table packer, the CSR builder and ezpz_constraint_measure's body.  Host
// code only, run on the CPU: no device, no library --
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Iezpz_amd/csrc -Iinclude tools/asan_measure.cpp -o /tmp/asan_measure && /tmp/asan_measure
// Every list is copied into an allocation of exactly its size (so a read past its end is seen), every packed table and CSR is
// checked against a direct restatement, and every measurable record is measured at random values and at a collapsed configuration.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

#include "measure_tables.hpp"

using namespace ezpz;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

int main() {
    std::mt19937_64 rng(20251019);
    auto below = [&](uint64_t n) { return (uint32_t)(rng() % n); };
    size_t valid = 0, invalid = 0, measured = 0, flagged = 0;
    for (int round = 0; round < 4000; ++round) {
        const size_t n_vars = 1 + below(round % 7 == 0 ? 3 : 40);
        const size_t n_meas = below(round % 5 == 0 ? 400 : 12);
        // what is wrong with this list, if anything: 0 nothing, 1 a kind without a parameter, 2 an angle kind's parallel tag,
        // 3 an id past the variables, 4 a kind past the table, 5 no list at all
        const int fault = round % 3 == 0 ? 1 + (int)below(5) : 0;
        const size_t at = n_meas ? below(n_meas) : 0;
        std::unique_ptr<EzpzConstraint[]> recs(new EzpzConstraint[n_meas]);
        for (size_t i = 0; i < n_meas; ++i) {
            EzpzConstraint& c = recs[i];
            std::memset(&c, 0, sizeof c);
            do {
                c.kind = (uint16_t)below(25);
                c.tag = (uint8_t)below(4);
            } while (!kind_has_param(c.kind, c.tag));
            for (int s = 0; s < 8; ++s) c.ids[s] = s < kKinds[c.kind].n_ids ? below(n_vars) : 0xFFFFFFFFu;  // (unused ids are never read)
            c.param = NAN;  // ignored
            c.weight = -1.0;
            if (fault && i == at) {
                if (fault == 1) c.kind = EZPZ_MIDPOINT;
                if (fault == 2) c.kind = EZPZ_ARC_ANGLE, c.tag = EZPZ_ANGLE_PERPENDICULAR;
                if (fault == 3) c.ids[kKinds[c.kind].n_ids - 1] = (uint32_t)n_vars + below(3);
                if (fault == 4) c.kind = (uint16_t)(25 + below(1000));
            }
        }
        std::vector<uint32_t> words;
        const int rc = measure_pack_records(fault == 5 ? nullptr : recs.get(), n_meas, n_vars, words);
        if (fault && n_meas) {
            CHECK(rc == EZPZ_ERR_INVALID_ARGUMENT);
            ++invalid;
            continue;
        }
        CHECK(rc == EZPZ_OK && words.size() == n_meas * kMeasureRecWords);
        ++valid;
        for (size_t i = 0; i < n_meas; ++i) {
            const uint32_t* w = &words[i * kMeasureRecWords];
            CHECK((w[0] & 0xFFFFu) == recs[i].kind && ((w[0] >> 16) & 0xFFu) == recs[i].tag && (w[0] >> 24) == kKinds[recs[i].kind].n_ids);
            for (uint32_t s = 0; s < 8; ++s) CHECK(w[1 + s] == (s < (w[0] >> 24) ? recs[i].ids[s] : 0u));
        }
        std::vector<uint32_t> csr;
        measure_build_csr(words, n_vars, csr);
        CHECK(csr.size() >= n_vars + 1 && csr[0] == 0 && csr.size() == n_vars + 1 + csr[n_vars]);
        size_t named = 0;
        for (size_t v = 0; v < n_vars; ++v) {
            CHECK(csr[v] <= csr[v + 1]);
            for (uint32_t e = csr[v]; e < csr[v + 1]; ++e) {
                const uint32_t p = csr[n_vars + 1 + e];
                CHECK(p / 8 < n_meas && p % 8 < (words[(p / 8) * kMeasureRecWords] >> 24) && words[(p / 8) * kMeasureRecWords + 1 + p % 8] == v);
                CHECK(e == csr[v] || csr[n_vars + e] < p);  // ascending (record, slot)
                ++named;
            }
        }
        size_t slots = 0;
        for (size_t i = 0; i < n_meas; ++i) slots += words[i * kMeasureRecWords] >> 24;
        CHECK(named == slots);
        // the values: exactly n_vars doubles, random or all on one spot
        std::unique_ptr<double[]> x(new double[n_vars]);
        for (int collapsed = 0; collapsed < 2; ++collapsed) {
            for (size_t v = 0; v < n_vars; ++v) x[v] = collapsed ? 1.25 : (double)(int)below(2000) / 256.0 - 4.0;
            for (size_t i = 0; i < n_meas; ++i) {
                double m = NAN, g[8];
                int fl = -1;
                const int n_ids = constraint_measure_host(&recs[i], x.get(), &m, g, &fl);
                CHECK(n_ids == kKinds[recs[i].kind].n_ids && fl >= 0 && fl <= 3 && !std::isnan(m));
                for (int s = n_ids; s < 8; ++s) CHECK(g[s] == 0.0 && !std::signbit(g[s]));
                if (fl & 1) {
                    CHECK(m == 0.0);
                    for (int s = 0; s < 8; ++s) CHECK(g[s] == 0.0);
                    ++flagged;
                }
                ++measured;
            }
        }
        EzpzConstraint none;
        std::memset(&none, 0, sizeof none);
        none.kind = EZPZ_SYMMETRIC;
        CHECK(constraint_measure_host(&none, x.get(), nullptr, nullptr, nullptr) == 0);
        CHECK(constraint_measure_host(nullptr, x.get(), nullptr, nullptr, nullptr) == 0);
        if (n_meas) CHECK(constraint_measure_host(&recs[0], nullptr, nullptr, nullptr, nullptr) == 0);
    }
    std::printf("asan_measure: %zu valid lists, %zu invalid ones refused, %zu measurements (%zu flagged)\n", valid, invalid, measured, flagged);
    return 0;
}
