// ASan / UBSan driver for the host side of the Monte-Carlo main effects (ezpz_amd/csrc/mc_effects.hip.hpp: mce::effects_host and
// mce::indices_host, the whole of ezpz_mc_effects and ezpz_mc_effect_indices -- the entries forward to them -- the second around
// mce::indices, the body that is also the one behind mc_effects_close_kernel).  Host code only, run on the CPU: no device, no library --
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Iezpz_amd/csrc -Iinclude tools/asan_effects.cpp -o /tmp/asan_effects && /tmp/asan_effects
// Every array is an allocation of exactly its size (so a read or write past its end is seen).  Random shapes (k, m, B) up to the
// limits -- 32 dimensions, 32 records, 64 bins, 4096 cells, each limit met exactly at least once -- with sample counts around a
// block of 256; the samples carry every cause of one that does not count, the edges repeat (a bin that stays empty), end in +inf
// (upper bins empty) or are all +inf (one bin), and one record is constant.  Every answer is checked for what the interface
// promises whatever the numbers: the bins' counts add up to the record's valid samples for every dimension, an empty cell is +0.0
// and its mean NaN, a dimension in one bin has bins_used == 1 and +0.0 indices, a constant record NaN ones.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#define EZPZ_MCE_HOST_ONLY
#include "mc_effects.hip.hpp"

using namespace ezpz;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

template <class T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

static bool plus_zero(double v) { return v == 0.0 && !std::signbit(v); }

int main() {
    std::mt19937_64 rng(20261021);
    std::normal_distribution<double> normal(0.0, 1.0);
    const double inf = std::numeric_limits<double>::infinity();
    const uint64_t sample_counts[] = {0, 1, 2, 255, 256, 257, 700};
    // the limits met exactly, then random shapes inside them
    std::vector<std::array<uint32_t, 3>> shapes = {{1, 1, 2}, {32, 32, 4}, {8, 8, 64}, {32, 1, 64}, {1, 32, 64}, {32, 2, 64}, {2, 32, 64}, {16, 16, 16}};
    while (shapes.size() < 64) {
        const uint32_t k = 1 + (uint32_t)(rng() % 32), m = 1 + (uint32_t)(rng() % 32), B = 2 + (uint32_t)(rng() % 63);
        if (k * B * m <= EZPZ_MC_EFFECT_MAX_CELLS) shapes.push_back({k, m, B});
    }
    size_t runs = 0, empty_seen = 0, one_bin_seen = 0, flat_seen = 0, partial_blocks = 0;
    for (size_t which = 0; which < shapes.size(); ++which) {
        const uint32_t k = shapes[which][0], m = shapes[which][1], B = shapes[which][2], cells = k * B * m;
        const uint64_t samples = sample_counts[which % 7];
        partial_blocks += samples % 256 != 0;
        const bool flat = which % 3 == 1;    // record 0 is constant
        const bool bare = which % 7 == 6;    // flags == NULL, ok == NULL
        auto params = exact<double>(samples * k);
        auto y = exact<double>(samples * m);
        auto flags = exact<uint8_t>(samples * m);
        auto ok = exact<uint8_t>(samples);
        auto nominal = exact<double>(m);
        auto edges = exact<double>((size_t)k * (B - 1));
        std::vector<bool> one_bin(k);
        for (uint32_t i = 0; i < m; ++i) nominal[i] = normal(rng);
        for (uint32_t j = 0; j < k; ++j) {
            const int kind = (int)(rng() % 4);  // 0: spread, 1: a repeated edge, 2: the upper edges +inf, 3: all +inf
            one_bin[j] = kind == 3;
            double at = -1.5;
            for (uint32_t e = 0; e + 1 < B; ++e) {
                if (!(kind == 1 && e == 1)) at += 3.0 / B * (0.5 + (double)(rng() % 100) / 100.0);
                edges[(size_t)j * (B - 1) + e] = kind == 3 || (kind == 2 && e >= (B - 1) / 2) ? inf : at;
            }
            if (kind == 0 && B > 2 && rng() % 2) edges[(size_t)j * (B - 1)] = -inf;
        }
        for (uint64_t b = 0; b < samples; ++b) {
            ok[b] = rng() % 40 ? 1 : 0;
            for (uint32_t j = 0; j < k; ++j) {  // (now and then a value exactly on an edge)
                const double on = edges[(size_t)j * (B - 1) + rng() % (B - 1)];
                params[b * k + j] = rng() % 50 || !std::isfinite(on) ? normal(rng) : on;
            }
            for (uint32_t i = 0; i < m; ++i) {
                y[b * m + i] = flat && i == 0 ? nominal[0] : nominal[i] + 0.1 * normal(rng) + 0.2 * params[b * k + i % k];
                flags[b * m + i] = (uint8_t)(rng() % 60 ? (rng() & 2u) : 1u);
                if (rng() % 90 == 0) y[b * m + i] = rng() % 2 ? std::nan("") : inf;
            }
        }
        auto sums = exact<double>((size_t)cells * 2);
        auto counts = exact<uint64_t>(cells);
        for (size_t e = 0; e < (size_t)cells * 2; ++e) sums[e] = 7.0;
        for (uint32_t e = 0; e < cells; ++e) counts[e] = 7;
        CHECK(mce::effects_host(params.get(), y.get(), bare ? nullptr : flags.get(), bare ? nullptr : ok.get(), nominal.get(), edges.get(), samples, k,
                                m, B, sums.get(), counts.get()) == EZPZ_OK);
        ++runs;
        if (samples == 0) {  // nothing written
            for (size_t e = 0; e < (size_t)cells * 2; ++e) CHECK(sums[e] == 7.0);
            for (uint32_t e = 0; e < cells; ++e) CHECK(counts[e] == 7);
            for (size_t e = 0; e < (size_t)cells * 2; ++e) sums[e] = 0.0;
            for (uint32_t e = 0; e < cells; ++e) counts[e] = 0;
        }
        // the valid samples of every record, counted here; every dimension's bins add up to them
        std::vector<uint64_t> n_valid(m, 0);
        for (uint64_t b = 0; b < samples; ++b)
            for (uint32_t i = 0; i < m; ++i)
                n_valid[i] += (bare || ok[b]) && (bare || !(flags[b * m + i] & 1u)) && std::isfinite(y[b * m + i]);
        for (uint32_t j = 0; j < k; ++j)
            for (uint32_t i = 0; i < m; ++i) {
                uint64_t n = 0;
                for (uint32_t c = 0; c < B; ++c) {
                    const uint32_t at = mce::cell_at(B, m, j, c, i);
                    n += counts[at];
                    if (!counts[at]) CHECK(plus_zero(sums[2 * at]) && plus_zero(sums[2 * at + 1]));
                    if (one_bin[j] && c) CHECK(!counts[at]);
                }
                CHECK(n == n_valid[i]);
            }
        auto cond_mean = exact<double>(cells), cond_var = exact<double>(cells);
        auto eta2 = exact<double>((size_t)m * k), first = exact<double>((size_t)m * k);
        auto used = exact<uint32_t>((size_t)m * k);
        CHECK(mce::indices_host(sums.get(), counts.get(), nominal.get(), k, m, B, cond_mean.get(), cond_var.get(), eta2.get(), first.get(),
                                used.get()) == EZPZ_OK);
        for (uint32_t e = 0; e < cells; ++e) {
            CHECK((counts[e] == 0) == std::isnan(cond_mean[e]) || !std::isfinite(sums[2 * (size_t)e]));
            if (counts[e] < 2) CHECK(std::isnan(cond_var[e]));
            empty_seen += counts[e] == 0;
        }
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = 0; j < k; ++j) {
                const size_t at = (size_t)i * k + j;
                CHECK(used[at] <= B);
                if (one_bin[j]) {
                    CHECK(used[at] == (n_valid[i] ? 1u : 0u));
                    ++one_bin_seen;
                }
                if (used[at] < 2) {
                    CHECK(plus_zero(eta2[at]) && plus_zero(first[at]));
                } else if (flat && i == 0) {
                    CHECK(std::isnan(eta2[at]) && std::isnan(first[at]));
                    ++flat_seen;
                } else if (n_valid[i] > used[at] && std::isfinite(eta2[at])) {
                    CHECK(eta2[at] >= 0.0 && first[at] <= eta2[at] + 1e-12);
                }
            }
    }
    // the argument errors touch nothing
    {
        auto one = exact<double>(4);
        auto n = exact<uint64_t>(2);
        auto u = exact<uint32_t>(1);
        for (int e = 0; e < 4; ++e) one[e] = 7.0;
        n[0] = n[1] = 7, u[0] = 7;
        const double nan_edge[1] = {std::nan("")}, down[2] = {1.0, 0.5}, fine[1] = {0.0};
        CHECK(mce::effects_host(one.get(), one.get(), nullptr, nullptr, one.get(), fine, 1, 0, 1, 2, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::effects_host(one.get(), one.get(), nullptr, nullptr, one.get(), fine, 1, 1, 0, 2, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::effects_host(one.get(), one.get(), nullptr, nullptr, one.get(), fine, 1, 33, 1, 2, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::effects_host(one.get(), one.get(), nullptr, nullptr, one.get(), fine, 1, 1, 1, 1, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::effects_host(one.get(), one.get(), nullptr, nullptr, one.get(), fine, 1, 1, 1, 65, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::effects_host(one.get(), one.get(), nullptr, nullptr, one.get(), fine, 1, 32, 32, 5, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::effects_host(one.get(), one.get(), nullptr, nullptr, one.get(), nan_edge, 1, 1, 1, 2, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::effects_host(one.get(), one.get(), nullptr, nullptr, one.get(), down, 1, 1, 1, 3, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::effects_host(nullptr, one.get(), nullptr, nullptr, one.get(), fine, 1, 1, 1, 2, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::effects_host(one.get(), one.get(), nullptr, nullptr, one.get(), nullptr, 1, 1, 1, 2, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::effects_host(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, 1, 2, nullptr, nullptr) == EZPZ_OK);
        CHECK(mce::indices_host(one.get(), n.get(), one.get(), 1, 1, 65, one.get(), one.get(), one.get(), one.get(), u.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::indices_host(one.get(), nullptr, one.get(), 1, 1, 2, one.get(), one.get(), one.get(), one.get(), u.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mce::indices_host(one.get(), n.get(), one.get(), 1, 1, 2, one.get(), one.get(), one.get(), one.get(), nullptr) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(one[0] == 7.0 && one[3] == 7.0 && n[0] == 7 && n[1] == 7 && u[0] == 7);
        EzpzMcEffectConfig c{7, 7};
        mce::default_config(&c);
        CHECK(c.bins == 8 && c.reserved == 0);
    }
    CHECK(runs == 64 && empty_seen > 1000 && one_bin_seen > 100 && flat_seen > 100 && partial_blocks > 30);
    std::printf("asan_effects: %zu reductions and closing steps up to 32 x 32 x 4 and 8 x 8 x 64, %zu of sample counts off a block, %zu empty "
                "cells, %zu pairs with a dimension in one bin, %zu of a constant record: clean\n", runs, partial_blocks, empty_seen, one_bin_seen,
                flat_seen);
    return 0;
}
