// ASan / UBSan driver for the host side of the Sobol tolerance indices (ezpz_amd/csrc/mc_sobol.hip.hpp: sobol::indices_host and
// sobol::sums_host, the whole of ezpz_mc_sobol_indices and ezpz_mc_sobol_sums -- the entries forward to them -- the first around
// sobol::indices, the body that is also the one behind mc_sobol_close_kernel).  Host code only, run on the CPU: no device, no library --
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Iezpz_amd/csrc -Iinclude tools/asan_sobol.cpp -o /tmp/asan_sobol && /tmp/asan_sobol
// Every array is an allocation of exactly its size (so a read or write past its end is seen).  k sweeps 0 .. 32 with m drawn from
// 1 .. 32 and sample counts around a block of 256; the rows carry every cause of an incomplete sample, FIXED dimensions, and a
// record that is constant.  Every answer is checked for what the interface promises whatever the numbers: +0.0 entries and indices
// for a FIXED dimension, n_complete within the samples, NaN for a record with fewer than two complete samples or no variance, a
// total-effect index that is not negative.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#define EZPZ_SOBOL_HOST_ONLY
#include "mc_sobol.hip.hpp"

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
    std::mt19937_64 rng(20261020);
    std::normal_distribution<double> normal(0.0, 1.0);
    const uint64_t counts[] = {0, 1, 2, 255, 256, 257, 700};
    size_t runs = 0, fixed_seen = 0, few_seen = 0, flat_seen = 0;
    for (uint32_t k = 0; k <= EZPZ_SOBOL_MAX; ++k) {
        for (int flavour = 0; flavour < 7; ++flavour) {
            const uint32_t m = k == EZPZ_SOBOL_MAX && flavour == 0 ? EZPZ_SOBOL_MAX : 1 + (uint32_t)(rng() % EZPZ_SOBOL_MAX), R = k + 2;
            const uint64_t samples = counts[flavour];
            const uint32_t W = sobol::width_of(k);
            uint32_t fixed_mask = 0;
            for (uint32_t j = 0; j < k; ++j)
                if (rng() % 4 == 0) fixed_mask |= 1u << j;
            const bool flat = flavour == 5;  // record 0 is constant
            auto f = exact<double>(samples * R * m);
            auto flags = exact<uint8_t>(samples * R * m);
            auto ok = exact<uint8_t>(samples * R);
            auto nominal = exact<double>(m);
            for (uint32_t i = 0; i < m; ++i) nominal[i] = normal(rng);
            for (uint64_t b = 0; b < samples; ++b)
                for (uint32_t r = 0; r < R; ++r) {
                    ok[b * R + r] = rng() % 40 ? 1 : 0;
                    for (uint32_t i = 0; i < m; ++i) {
                        const uint64_t at = (b * R + r) * m + i;
                        const bool copy = r >= 2 && ((fixed_mask >> (r - 2)) & 1u);
                        f[at] = copy ? f[(b * R) * m + i] : flat && i == 0 ? nominal[0] : nominal[i] + 0.1 * normal(rng);
                        flags[at] = (uint8_t)(rng() % 60 ? (rng() & 2u) : 1u);
                        if (rng() % 90 == 0) f[at] = rng() % 2 ? std::nan("") : std::numeric_limits<double>::infinity();
                    }
                }
            auto sums = exact<double>((size_t)m * W);
            auto n_complete = exact<uint64_t>(m);
            for (size_t e = 0; e < (size_t)m * W; ++e) sums[e] = 7.0;
            for (uint32_t i = 0; i < m; ++i) n_complete[i] = 7;
            const bool bare = flavour == 6;  // flags == NULL, ok == NULL
            CHECK(sobol::sums_host(f.get(), bare ? nullptr : flags.get(), bare ? nullptr : ok.get(), nominal.get(), fixed_mask, samples, k, m,
                                   sums.get(), n_complete.get()) == EZPZ_OK);
            ++runs;
            if (samples == 0) {  // nothing written
                for (size_t e = 0; e < (size_t)m * W; ++e) CHECK(sums[e] == 7.0);
                for (uint32_t i = 0; i < m; ++i) n_complete[i] = 0;
                for (size_t e = 0; e < (size_t)m * W; ++e) sums[e] = 0.0;
            }
            for (uint32_t i = 0; i < m; ++i) {
                CHECK(n_complete[i] <= samples);
                for (uint32_t j = 0; j < k; ++j)
                    if ((fixed_mask >> j) & 1u)
                        for (uint32_t c = 0; c < 4; ++c) CHECK(plus_zero(sums[sobol::sum_at(k, i, j, c)]));
            }
            fixed_seen += fixed_mask != 0;
            auto var = exact<double>(m), first = exact<double>((size_t)m * k), total = exact<double>((size_t)m * k);
            auto first_var = exact<double>((size_t)m * k), total_var = exact<double>((size_t)m * k);
            CHECK(sobol::indices_host(sums.get(), n_complete.get(), k, m, var.get(), first.get(), total.get(), first_var.get(), total_var.get()) ==
                  EZPZ_OK);
            for (uint32_t i = 0; i < m; ++i) {
                const bool few = n_complete[i] < 2, none = few || !(var[i] > 0.0);
                few_seen += few;
                flat_seen += !few && !(var[i] > 0.0);
                CHECK(few == std::isnan(var[i]));
                for (uint32_t j = 0; j < k; ++j) {
                    const size_t at = (size_t)i * k + j;
                    if (none) {
                        CHECK(std::isnan(first[at]) && std::isnan(total[at]) && std::isnan(first_var[at]) && std::isnan(total_var[at]));
                    } else if ((fixed_mask >> j) & 1u) {
                        CHECK(plus_zero(first[at]) && plus_zero(total[at]) && plus_zero(first_var[at]) && plus_zero(total_var[at]));
                    } else {
                        CHECK(total[at] >= 0.0 && std::isfinite(first[at]));
                    }
                }
            }
        }
    }
    // the argument errors touch nothing
    {
        auto one = exact<double>(4);
        auto n = exact<uint64_t>(1);
        for (int e = 0; e < 4; ++e) one[e] = 7.0;
        n[0] = 7;
        CHECK(sobol::sums_host(one.get(), nullptr, nullptr, one.get(), 0, 1, 33, 1, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(sobol::sums_host(one.get(), nullptr, nullptr, one.get(), 0, 1, 0, 0, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(sobol::sums_host(one.get(), nullptr, nullptr, one.get(), 0, 1, 0, 33, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(sobol::sums_host(one.get(), nullptr, nullptr, one.get(), 1, 1, 0, 1, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(sobol::sums_host(nullptr, nullptr, nullptr, one.get(), 0, 1, 0, 1, one.get(), n.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(sobol::indices_host(one.get(), n.get(), 33, 1, one.get(), one.get(), one.get(), one.get(), one.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(sobol::indices_host(one.get(), nullptr, 0, 1, one.get(), nullptr, nullptr, nullptr, nullptr) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(one[0] == 7.0 && one[3] == 7.0 && n[0] == 7);
        EzpzSobolConfig c{7, 7};
        sobol::default_config(&c);
        CHECK(c.seed_b == 0x9E3779B97F4A7C15ull && c.reserved == 0);
    }
    CHECK(runs == 33 * 7 && fixed_seen > 100 && few_seen > 100 && flat_seen >= 20);
    std::printf("asan_sobol: %zu reductions and closing steps for k = 0 .. 32, %zu with FIXED dimensions, %zu records with fewer than two "
                "complete samples, %zu without variance: clean\n", runs, fixed_seen, few_seen, flat_seen);
    return 0;
}
