// ASan / UBSan driver for the host side of the Monte-Carlo quantiles (ezpz_amd/csrc/mc_quantiles.hip.hpp: mcq::quantiles_host, the
// whole of ezpz_mc_quantiles -- the entry forwards to it -- around mcq::ranks_of and mcq::record_of, the body that is also the one
// behind the device's closing threads).  Host code only, run on the CPU: no device, no library --
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Iezpz_amd/csrc -Iinclude tools/asan_quantiles.cpp -o /tmp/asan_quantiles && /tmp/asan_quantiles
// Every array is an allocation of exactly its size (so a read or write past its end is seen).  The shapes are the tests': samples 0,
// 1, 2, 255, 256, 257 and 1000, (n_meas, n_q) of (1, 1), (3, 5) and (64, 16), z of 0 and 3, with and without flags and ok; the rows
// carry every cause of an invalid sample, ties, both zeros, a subnormal, a record without a valid sample and one with exactly one.
// Every answer is checked for what the interface promises whatever the numbers: ranks inside [0, n), rank_lo <= rank <= rank_hi,
// lo <= value <= hi inside [band_lo, band_hi], and the order statistics against a sort done here.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#define EZPZ_QUANTILES_HOST_ONLY
#include "mc_quantiles.hip.hpp"

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

int main() {
    std::mt19937_64 rng(20261020);
    std::normal_distribution<double> normal(0.0, 1.0);
    const uint64_t counts[] = {0, 1, 2, 255, 256, 257, 1000};
    const uint32_t shapes[][2] = {{1, 1}, {3, 5}, {64, 16}};
    const double all_probs[16] = {0.0, 1.0, 0.5, 0.00135, 0.99865, 1e-12, 0.25, 0.75, 0.1, 0.9, 1.0 / 3.0, 1.0 - 0x1p-53, 0.01, 0.99, 0.05, 0.618};
    size_t runs = 0, records = 0, empty_seen = 0, single_seen = 0;
    for (const auto& shape : shapes)
        for (uint64_t samples : counts)
            for (int flavour = 0; flavour < 4; ++flavour) {
                const uint32_t m = shape[0], n_q = shape[1];
                const bool bare = flavour & 1;  // flags == NULL, ok == NULL
                const double z = flavour & 2 ? 3.0 : 0.0;
                auto v = exact<double>(samples * m);
                auto flags = exact<uint8_t>(samples * m);
                auto ok = exact<uint8_t>(samples);
                auto probs = exact<double>(n_q);
                for (uint32_t q = 0; q < n_q; ++q) probs[q] = all_probs[q];
                for (uint64_t b = 0; b < samples; ++b) {
                    ok[b] = rng() % 11 ? 1 : 0;
                    for (uint32_t i = 0; i < m; ++i) {
                        const uint64_t at = b * m + i;
                        const uint64_t pick = rng() % 16;
                        v[at] = pick < 6 ? 0.125 * (i + 1) : pick == 6 ? -0.0 : pick == 7 ? 0.0 : pick == 8 ? 5e-324 : normal(rng) * (i + 1);
                        flags[at] = (uint8_t)(rng() % 9 ? (rng() & 2u) : 1u);
                        if (rng() % 13 == 0) v[at] = rng() % 2 ? std::nan("") : std::numeric_limits<double>::infinity();
                        if (m > 2 && i == 1) flags[at] = 1;                                      // a record without a valid sample
                        if (m > 2 && i == 2) flags[at] = b == samples / 2 ? 0 : 1, v[at] = 4.5;  // ... and one with exactly one
                    }
                    if (m > 2 && b == samples / 2) ok[b] = 1;
                }
                auto out = exact<EzpzMcQuantile>((size_t)m * n_q);
                for (size_t e = 0; e < (size_t)m * n_q; ++e) out[e] = EzpzMcQuantile{7, 7, 7, 7, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0};
                EzpzMcQuantileConfig qc{z, 0};
                CHECK(mcq::quantiles_host(v.get(), bare ? nullptr : flags.get(), bare ? nullptr : ok.get(), samples, m, probs.get(), n_q, &qc,
                                          out.get()) == EZPZ_OK);
                ++runs;
                for (uint32_t i = 0; i < m; ++i) {
                    std::vector<uint64_t> keys;
                    for (uint64_t b = 0; b < samples; ++b) {
                        const uint64_t at = b * m + i;
                        if ((!bare && (!ok[b] || (flags[at] & 1u))) || !std::isfinite(v[at])) continue;
                        keys.push_back(mcq::key_of_bits(mcq::bits_of(v[at])));
                    }
                    std::sort(keys.begin(), keys.end());
                    const uint64_t n = keys.size();
                    for (uint32_t q = 0; q < n_q; ++q) {
                        const EzpzMcQuantile& r = out[(size_t)i * n_q + q];
                        if (samples == 0) {  // nothing written
                            CHECK(r.n_valid == 7 && r.value == 7.0);
                            continue;
                        }
                        ++records;
                        CHECK(r.n_valid == n);
                        if (n == 0) {
                            ++empty_seen;
                            CHECK(r.rank == UINT64_MAX && r.rank_lo == UINT64_MAX && r.rank_hi == UINT64_MAX);
                            CHECK(std::isnan(r.frac) && std::isnan(r.lo) && std::isnan(r.hi) && std::isnan(r.value) && std::isnan(r.band_lo) &&
                                  std::isnan(r.band_hi));
                            continue;
                        }
                        single_seen += n == 1;
                        CHECK(r.rank_lo <= r.rank && r.rank <= r.rank_hi && r.rank_hi < n && r.frac >= 0.0 && r.frac < 1.0);
                        CHECK(z != 0.0 || r.rank_lo == r.rank);
                        CHECK(mcq::key_of_bits(mcq::bits_of(r.lo)) == keys[r.rank]);
                        CHECK(mcq::key_of_bits(mcq::bits_of(r.hi)) == keys[std::min<uint64_t>(r.rank + 1, n - 1)]);
                        CHECK(mcq::key_of_bits(mcq::bits_of(r.band_lo)) == keys[r.rank_lo]);
                        CHECK(mcq::key_of_bits(mcq::bits_of(r.band_hi)) == keys[r.rank_hi]);
                        CHECK(r.lo <= r.value && r.value <= r.hi && r.band_lo <= r.lo && r.value <= r.band_hi);
                    }
                }
            }
    // the shared body at the ends of its domain
    {
        const mcq::Ranks a = mcq::ranks_of(1, 0.5, 1e300), b = mcq::ranks_of(0xFFFFFFFFull, 1.0, 0.0), c = mcq::ranks_of(0xFFFFFFFFull, 0.5, 1e300);
        CHECK(a.k == 0 && a.k1 == 0 && a.k_lo == 0 && a.k_hi == 0 && a.g == 0.0);
        CHECK(b.k == 0xFFFFFFFEull && b.k1 == b.k && b.k_lo == b.k && b.k_hi == b.k && b.g == 0.0);
        CHECK(c.k_lo == 0 && c.k_hi == 0xFFFFFFFEull);
        CHECK(mcq::value_of_key(mcq::key_of_bits(mcq::bits_of(-0.0))) == 0.0 && std::signbit(mcq::value_of_key(mcq::key_of_bits(mcq::bits_of(-0.0)))));
        CHECK(mcq::key_of_bits(mcq::bits_of(-0.0)) + 1 == mcq::key_of_bits(mcq::bits_of(0.0)));
    }
    // the argument errors touch nothing
    {
        auto one = exact<double>(1);
        auto out = exact<EzpzMcQuantile>(1);
        one[0] = 0.5;
        out[0] = EzpzMcQuantile{7, 7, 7, 7, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0};
        auto many = exact<double>(17);
        for (int q = 0; q < 17; ++q) many[q] = 0.5;
        const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
        EzpzMcQuantileConfig good{0.0, 0}, neg{-1.0, 0}, zn{nan, 0}, zi{inf, 0};
        auto call = [&](const double* m, uint64_t samples, size_t n_meas, const double* probs, size_t n_q, const EzpzMcQuantileConfig* qc,
                        EzpzMcQuantile* o) { return mcq::quantiles_host(m, nullptr, nullptr, samples, n_meas, probs, n_q, qc, o); };
        CHECK(call(one.get(), 1, 0, one.get(), 1, &good, out.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(call(one.get(), 1, 65, one.get(), 1, &good, out.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(call(one.get(), 1, 1, many.get(), 17, &good, out.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(call(one.get(), 1ull << 32, 1, one.get(), 1, &good, out.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        for (double p : {-1e-300, 1.0000000000000002, nan, inf}) {
            auto bad = exact<double>(1);
            bad[0] = p;
            CHECK(call(one.get(), 1, 1, bad.get(), 1, &good, out.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        }
        for (const EzpzMcQuantileConfig* qc : {&neg, &zn, &zi}) CHECK(call(one.get(), 1, 1, one.get(), 1, qc, out.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(call(one.get(), 1, 1, nullptr, 1, &good, out.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(call(one.get(), 1, 1, one.get(), 1, &good, nullptr) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(call(nullptr, 1, 1, one.get(), 1, &good, out.get()) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(call(nullptr, 0, 1, one.get(), 1, &good, out.get()) == EZPZ_OK && call(one.get(), 1, 1, nullptr, 0, nullptr, nullptr) == EZPZ_OK);
        CHECK(out[0].n_valid == 7 && out[0].value == 7.0 && out[0].band_hi == 7.0);
        CHECK(call(one.get(), 1, 1, one.get(), 1, nullptr, out.get()) == EZPZ_OK && out[0].n_valid == 1 && out[0].value == 0.5);
        EzpzMcQuantileConfig c{7.0, 7};
        mcq::default_config(&c);
        CHECK(c.z == 0.0 && c.reserved == 0);
    }
    CHECK(runs == 3 * 7 * 4 && empty_seen > 100 && single_seen > 100);
    std::printf("asan_quantiles: %zu selections, %zu records checked against a sort, %zu without a valid sample, %zu with exactly one: clean\n",
                runs, records, empty_seen, single_seen);
    return 0;
}
