// ASan / UBSan driver for the closing step of the tolerance contributors (ezpz_amd/csrc/mc_moments.hip.hpp: mcm::contributors_host,
// the whole of ezpz_mc_contributors -- the entry forwards to it -- around mcm::contributors, the body that is also the one behind
// mc_contrib_kernel).  Host code only, run on the CPU: no device, no library --
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Iezpz_amd/csrc -Iinclude tools/asan_contrib.cpp -o /tmp/asan_contrib && /tmp/asan_contrib
// Every array is an allocation of exactly its size (so a read or write past its end is seen).  K sweeps 1 .. 64 with every flavour
// of moments: of random samples, with a zero-variance dimension, with duplicated dimensions, with a constant reference dimension,
// with n_complete of 0, 1 and 2, and sums that are no sample's (random, non-finite).  Every answer is checked for what the interface
// promises whatever the numbers: a symmetric cov, `dropped` inside the input block (or all ones), +0.0 coefficients and contributions
// for a dropped dimension, NaN for a reference dimension without variance.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#define EZPZ_MCM_HOST_ONLY
#include "mc_moments.hip.hpp"

using namespace ezpz;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static std::unique_ptr<double[]> exact(size_t n) { return std::unique_ptr<double[]>(new double[n]); }

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

int main() {
    std::mt19937_64 rng(20261020);
    std::normal_distribution<double> normal(0.0, 1.0);
    size_t runs = 0, dropped_seen = 0, few_seen = 0, nan_r2 = 0;
    for (uint32_t K = 1; K <= EZPZ_MC_MOMENT_MAX; ++K) {
        for (int flavour = 0; flavour < 9; ++flavour) {
            const uint32_t k = flavour == 8 ? 0 : (uint32_t)(rng() % (K + 1)), m = K - k;
            const size_t E = K + (size_t)K * (K + 1) / 2;
            uint64_t n = 40 + rng() % 100;
            if (flavour == 4) n = 0;
            if (flavour == 5) n = 1;
            if (flavour == 6) n = 2;
            // the samples: inputs, and references that answer to them
            std::vector<double> z((size_t)n * K);
            for (uint64_t b = 0; b < n; ++b) {
                for (uint32_t j = 0; j < k; ++j) z[b * K + j] = 0.1 * normal(rng);
                if (flavour == 1 && k) z[b * K + k - 1] = 0.0;                   // a zero-variance dimension (the last input)
                if (flavour == 2 && k >= 2) z[b * K + k - 1] = z[b * K];          // duplicated dimensions
                if (flavour == 2 && k >= 4) z[b * K + 2] = z[b * K + 1];
                for (uint32_t i = 0; i < m; ++i) {
                    double v = 0.01 * normal(rng);
                    for (uint32_t j = 0; j < k; ++j) v += ((i + j) % 3 - 1.0) * z[b * K + j];
                    z[b * K + k + i] = flavour == 3 && i == 0 ? 0.0 : v;  // a constant reference dimension
                }
            }
            auto mom = exact(E);
            for (uint32_t a = 0; a < K; ++a) {
                double s = 0.0;
                for (uint64_t b = 0; b < n; ++b) s += z[b * K + a];
                mom[a] = s;
            }
            size_t at = K;
            for (uint32_t a = 0; a < K; ++a)
                for (uint32_t c = a; c < K; ++c) {
                    double g = 0.0;
                    for (uint64_t b = 0; b < n; ++b) g += z[b * K + a] * z[b * K + c];
                    mom[at++] = g;
                }
            CHECK(at == E);
            if (flavour == 7) {  // sums that are no sample's
                for (size_t e = 0; e < E; ++e) mom[e] = normal(rng);
                mom[rng() % E] = std::numeric_limits<double>::infinity();
                mom[rng() % E] = std::nan("");
            }
            auto cov = exact((size_t)K * K), beta = exact((size_t)m * k), contrib = exact((size_t)m * k), r2 = exact(m);
            auto dropped = std::unique_ptr<uint64_t[]>(new uint64_t[1]);
            EzpzMcContribConfig cc;
            mcm::default_config(&cc);
            CHECK(cc.pivot_rel == 0x1p-26);
            if (K % 5 == 0) cc.pivot_rel = 0.0;
            const int rc = mcm::contributors_host(mom.get(), n, k, m, &cc, cov.get(), beta.get(), contrib.get(), r2.get(), dropped.get());
            CHECK(rc == EZPZ_OK);
            ++runs;
            if (n < 2) {
                ++few_seen;
                CHECK(dropped[0] == ~0ull);
                for (size_t e = 0; e < (size_t)K * K; ++e) CHECK(std::isnan(cov[e]));
                for (size_t e = 0; e < (size_t)m * k; ++e) CHECK(std::isnan(beta[e]) && std::isnan(contrib[e]));
                for (uint32_t i = 0; i < m; ++i) CHECK(std::isnan(r2[i]));
                continue;
            }
            CHECK(k == 64 || (dropped[0] >> k) == 0);
            dropped_seen += dropped[0] != 0;
            for (uint32_t a = 0; a < K; ++a)
                for (uint32_t c = 0; c < K; ++c) CHECK(same(cov[a * K + c], cov[c * K + a]));
            for (uint32_t i = 0; i < m; ++i) {
                const bool has_var = cov[(size_t)(k + i) * K + k + i] > 0.0;
                if (!has_var) {
                    CHECK(std::isnan(r2[i]));
                    ++nan_r2;
                }
                for (uint32_t j = 0; j < k; ++j) {
                    if (!has_var) CHECK(std::isnan(contrib[(size_t)i * k + j]));
                    if ((dropped[0] >> j) & 1u) {
                        CHECK(beta[(size_t)i * k + j] == 0.0 && !std::signbit(beta[(size_t)i * k + j]));
                        if (has_var) CHECK(contrib[(size_t)i * k + j] == 0.0);
                    }
                }
            }
            if (flavour == 1 && k) CHECK((dropped[0] >> (k - 1)) & 1u);
            if (flavour == 2 && k >= 2 && n > 2) CHECK((dropped[0] >> (k - 1)) & 1u);
            if (flavour == 6 && k >= 2) CHECK(dropped[0] != 0);  // (two samples span one direction)
        }
    }
    // the argument errors touch nothing
    {
        auto one = exact(1);
        uint64_t d = 7;
        one[0] = 7.0;
        CHECK(mcm::contributors_host(one.get(), 5, 0, 0, nullptr, one.get(), one.get(), one.get(), one.get(), &d) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mcm::contributors_host(one.get(), 5, 33, 32, nullptr, one.get(), one.get(), one.get(), one.get(), &d) == EZPZ_ERR_INVALID_ARGUMENT);
        EzpzMcContribConfig bad{-1.0, 0};
        CHECK(mcm::contributors_host(one.get(), 5, 1, 0, &bad, one.get(), one.get(), one.get(), one.get(), &d) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(one[0] == 7.0 && d == 7);
    }
    CHECK(runs == 64 * 9 && dropped_seen > 60 && few_seen == 128 && nan_r2 > 20);
    std::printf("asan_contrib: %zu closing steps for K = 1 .. 64, %zu with dropped dimensions, %zu with fewer than two samples, %zu reference "
                "dimensions without variance: clean\n", runs, dropped_seen, few_seen, nan_r2);
    return 0;
}
