// ASan / UBSan driver for the host side of the dimension targets' step (ezpz_amd/csrc/seek.hip.hpp: seek::step_host, the body
// behind ezpz_seek_step and, lane by lane, behind seek_step_kernel).  Host code only, run on the CPU: no device, no library --
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Iezpz_amd/csrc -Iinclude tools/asan_seek_step.cpp -o /tmp/asan_seek_step && /tmp/asan_seek_step
// Every array is copied into an allocation of exactly its size (so a read or write past its end is seen); shapes sweep n_param
// 1 .. 16 and n_meas 0 .. 64 with zero and duplicated columns, zero weights, active and frozen bounds, mixed scales, mu over
// 1e-12 .. 1e12 and non-finite entries.  Every step is checked for what the interface promises whatever the numbers: a known kind,
// p_trial inside [lo, hi], a held or PIVOT dimension left where it was with delta +0.0, p_trial = clamp(p + delta) elsewhere.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

#define EZPZ_SEEK_HOST_ONLY
#include "seek.hip.hpp"

using namespace ezpz;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static std::unique_ptr<double[]> exact(size_t n) { return std::unique_ptr<double[]>(new double[n]); }

int main() {
    std::mt19937_64 rng(20261020);
    std::normal_distribution<double> normal(0.0, 1.0);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    const double inf = std::numeric_limits<double>::infinity();
    size_t kinds[3] = {0, 0, 0}, held_seen = 0;
    for (int round = 0; round < 6000; ++round) {
        const uint32_t n = 1 + round % 16, k = round % 7 == 0 ? 0 : round % 5 == 0 ? 64 : (uint32_t)(rng() % 65);
        const int flavour = round % 9;
        auto p = exact(n), lo = exact(n), hi = exact(n), scale = exact(n), p_trial = exact(n), delta = exact(n);
        auto m = exact(k), t = exact(k), w = exact(k), D = exact((size_t)k * n);
        for (uint32_t r = 0; r < n; ++r) {
            p[r] = 3.0 * normal(rng);
            lo[r] = -inf, hi[r] = inf;
            scale[r] = round % 3 == 0 ? std::pow(10.0, 6.0 * unit(rng) - 3.0) : 1.0;
            if (flavour == 4 || flavour == 5) {
                const double u = unit(rng);
                if (u < 0.25) lo[r] = p[r];
                else if (u < 0.5) hi[r] = p[r];
                else if (u < 0.65) lo[r] = hi[r] = p[r];
                else if (u < 0.8) lo[r] = p[r] - 1e-3, hi[r] = p[r] + 1e-3;
            }
        }
        for (uint32_t i = 0; i < k; ++i) {
            m[i] = normal(rng);
            t[i] = m[i] + normal(rng);
            w[i] = flavour == 3 && unit(rng) < 0.5 ? 0.0 : 0.2 + 2.8 * unit(rng);
            for (uint32_t r = 0; r < n; ++r) D[(size_t)i * n + r] = normal(rng);
        }
        if (k) {
            const uint32_t c0 = (uint32_t)(rng() % n), c1 = (uint32_t)(rng() % n);
            for (uint32_t i = 0; i < k; ++i) {
                if (flavour == 1) D[(size_t)i * n + c0] = 0.0;
                if (flavour == 2) D[(size_t)i * n + c0] = D[(size_t)i * n + c1];
                if (flavour == 6) D[(size_t)i * n + c0] *= 1e160;
            }
            if (flavour == 7) D[(size_t)(rng() % k) * n + c0] = round % 2 ? std::nan("") : inf;
        }
        const double mu = flavour == 2 ? 1e-12 : std::pow(10.0, 24.0 * unit(rng) - 12.0);
        uint32_t held = 0xFFFFFFFFu;
        const int kind = seek::step_host(n, k, p.get(), m.get(), D.get(), t.get(), w.get(), lo.get(), hi.get(), scale.get(), mu, 1e-12,
                                         p_trial.get(), delta.get(), &held);
        CHECK(kind == EZPZ_SEEK_STEP_TRIAL || kind == EZPZ_SEEK_STEP_MINIMUM || kind == EZPZ_SEEK_STEP_PIVOT);
        CHECK((held >> n) == 0);
        ++kinds[kind];
        held_seen += held != 0;
        bool moved = false;
        for (uint32_t r = 0; r < n; ++r) {
            const bool is_held = (held >> r) & 1u;
            if (is_held || kind == EZPZ_SEEK_STEP_PIVOT) {
                CHECK(p_trial[r] == p[r] && delta[r] == 0.0 && !std::signbit(delta[r]));
            } else {
                const double q = p[r] + delta[r], c = q < lo[r] ? lo[r] : q > hi[r] ? hi[r] : q;
                CHECK(p_trial[r] == c && std::isfinite(delta[r]));
            }
            CHECK(p_trial[r] >= lo[r] && p_trial[r] <= hi[r]);
            moved = moved || p_trial[r] != p[r];
            if (lo[r] == hi[r]) CHECK(is_held);
        }
        if (kind == EZPZ_SEEK_STEP_TRIAL) CHECK(moved);
        if (k == 0) CHECK(kind == EZPZ_SEEK_STEP_MINIMUM);  // (nothing to learn from: a zero step)
    }
    CHECK(kinds[0] > 500 && kinds[1] > 100 && kinds[2] > 100 && held_seen > 300);
    std::printf("asan_seek_step: 6000 steps, %zu trial, %zu minimum, %zu pivot, %zu with held dimensions: clean\n", kinds[0], kinds[1], kinds[2],
                held_seen);
    return 0;
}
