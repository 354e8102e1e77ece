// ASan / UBSan driver for the host side of the factorial effects (ezpz_amd/csrc/mc_factorial.hip.hpp: mcf::factorial_host, the whole
// of ezpz_mc_factorial -- the entry forwards to it -- around mcf::record_of, the body that is also the one behind the device's
// closing thread).  Host code only, run on the CPU: no device, no library --
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Iezpz_amd/csrc -Iinclude tools/asan_factorial.cpp -o /tmp/asan_factorial && /tmp/asan_factorial
// Every array is an allocation of exactly its size (so a read or write past its end is seen).  The shapes: every n_corner from 1 to
// 12 at n_meas of 1, 3 and 32, random shapes beside them, with and without flags, ok and coef; the rows carry both zeros, a
// subnormal, a constant record and a record made incomplete by each cause -- ok == 0, flag bit 0, NaN, +inf -- at the first, a middle
// and the last row.  Every answer is checked for what the interface promises whatever the numbers: the counts, NaN and zero masks for
// an incomplete record, the symmetric pair with a +0.0 diagonal, the masks against the signs of main, m_hi and m_lo against the rows,
// ss_order summing to var, the indices inside [0, 1 + a rounding] and the argument errors leaving their outputs alone.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#define EZPZ_MCF_HOST_ONLY
#include "mc_factorial.hip.hpp"

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

static bool is_the_nan(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b == 0x7FF8000000000000ull;
}

static size_t runs = 0, records = 0, incomplete_seen = 0, constant_seen = 0;

// cause: 0 none, 1 ok == 0, 2 flag bit 0, 3 NaN, 4 +inf; place: 0 first, 1 middle, 2 last
static void one_case(std::mt19937_64& rng, uint32_t kc, uint32_t M, bool bare, bool with_coef, int cause, int place) {
    std::normal_distribution<double> normal(0.0, 1.0);
    const size_t N = (size_t)1 << kc;
    auto m = exact<double>(N * M);
    auto flags = exact<uint8_t>(N * M);
    auto ok = exact<uint8_t>(N);
    auto nominal = exact<double>(M);
    for (uint32_t i = 0; i < M; ++i) nominal[i] = normal(rng) * 2.0;
    for (size_t b = 0; b < N; ++b) {
        ok[b] = 1;
        for (uint32_t i = 0; i < M; ++i) {
            flags[b * M + i] = (uint8_t)((rng() & 1) * 2);  // (bit 1 is noise)
            m[b * M + i] = i == 1 ? nominal[1] + 0.375 : nominal[i] + normal(rng) * (i + 1);
        }
    }
    m[0] = -0.0, m[M] = 0.0;
    if (N >= 4) m[2 * M] = 5e-324 * 3;
    const uint32_t victim = M - 1 < 2 ? M - 1 : 2;
    const size_t where = place == 0 ? 0 : place == 1 ? N / 2 - 1 : N - 1;
    if (cause == 1 && !bare) ok[where] = 0;
    if (cause == 2 && !bare) flags[where * M + victim] |= 1;
    if (cause == 3) m[where * M + victim] = std::nan("");
    if (cause == 4) m[where * M + victim] = INFINITY;
    auto info = exact<EzpzMcFactorial>(M);
    auto mainv = exact<double>((size_t)M * kc);
    auto pair = exact<double>((size_t)M * kc * kc);
    auto ss_order = exact<double>((size_t)M * (kc + 1));
    auto ss_total = exact<double>((size_t)M * kc);
    auto first = exact<double>((size_t)M * kc);
    auto total = exact<double>((size_t)M * kc);
    auto coef = exact<double>(with_coef ? M * N : 0);
    CHECK(mcf::factorial_host(m.get(), bare ? nullptr : flags.get(), bare ? nullptr : ok.get(), nominal.get(), kc, M, info.get(), mainv.get(),
                              pair.get(), ss_order.get(), ss_total.get(), first.get(), total.get(), with_coef ? coef.get() : nullptr) == EZPZ_OK);
    ++runs;
    for (uint32_t i = 0; i < M; ++i) {
        ++records;
        size_t n = 0;
        for (size_t b = 0; b < N; ++b)
            n += (bare || ok[b]) && (bare || !(flags[b * M + i] & 1)) && std::isfinite(m[b * M + i]);
        const EzpzMcFactorial& r = info[i];
        CHECK(r.n_valid == n && r.complete == (n == N ? 1u : 0u) && r.reserved == 0);
        const double* mn = mainv.get() + (size_t)i * kc;
        if (!r.complete) {
            ++incomplete_seen;
            CHECK(r.corner_hi == 0 && r.corner_lo == 0 && is_the_nan(r.mean_dev) && is_the_nan(r.var) && is_the_nan(r.m_hi) && is_the_nan(r.m_lo));
            for (uint32_t c = 0; c < kc; ++c)
                CHECK(is_the_nan(mn[c]) && is_the_nan(ss_total[i * kc + c]) && is_the_nan(first[i * kc + c]) && is_the_nan(total[i * kc + c]));
            for (uint32_t e = 0; e < kc * kc; ++e) CHECK(is_the_nan(pair[(size_t)i * kc * kc + e]));
            for (uint32_t o = 0; o <= kc; ++o) CHECK(is_the_nan(ss_order[(size_t)i * (kc + 1) + o]));
            if (with_coef)
                for (size_t S = 0; S < N; ++S) CHECK(is_the_nan(coef[i * N + S]));
            continue;
        }
        uint32_t hi = 0, lo = 0;
        double var = 0.0;
        for (uint32_t c = 0; c < kc; ++c) {
            hi |= mn[c] > 0.0 ? 1u << c : 0u;
            lo |= mn[c] < 0.0 ? 1u << c : 0u;
            var += ss_order[(size_t)i * (kc + 1) + c + 1];
            const double* pr = pair.get() + (size_t)i * kc * kc;
            CHECK(pr[c * kc + c] == 0.0 && !std::signbit(pr[c * kc + c]));
            for (uint32_t e = 0; e < kc; ++e) CHECK(pr[c * kc + e] == pr[e * kc + c]);
            CHECK(first[i * kc + c] >= 0.0 && first[i * kc + c] <= total[i * kc + c] * (1.0 + 1e-12) + 1e-300 && total[i * kc + c] <= 1.0 + 1e-12);
            if (with_coef) CHECK(coef[i * N + ((size_t)1 << c)] == mn[c]);
        }
        CHECK(r.corner_hi == hi && r.corner_lo == lo && r.var == var && r.var >= 0.0);
        CHECK(r.m_hi == m[(size_t)hi * M + i] && r.m_lo == m[(size_t)lo * M + i]);
        if (with_coef) CHECK(coef[i * N] == r.mean_dev);
        if (i == 1) {
            ++constant_seen;
            CHECK(r.var == 0.0 && hi == 0 && lo == 0 && r.mean_dev == (nominal[1] + 0.375) - nominal[1]);
            for (uint32_t c = 0; c < kc; ++c) CHECK(first[i * kc + c] == 0.0 && total[i * kc + c] == 0.0);
        }
    }
}

int main() {
    std::mt19937_64 rng(20261021);
    const uint32_t meas[] = {1, 3, 32};
    for (uint32_t kc = 1; kc <= 12; ++kc)
        for (uint32_t M : meas) {
            one_case(rng, kc, M, false, true, 0, 0);
            one_case(rng, kc, M, true, false, 0, 0);
            for (int cause = 1; cause <= 4; ++cause)
                for (int place = 0; place < 3; ++place) one_case(rng, kc, M, cause >= 3 && (place & 1), (cause + place) & 1, cause, place);
        }
    for (int r = 0; r < 200; ++r) {
        const uint32_t kc = 1 + (uint32_t)(rng() % 10), M = 1 + (uint32_t)(rng() % 32);
        one_case(rng, kc, M, rng() & 1, rng() & 1, (int)(rng() % 5), (int)(rng() % 3));
    }
    // the argument errors touch nothing: the outputs are one byte each, so any write is seen
    {
        auto m = exact<double>(2);
        auto nominal = exact<double>(1);
        m[0] = 1.0, m[1] = 2.0, nominal[0] = 0.0;
        auto info = exact<EzpzMcFactorial>(1);
        auto d = exact<double>(7);
        double* o[6] = {d.get(), d.get() + 1, d.get() + 2, d.get() + 4, d.get() + 5, d.get() + 6};
        CHECK(mcf::factorial_host(m.get(), nullptr, nullptr, nominal.get(), 1, 1, info.get(), o[0], o[1], o[2], o[3], o[4], o[5], nullptr) == EZPZ_OK);
        CHECK(info[0].complete == 1 && d[0] == 0.5 && d[1] == 0.0 && d[2] == 2.25 && d[3] == 0.25 && d[4] == 0.25 && d[5] == 1.0 && d[6] == 1.0);
        auto tiny = exact<unsigned char>(1);
        double* t = reinterpret_cast<double*>(tiny.get());
        EzpzMcFactorial* ti = reinterpret_cast<EzpzMcFactorial*>(tiny.get());
        CHECK(mcf::factorial_host(m.get(), nullptr, nullptr, nominal.get(), 0, 1, ti, t, t, t, t, t, t, t) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mcf::factorial_host(m.get(), nullptr, nullptr, nominal.get(), 21, 1, ti, t, t, t, t, t, t, t) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mcf::factorial_host(m.get(), nullptr, nullptr, nominal.get(), 1, 0, ti, t, t, t, t, t, t, t) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mcf::factorial_host(m.get(), nullptr, nullptr, nominal.get(), 1, 33, ti, t, t, t, t, t, t, t) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mcf::factorial_host(nullptr, nullptr, nullptr, nominal.get(), 1, 1, ti, t, t, t, t, t, t, t) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mcf::factorial_host(m.get(), nullptr, nullptr, nullptr, 1, 1, ti, t, t, t, t, t, t, t) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mcf::factorial_host(m.get(), nullptr, nullptr, nominal.get(), 1, 1, nullptr, t, t, t, t, t, t, t) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mcf::factorial_host(m.get(), nullptr, nullptr, nominal.get(), 1, 1, ti, t, t, nullptr, t, t, t, t) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mcf::factorial_host(m.get(), nullptr, nullptr, nominal.get(), 1, 1, ti, t, t, t, t, t, nullptr, t) == EZPZ_ERR_INVALID_ARGUMENT);
    }
    CHECK(incomplete_seen > 100 && constant_seen > 50);
    std::printf("asan_factorial: %zu runs, %zu records (%zu incomplete, %zu constant): clean\n", runs, records, incomplete_seen, constant_seen);
    return 0;
}
