// ASan / UBSan driver for the host side of the low-discrepancy draws (ezpz_amd/csrc/mc_sampler.hip.hpp: mc::check_dists and
// mc::sample_host, the whole of ezpz_mc_sample -- the entry forwards to it -- around mc::draw, the body that is also the one behind
// the device's sampler kernels; ezpz_amd/csrc/mc_sequence.hip.hpp: the point, the step, the inverse).  Host code only, run on the
// CPU: no device, no library --
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Iezpz_amd/csrc -Iinclude tools/asan_sequence.cpp -o /tmp/asan_sequence && /tmp/asan_sequence
// Every array is an allocation of exactly its size (so a read or write past its end is seen).  The lists are the edges of the rule:
// a flagged dimension at position 63 (the table's last row) and at 64 (refused), first + count at 2^32 (the table's last column, the
// index's last value) and one past it (refused), a truncation of 1 and none, the flag on FIXED and CORNER, every other bit of
// `reserved` set.  Every answer is checked for what the interface promises whatever the numbers: inside the distribution's range,
// finite, the walk equal to the direct evaluation, a refused call leaving its output as it was.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "mc_sampler.hip.hpp"

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

static const uint64_t kTop = 1ull << 32;
static const double kMark = 7.25;

// one call on exact allocations; returns the code, `out` [count][n] (marked before)
static int sample(uint64_t seed, const std::vector<EzpzMcDist>& list, uint64_t first, size_t count, std::vector<double>& out) {
    const size_t n = list.size();
    auto dist = exact<EzpzMcDist>(n);
    auto nominal = exact<double>(n);
    auto params = exact<double>(count * n);
    for (size_t j = 0; j < n; ++j) dist[j] = list[j], nominal[j] = 0.5 * (double)j;
    for (size_t e = 0; e < count * n; ++e) params[e] = kMark;
    const int rc = mc::sample_host(seed, dist.get(), nominal.get(), n, first, count, params.get());
    out.assign(params.get(), params.get() + count * n);
    return rc;
}

int main() {
    const EzpzMcDist plain_u{EZPZ_MC_UNIFORM, 0, -1.0, 1.0}, seq_u{EZPZ_MC_UNIFORM, EZPZ_MC_SEQUENCE, -1.0, 1.0};
    const EzpzMcDist seq_n{EZPZ_MC_NORMAL, EZPZ_MC_SEQUENCE, 2.0, 0.0}, seq_n1{EZPZ_MC_NORMAL, 0xFFFFFFFFu, 2.0, 1.0};
    const EzpzMcDist seq_fixed{EZPZ_MC_FIXED, EZPZ_MC_SEQUENCE, 0.0, 0.0}, seq_corner{EZPZ_MC_CORNER, EZPZ_MC_SEQUENCE, -1.0, 1.0};
    const EzpzMcDist other_bits{EZPZ_MC_UNIFORM, 0xFFFFFFFEu, -1.0, 1.0};
    std::vector<double> out, again;
    size_t calls = 0, draws = 0;

    // position 63 and 64, at the start, across 2^31 and at the end of the samples
    const uint64_t firsts[] = {0, 1, (1ull << 31) - 3, kTop - 6};
    for (uint64_t first : firsts)
        for (const EzpzMcDist& last : {seq_u, seq_n, seq_n1}) {
            std::vector<EzpzMcDist> list(63, plain_u);
            list[0] = seq_n, list[1] = seq_n1, list[2] = seq_fixed, list[3] = seq_corner, list[4] = other_bits, list[62] = seq_u;
            list.push_back(last);  // position 63
            CHECK(sample(0x5EED, list, first, 6, out) == EZPZ_OK);
            ++calls;
            for (size_t s = 0; s < 6; ++s)
                for (size_t j = 0; j < 64; ++j) {
                    const double dev = out[s * 64 + j] - 0.5 * (double)j;
                    const EzpzMcDist& d = list[j];
                    CHECK(std::isfinite(dev));
                    if (d.kind == EZPZ_MC_UNIFORM) CHECK(dev >= -1.0 - 1e-12 && dev <= 1.0 + 1e-12);
                    if (d.kind == EZPZ_MC_NORMAL && d.b != 0.0) CHECK(std::fabs(dev) <= 2.0 * d.b + 1e-12);
                    if (d.kind == EZPZ_MC_NORMAL && d.b == 0.0) CHECK(std::fabs(dev) <= 2.0 * 6.35);
                    if (d.kind == EZPZ_MC_FIXED) CHECK(dev == 0.0);
                    ++draws;
                }
            // one sample at a time gives the same bytes
            for (size_t s = 0; s < 6; ++s) {
                CHECK(sample(0x5EED, list, first + s, 1, again) == EZPZ_OK);
                for (size_t j = 0; j < 64; ++j) CHECK(again[j] == out[s * 64 + j]);
            }
            list.insert(list.begin(), plain_u);  // `last` at position 64
            CHECK(sample(0x5EED, list, first, 6, out) == EZPZ_ERR_INVALID_ARGUMENT);
            for (double v : out) CHECK(v == kMark);
            list.back() = last.kind == EZPZ_MC_UNIFORM ? seq_fixed : seq_corner;  // (ignored there)
            CHECK(sample(0x5EED, list, first, 6, out) == EZPZ_OK);
            calls += 8;
        }

    // first + count past 2^32
    const uint64_t past[][2] = {{kTop - 5, 6}, {kTop, 1}, {~0ull - 2, 6}, {0, 0}};
    for (const auto& p : past) {
        if (!p[1]) break;
        CHECK(sample(1, {plain_u, seq_n1}, p[0], (size_t)p[1], out) == EZPZ_ERR_INVALID_ARGUMENT);
        for (double v : out) CHECK(v == kMark);
        std::vector<mc::Dist> dists;
        const EzpzMcDist two[] = {plain_u, seq_n1};
        const double nominal[] = {0.0, 0.0};
        CHECK(mc::check_dists(two, nominal, 2, p[0], p[1], dists) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mc::check_dists(two, nominal, 2, p[0], 0, dists) == (p[0] > kTop ? EZPZ_ERR_INVALID_ARGUMENT : EZPZ_OK));
        const EzpzMcDist unflagged[] = {plain_u, other_bits};
        CHECK(mc::check_dists(unflagged, nominal, 2, p[0], p[1], dists) == EZPZ_OK);
        ++calls;
    }
    {
        std::vector<mc::Dist> dists;
        const EzpzMcDist two[] = {seq_u, seq_n1};
        const double nominal[] = {0.0, 0.0};
        CHECK(mc::check_dists(two, nominal, 2, 0, kTop, dists) == EZPZ_OK && dists.size() == 2);
        CHECK(dists[0].sequence == 1 && dists[1].sequence == 1 && dists[0].pad == 0 && dists[0].p_lo == 0.0 && dists[0].p_hi == 1.0);
        CHECK(dists[1].p_lo > 0.158 && dists[1].p_lo < 0.159 && dists[1].p_hi == 1.0 - dists[1].p_lo);
        CHECK(mc::check_dists(two, nominal, 2, 0, kTop + 1, dists) == EZPZ_ERR_INVALID_ARGUMENT);
        CHECK(mc::check_dists(two, nominal, 2, 1, kTop, dists) == EZPZ_ERR_INVALID_ARGUMENT);
    }

    // the walk against the direct evaluation, every row of the table, across every carry up to bit 31
    for (uint32_t j = 0; j < mc::kSequenceDims; ++j) {
        const uint32_t* v = mc::sequence_row(j);
        for (uint32_t c = 1; c < 32; ++c) {
            const uint32_t start = (c == 31 ? 0x80000000u : (1u << (c + 1))) - 3u;
            uint32_t x = mc::sequence_point(v, start);
            for (uint32_t b = start + 1; b != start + 6; ++b) {
                x = mc::sequence_step(v, x, b);
                CHECK(x == mc::sequence_point(v, b));
            }
        }
        uint32_t x = mc::sequence_point(v, 0xFFFFFFFAu);
        for (uint32_t b = 0xFFFFFFFBu; b != 0; ++b) {
            x = mc::sequence_step(v, x, b);
            CHECK(x == mc::sequence_point(v, b));
        }
    }

    // the inverse at both ends of the grid, at the branch points and around them
    const double ps[] = {mc::sequence_unit(0), mc::sequence_unit(0xFFFFFFFFu), 0.075, 0.925, std::nextafter(0.075, 0.0), std::nextafter(0.925, 1.0),
                         0.5, std::exp(-25.0), 1.0 - std::exp(-25.0), std::nextafter(std::exp(-25.0), 0.0), 1e-300, 0x1p-1074};
    double before = -INFINITY;
    std::vector<double> sorted(ps, ps + sizeof ps / sizeof *ps);
    std::sort(sorted.begin(), sorted.end());
    for (double p : sorted) {
        const double z = mc::normal_inverse(p);
        // (where two branches of the inverse meet, neighbouring p can come out a few ulp out of order: each is good to 1e-16)
        CHECK(std::isfinite(z) && (before == -INFINITY || z >= before - 0x1p-48 * std::fabs(before)));
        before = z;
    }
    CHECK(std::fabs(mc::normal_inverse(mc::sequence_unit(0)) + 6.338) < 1e-3 && mc::normal_inverse(0.5) == 0.0);
    std::printf("asan_sequence: %zu calls, %zu draws checked\n", calls, draws);
    return 0;
}
