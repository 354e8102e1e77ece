// hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Iezpz_amd/csrc -Iinclude tools/asan_driven_list.cpp ezpz_amd/csrc/driven.cpp -Lezpz_amd -lezpz_amd -Wl,-rpath,$PWD/ezpz_amd -o /tmp/asan_driven_list && /tmp/asan_driven_list
// The device-free part of driven.cpp under ASan + UBSan: driven_slot_map (the check of a `positions` list that every driven entry
// shares) and driven_request's route resolution, on systems built here without a device -- a few thousand random lists, valid and
// broken in each of the ways the entries decline, and every launch shape a request resolves.  The rest of the library is linked as
// built (its functions are not called); no device is touched.
#include <cstdio>
#include <numeric>
#include <random>

#include "driven_params.hpp"

static int fail(const char* what, int trial) {
    std::printf("trial %d: %s\n", trial, what);
    return 1;
}

int main() {
    std::mt19937_64 rng(7);
    auto below = [&](uint64_t n) { return (uint32_t)(rng() % n); };
    size_t lists = 0, declined = 0, requests = 0;
    for (int trial = 0; trial < 4000; ++trial) {
        EzpzSystem s;
        const uint32_t n_cs = trial % 50 == 0 ? 0 : 1 + below(300);
        s.host_has_param.resize(n_cs);
        std::vector<uint32_t> with, without;
        for (uint32_t i = 0; i < n_cs; ++i) {
            s.host_has_param[i] = below(4) != 0;
            (s.host_has_param[i] ? with : without).push_back(i);
        }
        std::shuffle(with.begin(), with.end(), rng);
        std::vector<uint32_t> pos(with.begin(), with.begin() + (with.empty() ? 0 : below(with.size() + 1)));
        std::vector<uint32_t> map;
        // a valid list: the map names every listed position's place and nothing else
        if (driven_slot_map(s, pos.empty() ? nullptr : pos.data(), pos.size(), map) != EZPZ_OK) return fail("a valid list was declined", trial);
        if (map.size() != std::max<size_t>(n_cs, 1)) return fail("the map's size", trial);
        size_t named = 0;
        for (uint32_t v : map) named += v != kNoParamSlot;
        for (size_t j = 0; j < pos.size(); ++j)
            if (map[pos[j]] != j) return fail("a place in the map", trial);
        if (named != pos.size()) return fail("a position that is not listed has a place", trial);
        ++lists;
        // the ways a list is declined
        std::vector<uint32_t> bad = pos;
        const int how = trial % 5;
        size_t n_bad = 0;
        const uint32_t* p_bad = nullptr;
        if (how == 0) bad.push_back(n_cs + below(3)), p_bad = bad.data(), n_bad = bad.size();          // past the constraints
        else if (how == 1 && !pos.empty()) bad.push_back(pos[below(pos.size())]), p_bad = bad.data(), n_bad = bad.size();  // twice
        else if (how == 2 && !without.empty()) bad.insert(bad.begin() + below(bad.size() + 1), without[below(without.size())]), p_bad = bad.data(), n_bad = bad.size();
        else if (how == 3) p_bad = nullptr, n_bad = 1 + below(5);                                       // no list
        else if (how == 4) bad.push_back(0), p_bad = bad.data(), n_bad = 0xFFFFFFFFull + below(3);      // too long: never read
        if (n_bad) {
            if (driven_slot_map(s, p_bad, n_bad, map) != EZPZ_ERR_INVALID_ARGUMENT) return fail("a broken list was accepted", trial);
            ++declined;
        }
        // the routes a request resolves (no program is deferred on these systems: ensure_program has nothing to build)
        DrivenRequest r;
        uint32_t want = 0;
        bool decline = false;
        const int shape = trial % 7;
        s.rec = false;
        if (shape == 0) s.params_route = EZPZ_PARAMS_ROUTE_FRONTS, want = EZPZ_SWEEP_FRONTS;
        else if (shape == 1) s.comp = std::make_unique<CompPlan>(), s.comp->interpretable = true, want = EZPZ_SWEEP_INTERPRETER;
        else if (shape == 2) s.mode = MODE_SUB, s.grid_wgs = 1 + below(2), want = EZPZ_SWEEP_SUB_WAVEFRONT_TEAMS;
        else if (shape == 3) s.mode = MODE_PART, want = EZPZ_SWEEP_PARTITIONED_WORKGROUP;
        else if (shape == 4) s.mode = MODE_WGB, want = EZPZ_SWEEP_BARRIER_WORKGROUP;
        else if (shape == 5) s.mode = MODE_WGB, s.rec = true, want = EZPZ_SWEEP_RECORD_WALK;
        else s.mode = MODE_WGB, s.grid_wgs = 2 + below(3), decline = true;
        const int rc = driven_request(&s, pos.empty() ? nullptr : pos.data(), pos.size(), r);
        if (decline ? rc != EZPZ_ERR_INVALID_ARGUMENT : rc != EZPZ_OK) return fail("a request's verdict", trial);
        if (!decline && (r.sweep_route != want || r.for_comp != (shape == 1) || r.params_route != s.params_route || r.slot_of_pos.size() != map.size()))
            return fail("a request's routes", trial);
        ++requests;
    }
    std::printf("lists %zu mapped, %zu declined, requests %zu resolved: all as expected\n", lists, declined, requests);
    return 0;
}
