// The host-only part of the exact search (auncel_amd/csrc/exact_args.h: the argument checks and the tie rule over a query's sorted
// candidates) as a program of its own, for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/exact_args_main.cpp -o exact_args_main
// Prints DONE and returns 0 when every check held.
#include <cstdio>
#include <vector>

#include "../../auncel_amd/csrc/exact_args.h"

using namespace amdivf;

static int failures = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                         \
        }                                                       \
    } while (0)

// `count` candidates with pairwise different distances 10, 20, 30, ... at positions 1000 - i (the position never decides a tie)
static std::vector<uint64_t> distinct(size_t count) {
    std::vector<uint64_t> v(count);
    for (size_t i = 0; i < count; i++) v[i] = exact_key((uint32_t)(10 * (i + 1)), (uint32_t)(1000 - i));
    return v;
}
// ... with entry at + 1 given the distance of entry `at` (positions stay different, the order ascending)
static std::vector<uint64_t> tied_at(size_t count, size_t at) {
    std::vector<uint64_t> v = distinct(count);
    v[at + 1] = exact_key((uint32_t)(v[at] >> 32), (uint32_t)v[at] + 1);
    return v;
}
// the rule as a wave reads it: lane l looks at pairs l, l + 64, ...
static bool by_lanes(const std::vector<uint64_t>& v, size_t count, size_t k) {
    bool t = false;
    for (size_t lane = 0; lane < 64; lane++) t |= exact_window_tied(v.data(), count, k, lane, 64);
    return t;
}

int main() {
    // ---- the tie rule.  A tie AT position p means entries p and p + 1 are equal; the window is the best min(count, k + 1)
    for (size_t k : {2, 3, 10, 64, 65, 100, 130}) {
        const size_t count = k + 40;
        CHECK(!exact_window_tied(distinct(count).data(), count, k));
        CHECK(!by_lanes(distinct(count), count, k));
        for (size_t p : {(size_t)0, k - 2, k - 1}) {  // inside the k best, and between the k-th and the (k + 1)-th
            CHECK(exact_window_tied(tied_at(count, p).data(), count, k));
            CHECK(by_lanes(tied_at(count, p), count, k));
        }
        // a tie at k: the (k + 1)-th equals the (k + 2)-th -- outside the window, the result is decided
        CHECK(!exact_window_tied(tied_at(count, k).data(), count, k));
        CHECK(!by_lanes(tied_at(count, k), count, k));
        // exactly k + 1 entries: the pair (k - 1, k) is the last one looked at
        CHECK(exact_window_tied(tied_at(k + 1, k - 1).data(), k + 1, k));
        CHECK(!exact_window_tied(distinct(k + 1).data(), k + 1, k));
        // exactly k entries (fewer than k + 1): the (k + 1)-th lies beyond the threshold; only the k there are can tie
        CHECK(!exact_window_tied(distinct(k).data(), k, k));
        CHECK(exact_window_tied(tied_at(k, k - 2).data(), k, k));
        CHECK(by_lanes(tied_at(k, k - 2), k, k));
        CHECK(exact_window_tied(tied_at(k, 0).data(), k, k));
        // fewer than k entries never reach the rule in the engine; it still reads nothing past `count`
        std::vector<uint64_t> few = distinct(k - 1);
        few.shrink_to_fit();
        CHECK(!exact_window_tied(few.data(), k - 1, k));
    }
    {  // k = 1: the window is the best two
        CHECK(!exact_window_tied(distinct(5).data(), 5, 1));
        CHECK(exact_window_tied(tied_at(5, 0).data(), 5, 1));
        CHECK(!exact_window_tied(tied_at(5, 1).data(), 5, 1));
        CHECK(!exact_window_tied(distinct(1).data(), 1, 1));  // one candidate: nothing to compare
        CHECK(!exact_window_tied(nullptr, 0, 1));
        CHECK(!by_lanes(distinct(1), 1, 1));
    }
    {  // equal positions' worth: the key orders by distance first, the position only breaks the sort's ties
        CHECK(exact_key(1, 0xffffffffu) < exact_key(2, 0));
        CHECK(exact_key(7, 3) < exact_key(7, 4));
        CHECK((exact_key(0xffffffffu, 0xffffffffu) >> 32) == 0xffffffffu);
    }
    // ---- the argument checks: what amd_ivf_search_exact / _resident refuse before the device is touched
    float D[4];
    int64_t I[4];
    CHECK(exact_args_error(true, true, 0, 2, 2, D, I).empty());
    CHECK(exact_args_error(true, true, 0, 0, 2, nullptr, nullptr).empty());  // (no queries: nothing is read or written)
    CHECK(exact_args_error(true, false, 0, 0, 2, nullptr, nullptr).empty());
    CHECK(exact_args_error(false, true, 0, 2, 2, D, I).find("null") != std::string::npos);
    CHECK(exact_args_error(true, false, 0, 2, 2, D, I).find("null") != std::string::npos);
    CHECK(exact_args_error(true, true, 0, 2, 2, nullptr, I).find("null") != std::string::npos);
    CHECK(exact_args_error(true, true, 0, 2, 2, D, nullptr).find("null") != std::string::npos);
    CHECK(exact_args_error(true, true, 0, 2, 0, D, I).find("k must be positive") != std::string::npos);
    CHECK(exact_args_error(true, true, 0, 0, 0, D, I).find("k must be positive") != std::string::npos);
    CHECK(exact_args_error(true, true, SIZE_MAX - 1, 5, 2, D, I).find("range") != std::string::npos);  // start + n wraps round
    CHECK(exact_args_error(true, true, SIZE_MAX, 1, 2, D, I).find("range") != std::string::npos);
    CHECK(exact_args_error(true, true, SIZE_MAX - 5, 5, 2, D, I).empty());
    CHECK(exact_args_error(false, true, 0, 2, 2, D, I).rfind("exact search: ", 0) == 0);
    if (failures) return 1;
    printf("DONE\n");
    return 0;
}
