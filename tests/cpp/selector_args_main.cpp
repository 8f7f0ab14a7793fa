// The host-only part of a selector (auncel_amd/csrc/selector_args.h: argument checks, the per-list runs of a SLICE, the sorted ids of
// an ID_BATCH) as a program of its own, for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/selector_args_main.cpp -o selector_args_main
// Prints DONE and returns 0 when every check held.
#include <cstdio>
#include <cstdlib>
#include <numeric>

#include "../../auncel_amd/csrc/selector_args.h"

using namespace amdivf;

static int failures = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                         \
        }                                                       \
    } while (0)

int main() {
    const uint64_t nt = 3000;
    const uint64_t some[2] = {1, 2};
    // ---- the argument checks: what amd_ivf_subset and amd_ivf_selector_create refuse
    for (int type : {-1, 3, 4, 7, 100}) CHECK(!selector_args_error("x", type, 0, 0, nullptr, 0, nt).empty());
    CHECK(selector_args_error("x", SUBSET_ID_RANGE, 5, 2, nullptr, 0, nt).empty());  // (an empty range is valid)
    CHECK(selector_args_error("x", SUBSET_ID_RANGE, INT64_MIN, INT64_MAX, nullptr, 0, nt).empty());
    CHECK(selector_args_error("x", SUBSET_ID_MOD, 3, 1, nullptr, 0, nt).empty());
    CHECK(!selector_args_error("x", SUBSET_ID_MOD, 0, 0, nullptr, 0, nt).empty());
    CHECK(!selector_args_error("x", SUBSET_ID_MOD, -3, 0, nullptr, 0, nt).empty());
    CHECK(!selector_args_error("x", SUBSET_ID_MOD, INT64_MIN, 0, nullptr, 0, nt).empty());
    CHECK(selector_args_error("x", SUBSET_SLICE, 0, (int64_t)nt, nullptr, 0, nt).empty());
    CHECK(selector_args_error("x", SUBSET_SLICE, 5, 5, nullptr, 0, nt).empty());
    CHECK(selector_args_error("x", SUBSET_SLICE, 0, 0, nullptr, 0, 0).empty());
    CHECK(!selector_args_error("x", SUBSET_SLICE, 10, 5, nullptr, 0, nt).empty());
    CHECK(!selector_args_error("x", SUBSET_SLICE, -1, 5, nullptr, 0, nt).empty());
    CHECK(!selector_args_error("x", SUBSET_SLICE, 0, (int64_t)nt + 1, nullptr, 0, nt).empty());
    CHECK(!selector_args_error("x", SUBSET_SLICE, INT64_MIN, INT64_MAX, nullptr, 0, nt).empty());
    for (int type : {SUBSET_ID_BITS, SUBSET_ID_BATCH}) {
        CHECK(selector_args_error("x", type, 0, 0, nullptr, 0, nt).empty());
        CHECK(selector_args_error("x", type, 0, 0, some, 2, nt).empty());
        CHECK(!selector_args_error("x", type, 0, 0, nullptr, 4, nt).empty());
    }
    CHECK(selector_args_error("subset", 9, 0, 0, nullptr, 0, nt).rfind("subset: ", 0) == 0);
    CHECK(selector_args_error("selector", SUBSET_ID_BITS, 0, 0, nullptr, 1, nt).find("null") != std::string::npos);

    // ---- SLICE: the runs are IndexIVF::copy_subset_to's, their ends lie inside their lists and they add up to a2 - a1
    srand(7);
    for (int trial = 0; trial < 200; trial++) {
        const size_t nlist = 1 + (size_t)(rand() % 40);
        std::vector<uint64_t> off(nlist + 1, 0);
        for (size_t l = 0; l < nlist; l++) off[l + 1] = off[l] + (rand() % 4 == 0 ? 0 : (uint64_t)(rand() % 300));
        const uint64_t total = off[nlist];
        const int64_t a1 = total ? (int64_t)((uint64_t)rand() % (total + 1)) : 0;
        const int64_t a2 = total ? a1 + (int64_t)((uint64_t)rand() % (total - (uint64_t)a1 + 1)) : 0;
        CHECK(selector_args_error("x", SUBSET_SLICE, a1, a2, nullptr, 0, total).empty());
        const std::vector<uint64_t> runs = selector_slice_runs(off.data(), nlist, a1, a2);
        CHECK(runs.size() == 2 * nlist);
        int64_t kept = 0;  // (a list's run may be empty the "wrong" way round, begin > end, as in the reference: the sum telescopes)
        for (size_t l = 0; l < nlist; l++) {
            CHECK(runs[2 * l] <= off[l + 1] - off[l] && runs[2 * l + 1] <= off[l + 1] - off[l]);
            kept += (int64_t)runs[2 * l + 1] - (int64_t)runs[2 * l];
        }
        CHECK(kept == a2 - a1);
    }
    {  // lists whose running count is beyond 2^32 entries: the products stay inside 64 bits for the sizes an index can hold
        const uint64_t off[3] = {0, 5000000000ull, 9000000000ull};
        const std::vector<uint64_t> runs = selector_slice_runs(off, 2, 1000000000ll, 2000000000ll);
        CHECK(runs[1] - runs[0] + runs[3] - runs[2] == 1000000000ull);
    }
    {  // no entries at all: no division by the total
        const uint64_t off[4] = {0, 0, 0, 0};
        const std::vector<uint64_t> runs = selector_slice_runs(off, 3, 0, 0);
        CHECK(std::accumulate(runs.begin(), runs.end(), (uint64_t)0) == 0);
    }

    // ---- ID_BATCH: ascending, each id once, whatever the caller's order; nothing read when there is nothing
    CHECK(selector_batch(nullptr, 0).empty());
    for (int trial = 0; trial < 200; trial++) {
        const size_t n = (size_t)(rand() % 500);
        std::vector<int64_t> ids(n);
        for (auto& v : ids) v = (int64_t)(rand() % 200) - 50 + (rand() % 50 == 0 ? INT64_MAX - 300 : 0);
        const std::vector<int64_t> b = selector_batch(ids.data(), n);
        CHECK(b.size() <= n);
        for (size_t i = 1; i < b.size(); i++) CHECK(b[i - 1] < b[i]);
        for (int64_t v : ids) CHECK(std::binary_search(b.begin(), b.end(), v));
    }
    const int64_t edge[5] = {INT64_MAX, INT64_MIN, 0, INT64_MIN, INT64_MAX};
    CHECK(selector_batch(edge, 5) == (std::vector<int64_t>{INT64_MIN, 0, INT64_MAX}));
    if (failures) return 1;
    printf("DONE\n");
    return 0;
}
