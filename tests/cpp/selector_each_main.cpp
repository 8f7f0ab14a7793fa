// The host-only part of a search under a selector per query (amd_ivf_search_selected_each and its siblings; auncel_amd/csrc/selector_args.h:
// selector_each_null_error, selector_each_error, selector_each_range_error -- what the entry points refuse before anything reaches the
// device) as a program of its own, for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/selector_each_main.cpp -o selector_each_main
// Prints DONE and returns 0 when every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

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

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

int main() {
    const char* W = "search_selected_each";
    // ---- what the caller passed at all: h, sels, sel_of, x, D, I
    CHECK(selector_each_null_error(W, true, true, true, true, true, true, 3, 10).empty());
    for (int missing = 0; missing < 6; missing++) {
        if (missing == 3) continue;  // (x: its own message, below)
        const std::string e = selector_each_null_error(W, missing != 0, missing != 1, missing != 2, true, missing != 4, missing != 5, 3, 10);
        CHECK(has(e, "null argument") && e.rfind(W, 0) == 0);
        // ... whatever n and nsel are: nothing is searched, the pointers are still wanted
        CHECK(has(selector_each_null_error(W, missing != 0, missing != 1, missing != 2, true, missing != 4, missing != 5, 0, 0), "null argument"));
    }
    CHECK(has(selector_each_null_error(W, true, true, true, false, true, true, 3, 10), "null queries"));
    CHECK(selector_each_null_error(W, true, true, true, false, true, true, 3, 0).empty());  // (no queries: x is not read)
    CHECK(has(selector_each_null_error(W, true, true, true, true, true, true, 0, 10), "nsel == 0"));
    CHECK(selector_each_null_error(W, true, true, true, true, true, true, 0, 0).empty());
    CHECK(has(selector_each_null_error(W, false, true, true, false, true, true, 0, 10), "null argument"));  // (null comes first)

    // ---- the table and the indexes
    int index1 = 0, index2 = 0;
    const SelectorOperand good{&index1, 5}, other{&index2, 5}, old{&index1, 4}, null{nullptr, 0};
    const std::vector<uint32_t> sel_of = {0, 2, 1, 1, 0, 2, 2, 0};
    {
        const std::vector<SelectorOperand> t = {good, good, good};  // (the same selector more than once is fine)
        CHECK(selector_each_error(W, t.data(), 3, sel_of.data(), sel_of.size(), &index1, 5).empty());
        CHECK(selector_each_error(W, t.data(), 3, sel_of.data(), 0, &index1, 5).empty());
        // a selector that no query uses is checked like the others; none is needed at all without queries
        const std::vector<uint32_t> zeros(8, 0);
        CHECK(selector_each_error(W, t.data(), 3, zeros.data(), zeros.size(), &index1, 5).empty());
        CHECK(selector_each_error(W, nullptr, 0, nullptr, 0, &index1, 5).empty());
        CHECK(has(selector_each_error(W, t.data(), 3, sel_of.data(), sel_of.size(), &index1, 6), "selector 0 of the table is stale"));
        CHECK(has(selector_each_error(W, t.data(), 3, sel_of.data(), sel_of.size(), &index2, 5), "selector 0 of the table was made on another index"));
    }
    for (size_t at = 0; at < 3; at++) {
        std::vector<SelectorOperand> t = {good, good, good};
        const std::string where = "selector " + std::to_string(at) + " of the table";
        t[at] = null;
        std::string e = selector_each_error(W, t.data(), 3, sel_of.data(), sel_of.size(), &index1, 5);
        CHECK(has(e, where.c_str()) && has(e, "is null"));
        t[at] = other;
        e = selector_each_error(W, t.data(), 3, sel_of.data(), sel_of.size(), &index1, 5);
        CHECK(has(e, where.c_str()) && has(e, "another index"));
        t[at] = old;
        e = selector_each_error(W, t.data(), 3, sel_of.data(), sel_of.size(), &index1, 5);
        CHECK(has(e, where.c_str()) && has(e, "stale"));
        // ... also where no query names it
        const std::vector<uint32_t> away(8, (uint32_t)((at + 1) % 3));
        CHECK(has(selector_each_error(W, t.data(), 3, away.data(), away.size(), &index1, 5), "stale"));
    }
    {
        const std::vector<SelectorOperand> t = {good, good, good};
        for (size_t at : {(size_t)0, (size_t)3, sel_of.size() - 1})
            for (uint32_t bad : {3u, 4u, 0xffffffffu}) {
                std::vector<uint32_t> s = sel_of;
                s[at] = bad;
                const std::string e = selector_each_error(W, t.data(), 3, s.data(), s.size(), &index1, 5);
                const std::string where = "sel_of[" + std::to_string(at) + "] = " + std::to_string(bad);
                CHECK(has(e, where.c_str()) && has(e, "nsel = 3"));
                // the first bad one is named
                s.back() = 99;
                CHECK(has(selector_each_error(W, t.data(), 3, s.data(), s.size(), &index1, 5), where.c_str()) || at == sel_of.size() - 1);
            }
        // the table is checked before the indexes
        std::vector<SelectorOperand> t2 = t;
        t2[1] = old;
        std::vector<uint32_t> s = sel_of;
        s[0] = 7;
        CHECK(has(selector_each_error(W, t2.data(), 3, s.data(), s.size(), &index1, 5), "stale"));
    }

    // ---- resident ranges
    const size_t top = ~(size_t)0;
    CHECK(selector_each_range_error(W, 0, 0, 0).empty());
    CHECK(selector_each_range_error(W, 0, 100, 100).empty());
    CHECK(selector_each_range_error(W, 100, 0, 100).empty());
    CHECK(has(selector_each_range_error(W, 1, 100, 100), "out of bounds"));
    CHECK(has(selector_each_range_error(W, 101, 0, 100), "out of bounds"));
    CHECK(has(selector_each_range_error(W, top, 1, 100), "wraps"));
    CHECK(has(selector_each_range_error(W, top, 2, 100), "wraps"));
    CHECK(has(selector_each_range_error(W, 5, top - 3, 100), "wraps"));
    CHECK(has(selector_each_range_error(W, top - 3, 3, 100), "out of bounds"));  // (start + n == SIZE_MAX: no wrap)
    if (failures) return 1;
    printf("DONE\n");
    return 0;
}
