// The host-only part of amd_ivf_selector_combine (auncel_amd/csrc/selector_args.h: the operand checks, the word rule of an op, and
// selector_valid_word -- the bits of a keep word that stand for entries, the same definition the combine kernel reads) as a program of
// its own, for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/selector_combine_main.cpp -o selector_combine_main
// Prints DONE and returns 0 when every check held.
#include <cstdio>
#include <cstdlib>

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

// the words a list of n entries owns: its 32-entry block count rounded up to even, halved (ivf_kernels.h: mfma_list_blocks)
static uint64_t list_words(uint64_t n) {
    const uint64_t blocks = ((n + 63) / 64) * 2;
    return blocks / 2;
}

// a list of n entries in `words` words (>= list_words(n): the rest is padding): the rule against one bit at a time
static void check_list(uint64_t n, uint64_t words) {
    uint64_t total = 0;
    for (uint64_t j = 0; j < words; j++) {
        const uint64_t v = selector_valid_word(n, j);
        for (int b = 0; b < 64; b++) CHECK(((v >> b) & 1) == (j * 64 + (uint64_t)b < n ? 1u : 0u));
        total += (uint64_t)__builtin_popcountll(v);
        // NOT of a word with no bit set keeps exactly the entries; NOT of the full word keeps nothing, padding included
        CHECK((selector_combine_word(SELECTOR_NOT, 0, 0) & v) == v);
        CHECK((selector_combine_word(SELECTOR_NOT, v, 0) & v) == 0);
    }
    CHECK(total == n);
}

int main() {
    // ---- selector_valid_word: the lengths around a word's end, and one list whose 32-entry block count is odd (n = 70: three blocks)
    for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 127ull, 128ull, 70ull}) {
        check_list(n, list_words(n));
        check_list(n, list_words(n) + 3);  // (padding words behind the list: nothing of them is an entry)
    }
    CHECK((70 + 31) / 32 % 2 == 1);
    CHECK(selector_valid_word(0, 0) == 0);
    CHECK(selector_valid_word(1, 0) == 1);
    CHECK(selector_valid_word(63, 0) == ~0ull >> 1);
    CHECK(selector_valid_word(64, 0) == ~0ull && selector_valid_word(64, 1) == 0);
    CHECK(selector_valid_word(65, 0) == ~0ull && selector_valid_word(65, 1) == 1);
    CHECK(selector_valid_word(127, 1) == ~0ull >> 1);
    CHECK(selector_valid_word(128, 1) == ~0ull && selector_valid_word(128, 2) == 0);
    CHECK(selector_valid_word(70, 1) == 63 && selector_valid_word(70, 2) == 0);
    // the largest list a selector takes (2^32 - 1 entries), and word numbers whose first entry does not fit 64 bits
    CHECK(selector_valid_word(0xffffffffull, 0x3ffffffull) == ~0ull >> 1 && selector_valid_word(0xffffffffull, 0x4000000ull) == 0);
    CHECK(selector_valid_word(~0ull, ~0ull) == 0 && selector_valid_word(~0ull, 1ull << 58) == 0);
    CHECK(selector_valid_word(~0ull, (1ull << 58) - 1) == ~0ull >> 1);
    srand(11);
    for (int trial = 0; trial < 300; trial++) {
        const uint64_t n = (uint64_t)(rand() % 1000);
        check_list(n, list_words(n) + (uint64_t)(rand() % 3));
    }

    // ---- the word rule of every op
    const uint64_t a = 0xf0f0f0f0f0f0f0f0ull, b = 0xff00ff00ff00ff00ull;
    CHECK(selector_combine_word(SELECTOR_AND, a, b) == (a & b));
    CHECK(selector_combine_word(SELECTOR_OR, a, b) == (a | b));
    CHECK(selector_combine_word(SELECTOR_ANDNOT, a, b) == (a & ~b));
    CHECK(selector_combine_word(SELECTOR_ANDNOT, b, a) == (b & ~a));
    CHECK(selector_combine_word(SELECTOR_NOT, a, b) == ~a);

    // ---- the operand checks, in the order the refusals are documented
    int index1 = 0, index2 = 0;
    const SelectorOperand x{&index1, 5}, y{&index1, 5}, other{&index2, 5}, old{&index1, 4};
    for (int op : {SELECTOR_AND, SELECTOR_OR, SELECTOR_ANDNOT}) {
        CHECK(selector_combine_error(op, &x, &y, true, 5, false).empty());
        CHECK(selector_combine_error(op, &x, &x, true, 5, false).empty());  // (a selector with itself)
        CHECK(selector_combine_error(op, &x, nullptr, true, 5, false).find("two operands") != std::string::npos);
        CHECK(selector_combine_error(op, &x, &other, true, 5, false).find("different indexes") != std::string::npos);
        CHECK(selector_combine_error(op, &old, &y, true, 5, false).find("stale") != std::string::npos);
        CHECK(selector_combine_error(op, &x, &old, true, 5, false).find("stale") != std::string::npos);
        CHECK(selector_combine_error(op, &x, &y, true, 6, false).find("stale") != std::string::npos);
        CHECK(selector_combine_error(op, &x, &y, true, 5, true).find("tickets") != std::string::npos);
        CHECK(selector_combine_error(op, nullptr, &y, true, 5, false).find("null") != std::string::npos);
        CHECK(selector_combine_error(op, &x, &y, false, 5, false).find("null") != std::string::npos);
    }
    CHECK(selector_combine_error(SELECTOR_NOT, &x, nullptr, true, 5, false).empty());
    CHECK(selector_combine_error(SELECTOR_NOT, &x, &y, true, 5, false).find("one operand") != std::string::npos);
    CHECK(selector_combine_error(SELECTOR_NOT, &old, nullptr, true, 5, false).find("stale") != std::string::npos);
    CHECK(selector_combine_error(SELECTOR_NOT, &x, nullptr, true, 5, true).find("tickets") != std::string::npos);
    CHECK(selector_combine_error(SELECTOR_NOT, nullptr, nullptr, true, 5, false).find("null") != std::string::npos);
    CHECK(selector_combine_error(SELECTOR_NOT, nullptr, nullptr, false, 5, false).find("null") != std::string::npos);
    for (int op : {-1, 4, 100}) {
        CHECK(selector_combine_error(op, &x, &y, true, 5, false).find("unknown op") != std::string::npos);
        CHECK(selector_combine_error(op, &x, nullptr, true, 5, false).find("unknown op") != std::string::npos);
        CHECK(selector_combine_error(op, nullptr, nullptr, true, 5, false).find("null") != std::string::npos);  // (null comes first)
    }
    if (failures) return 1;
    printf("DONE\n");
    return 0;
}
