// The host-only part of the exact search under an id selector (auncel_amd/csrc/exact_args.h: the mask of a block's live slots that
// the keep-aware block table writes and the list pass reads, the seed's nprobe under a selector, and the argument checks of
// amd_ivf_search_exact_selected / _resident_selected) as a program of its own, for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/exact_selected_main.cpp -o exact_selected_main
// Prints DONE and returns 0 when every check held.
#include <cstdio>
#include <random>

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

// the rule bit by bit: slot m is live iff it holds an entry and the selector keeps it
static uint32_t mask_by_bits(uint64_t left, uint32_t keep_half) {
    uint32_t r = 0;
    for (uint32_t m = 0; m < 32; m++)
        if ((uint64_t)m < left && ((keep_half >> m) & 1u)) r |= (uint32_t)1 << m;
    return r;
}

int main() {
    std::mt19937 rng(12345);
    // ---- the valid mask: every `left` at which the rule changes form, keep halves of nothing, everything and random patterns
    for (uint64_t left : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)31, (uint64_t)32, (uint64_t)33, (uint64_t)40, (uint64_t)64,
                          (uint64_t)0xffffffffull, (uint64_t)1 << 40}) {
        CHECK(exact_block_valid_mask(left, 0u) == 0u);
        CHECK(exact_block_valid_mask(left, 0xffffffffu) == mask_by_bits(left, 0xffffffffu));
        CHECK(exact_block_valid_mask(left, 0x80000000u) == mask_by_bits(left, 0x80000000u));
        CHECK(exact_block_valid_mask(left, 1u) == mask_by_bits(left, 1u));
        for (int i = 0; i < 200; i++) {
            const uint32_t half = (uint32_t)rng();
            CHECK(exact_block_valid_mask(left, half) == mask_by_bits(left, half));
        }
    }
    CHECK(exact_block_valid_mask(0, 0xffffffffu) == 0u);            // the padding block behind a list: nothing, whatever the bits say
    CHECK(exact_block_valid_mask(1, 0xffffffffu) == 1u);
    CHECK(exact_block_valid_mask(31, 0xffffffffu) == 0x7fffffffu);  // bits past the list's end are not trusted to be zero
    CHECK(exact_block_valid_mask(32, 0xffffffffu) == 0xffffffffu);
    CHECK(exact_block_valid_mask(40, 0xdeadbeefu) == 0xdeadbeefu);
    // ---- the half of a keep word that belongs to a block: even blocks the low half, odd blocks the high one
    CHECK(exact_block_keep_half(0x1122334455667788ull, 0) == 0x55667788u);
    CHECK(exact_block_keep_half(0x1122334455667788ull, 1) == 0x11223344u);
    CHECK(exact_block_keep_half(0x1122334455667788ull, 6) == 0x55667788u);
    CHECK(exact_block_keep_half(0x1122334455667788ull, ((uint64_t)1 << 40) + 1) == 0x11223344u);
    for (int i = 0; i < 200; i++) {  // a list of `size` entries under a random selector, block by block: the members and nothing else
        const uint64_t size = rng() % 200;
        const uint64_t blocks = ((size + 31) / 32 + 1) & ~(uint64_t)1;
        uint64_t members = 0, live = 0;
        for (uint64_t b = 0; b < blocks; b++) {
            const uint64_t word = ((uint64_t)rng() << 32) | rng();  // (bits past the end set at random)
            const uint64_t p = b * 32, left = p < size ? size - p : 0;
            const uint32_t half = exact_block_keep_half(word, b);
            for (uint32_t m = 0; m < 32; m++) members += p + m < size && ((word >> (32 * (b & 1) + m)) & 1);
            live += (uint64_t)__builtin_popcount(exact_block_valid_mask(left, half));
        }
        CHECK(members == live);
    }
    // ---- the seed's nprobe: ceil(seed x ntotal / kept); no members, a product past 64 bits: the largest value
    CHECK(exact_selected_seed(16, 1000, 1000) == 16);
    CHECK(exact_selected_seed(16, 1000, 500) == 32);
    CHECK(exact_selected_seed(16, 1000, 501) == 32);
    CHECK(exact_selected_seed(16, 1000, 499) == 33);
    CHECK(exact_selected_seed(16, 1000, 10) == 1600);
    CHECK(exact_selected_seed(1, 7, 3) == 3);
    CHECK(exact_selected_seed(16, 1000, 1) == 16000);
    CHECK(exact_selected_seed(16, 1000, 0) == UINT64_MAX);
    CHECK(exact_selected_seed(16, 0, 0) == UINT64_MAX);
    CHECK(exact_selected_seed(0, 1000, 10) == 0);
    CHECK(exact_selected_seed(UINT64_MAX, 3, 2) == UINT64_MAX);
    CHECK(exact_selected_seed((uint64_t)1 << 32, (uint64_t)1 << 32, 1) == UINT64_MAX);
    CHECK(exact_selected_seed((uint64_t)1 << 31, (uint64_t)1 << 32, (uint64_t)1 << 32) == (uint64_t)1 << 31);
    for (int i = 0; i < 1000; i++) {  // never fewer lists than the unfiltered seed; the members of that many lists reach the seed's entries
        const uint64_t seed = 1 + rng() % 64, ntotal = 1 + rng() % 100000, kept = 1 + rng() % ntotal;
        const uint64_t s = exact_selected_seed(seed, ntotal, kept);
        CHECK(s >= seed);
        CHECK(s * kept >= seed * ntotal && (s - 1) * kept < seed * ntotal);
    }
    // ---- the argument checks: everything exact_args_error refuses, and a missing selector
    float D[4];
    int64_t I[4];
    CHECK(exact_selected_args_error(true, true, true, 0, 2, 2, D, I).empty());
    CHECK(exact_selected_args_error(true, true, true, 0, 0, 2, nullptr, nullptr).empty());
    CHECK(exact_selected_args_error(true, false, true, 0, 2, 2, D, I).find("null selector") != std::string::npos);
    CHECK(exact_selected_args_error(true, false, true, 0, 0, 2, nullptr, nullptr).find("null selector") != std::string::npos);  // (even without queries)
    CHECK(exact_selected_args_error(false, true, true, 0, 2, 2, D, I).find("null handle") != std::string::npos);
    CHECK(exact_selected_args_error(false, false, true, 0, 2, 2, D, I).find("null handle") != std::string::npos);
    CHECK(exact_selected_args_error(true, true, false, 0, 2, 2, D, I).find("null") != std::string::npos);
    CHECK(exact_selected_args_error(true, true, true, 0, 2, 2, nullptr, I).find("null") != std::string::npos);
    CHECK(exact_selected_args_error(true, true, true, 0, 2, 2, D, nullptr).find("null") != std::string::npos);
    CHECK(exact_selected_args_error(true, true, true, 0, 2, 0, D, I).find("k must be positive") != std::string::npos);
    CHECK(exact_selected_args_error(true, true, true, SIZE_MAX - 1, 5, 2, D, I).find("range") != std::string::npos);
    CHECK(exact_selected_args_error(true, true, true, SIZE_MAX - 5, 5, 2, D, I).empty());
    CHECK(exact_selected_args_error(true, false, true, 0, 2, 2, D, I).rfind("exact search: ", 0) == 0);
    if (failures) return 1;
    printf("DONE\n");
    return 0;
}
