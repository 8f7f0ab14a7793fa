// The pass decision of the exact search (auncel_amd/csrc/exact_args.h: exact_pass_kind) and the wide pass's host helpers, as a program
// of its own: built plain and under the address and undefined-behaviour sanitizers by tests/test_exact_wide_cpu.py.
//   - for d in 1 .. 128 the decision equals the rule exact_slice had before the wide pass existed, written out below, for every
//     combination of the flags: option "exact_wide" changes nothing there
//   - beyond, it is 3 exactly when 128 < d <= 1024, both options are set, the shape and float conditions hold and byte codes are not
//     in use, and 0 otherwise (d = 1025, either option off, byte-coded lists)
//   - exact_wide_stages / exact_wide_slab / exact_wide_chunk_blocks / exact_wide_wave_block against brute-force loops
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../auncel_amd/csrc/exact_args.h"

using namespace amdivf;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (failures++ < 20) {            \
                printf("FAIL %s: ", #cond);   \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

// exact_slice before the wide pass: shape_ok held `d <= 128`; pass = shape_ok && bytes; pass16 = !pass && shape_ok &&
// filter_available && option exact_float (ensure_frag16 and the queries' scale come after, as they still do)
static int rule_before(int d, bool shape, bool bytes, bool float_ok, bool opt_float) {
    const bool shape_ok = shape && d <= 128;
    const bool pass = shape_ok && bytes;
    const bool pass16 = !pass && shape_ok && float_ok && opt_float;
    return pass ? 1 : pass16 ? 2 : 0;
}

int main() {
    long cases = 0, threes = 0;
    for (int d = 1; d <= 1100; d++)
        for (int f = 0; f < 32; f++) {
            const bool shape = f & 1, bytes = f & 2, float_ok = f & 4, opt_float = f & 8, opt_wide = f & 16;
            const int got = exact_pass_kind(d, shape, bytes, float_ok, opt_float, opt_wide);
            cases++;
            if (d <= 128) {
                CHECK(got == rule_before(d, shape, bytes, float_ok, opt_float), "d %d flags %d: %d", d, f, got);
                CHECK(got == exact_pass_kind(d, shape, bytes, float_ok, opt_float, !opt_wide), "d %d flags %d: exact_wide matters", d, f);
                CHECK(got != 3, "d %d flags %d", d, f);
            } else {
                const bool want3 = d <= 1024 && shape && !bytes && float_ok && opt_float && opt_wide;
                CHECK(got == (want3 ? 3 : 0), "d %d flags %d: %d", d, f, got);
                threes += got == 3;
            }
        }
    CHECK(threes == 1024 - 128, "served (d, flags) beyond 128 dimensions: %ld", threes);
    CHECK(exact_pass_kind(1024, true, false, true, true, true) == 3, "d 1024");
    CHECK(exact_pass_kind(1025, true, false, true, true, true) == 0, "d 1025");
    CHECK(exact_pass_kind(129, true, false, true, true, true) == 3, "d 129");
    CHECK(exact_pass_kind(200, true, false, true, false, true) == 0, "exact_float off");
    CHECK(exact_pass_kind(200, true, false, true, true, false) == 0, "exact_wide off");
    CHECK(exact_pass_kind(200, true, true, true, true, true) == 0, "byte codes in use");
    CHECK(exact_pass_kind(128, true, true, false, false, true) == 1, "bytes at 128");

    // stages of J pieces at sp a stage
    for (int sp = 2; sp <= 10; sp += 2)
        for (int J = 1; J <= 64; J++) {
            int s = 0;
            while (s * sp < J) s++;
            CHECK(exact_wide_stages(J, sp) == s, "J %d sp %d", J, sp);
        }
    // the slab: the next multiple of four
    for (uint32_t slab = 2; slab <= 4096; slab += 2) {
        uint32_t w = slab;
        while (w % 4) w++;
        CHECK(exact_wide_slab(slab) == w, "slab %u", slab);
    }
    // chunks of a slab [B0, B1): every block of the slab is computed exactly once by the wave that owns it, a wave without a block
    // recomputes the chunk's first (an existing one), and a chunk has 4 blocks or, as the stream's last, 2
    for (uint64_t nblk = 2; nblk <= 66; nblk += 2)
        for (uint32_t slab = 4; slab <= 24; slab += 4)
            for (uint64_t B0 = 0; B0 < nblk; B0 += slab) {
                const uint64_t B1 = B0 + slab < nblk ? B0 + slab : nblk;
                std::vector<int> seen(nblk, 0);
                for (uint64_t c = B0; c < B1; c += EXACT_WIDE_CHUNK) {
                    uint32_t have = 0;
                    for (uint64_t b = c; b < B1 && b < c + 4; b++) have++;
                    CHECK(exact_wide_chunk_blocks(c, B1) == have, "chunk %llu of [%llu, %llu)", (unsigned long long)c, (unsigned long long)B0, (unsigned long long)B1);
                    CHECK(have == 4 || (have == 2 && B1 == nblk && nblk % 4 == 2), "chunk of %u blocks", have);
                    for (uint32_t w = 0; w < 4; w++) {
                        const uint64_t b = exact_wide_wave_block(c, B1, w);
                        CHECK(b < B1 && b >= c, "block %llu outside the chunk", (unsigned long long)b);
                        if (w < have) {
                            CHECK(b == c + w, "wave %u", w);
                            seen[b]++;
                        } else {
                            CHECK(b == c, "idle wave %u", w);
                        }
                    }
                }
                for (uint64_t b = 0; b < nblk; b++) CHECK(seen[b] == (b >= B0 && b < B1 ? 1 : 0), "block %llu seen %d times", (unsigned long long)b, seen[b]);
            }
    printf("decisions %ld, served beyond 128 dimensions %ld, failures %d\n", cases, threes, failures);
    if (failures) return 1;
    printf("DONE\n");
    return 0;
}
