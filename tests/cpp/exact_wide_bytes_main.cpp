// The pass decision with the byte pass beyond 128 dimensions (auncel_amd/csrc/exact_args.h: exact_pass_kind_bytes), as a program of its
// own: built plain and under the address and undefined-behaviour sanitizers by tests/test_exact_wide_bytes_cpu.py.  For every d in
// 1 .. 1100 and all 64 combinations of the flags:
//   - with option "exact_wide_bytes" off the decision is exact_pass_kind's
//   - it is 4 exactly when the shape holds, the call runs on byte codes, 128 < d <= 1024 and the option is set -- whatever the other
//     three flags say
//   - an answer of exact_pass_kind of 1, 2 or 3 is never changed; where the decision is 4, exact_pass_kind said 0
// and the boundaries d = 128 -> 1, 129 -> 4, 1024 -> 4, 1025 -> 0.
#include <cstdio>
#include <cstdlib>

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

int main() {
    long cases = 0, fours = 0;
    for (int d = 1; d <= 1100; d++)
        for (int f = 0; f < 64; f++) {
            const bool shape = f & 1, bytes = f & 2, float_ok = f & 4, opt_float = f & 8, opt_wide = f & 16, opt_wb = f & 32;
            const int before = exact_pass_kind(d, shape, bytes, float_ok, opt_float, opt_wide);
            const int got = exact_pass_kind_bytes(d, shape, bytes, float_ok, opt_float, opt_wide, opt_wb);
            cases++;
            if (!opt_wb) CHECK(got == before, "d %d flags %d: %d, the rule without the option says %d", d, f, got, before);
            const bool want4 = shape && bytes && d > 128 && d <= EXACT_WIDE_MAX_D && opt_wb;
            CHECK((got == 4) == want4, "d %d flags %d: %d", d, f, got);
            if (got != 4) CHECK(got == before, "d %d flags %d: %d instead of %d", d, f, got, before);
            if (got == 4) CHECK(before == 0, "d %d flags %d: an answer of %d was changed", d, f, before);
            if (before != 0) CHECK(got == before, "d %d flags %d: %d became %d", d, f, before, got);
            CHECK(exact_kind_is_bytes(got) == (got == 1 || got == 4), "d %d flags %d", d, f);
            fours += got == 4;
        }
    // (d, the four flags that do not matter to the set: float_ok, opt_float, opt_wide) -> 8 combinations for each served d
    CHECK(fours == (long)(EXACT_WIDE_MAX_D - 128) * 8, "served (d, flags): %ld", fours);
    CHECK(exact_pass_kind_bytes(128, true, true, false, false, false, true) == 1, "d 128");
    CHECK(exact_pass_kind_bytes(129, true, true, false, false, false, true) == 4, "d 129");
    CHECK(exact_pass_kind_bytes(1024, true, true, false, false, false, true) == 4, "d 1024");
    CHECK(exact_pass_kind_bytes(1025, true, true, false, false, false, true) == 0, "d 1025");
    CHECK(exact_pass_kind_bytes(200, true, true, true, true, true, false) == 0, "the option off");
    CHECK(exact_pass_kind_bytes(200, true, false, true, true, true, true) == 3, "float lists keep the wide fp16 pass");
    CHECK(exact_pass_kind_bytes(200, true, false, false, false, false, true) == 0, "no byte codes in use, no fp16 options");
    CHECK(exact_pass_kind_bytes(200, false, true, true, true, true, true) == 0, "the shape does not hold");
    CHECK(exact_pass_kind_bytes(96, true, false, true, true, false, true) == 2, "the narrow fp16 pass");
    printf("decisions %ld, served by the wide byte pass %ld, failures %d\n", cases, fours, failures);
    if (failures) return 1;
    printf("DONE\n");
    return 0;
}
