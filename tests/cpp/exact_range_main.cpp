// The host-only part of the exact range search (auncel_amd/csrc/exact_args.h: the argument checks, the threshold the byte list pass is
// given for a radius, the strict range test and the candidates' sort key) as a program of its own, for the address and
// undefined-behaviour sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/exact_range_main.cpp -o exact_range_main
// Prints DONE and returns 0 when every check held.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

// what scan_all_kernel asks of a threshold before it emits anything for the query
static bool passes_guard(float t) { return t == t && std::fabs(t) <= 1073741824.f; }
// the pass's own test of an exact integer distance against a threshold (L2: dis <= floor(tau); IP: dis >= ceil(tau))
static bool pass_emits(bool l2, float tau, long dis) { return l2 ? dis <= (long)std::floor(tau) : dis >= (long)std::ceil(tau); }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const long far = 1L << 24;  // the byte rule: |dis| <= d m^2 <= 2^24
    bool none = false;

    // ---- NaN maps to none
    (void)exact_range_threshold(nan, &none);
    CHECK(none);
    (void)exact_range_threshold(-nan, &none);
    CHECK(none);

    // ---- +-inf and +-1e30: finite, inside the kernel's guard, on the right side for both metrics: on the full side the pass emits
    // every distance the byte rule allows, on the empty side none -- which is what the strict test on the radius itself decides
    for (float r : {inf, 1e30f, 3e9f, 1073741824.f, 268435457.f}) {
        const float t = exact_range_threshold(r, &none);
        CHECK(!none && std::isfinite(t) && passes_guard(t) && t > (float)far);
        for (long dis : {0L, 1L, far - 1, far}) {
            CHECK(pass_emits(true, t, dis) && exact_range_within(true, r, (float)dis));     // L2: everything
            CHECK(!pass_emits(false, t, dis) && !exact_range_within(false, r, (float)dis));  // IP: nothing
            CHECK(!pass_emits(false, t, -dis) && !exact_range_within(false, r, (float)-dis));
        }
    }
    for (float r : {-inf, -1e30f, -3e9f, -1073741824.f, -268435457.f}) {
        const float t = exact_range_threshold(r, &none);
        CHECK(!none && std::isfinite(t) && passes_guard(t) && t < -(float)far);
        for (long dis : {0L, 1L, far - 1, far}) {
            CHECK(!pass_emits(true, t, dis) && !exact_range_within(true, r, (float)dis));  // L2: nothing
            CHECK(pass_emits(false, t, dis) && exact_range_within(false, r, (float)dis));   // IP: everything
            CHECK(pass_emits(false, t, -dis) && exact_range_within(false, r, (float)-dis));
        }
    }

    // ---- a threshold inside the range is returned unchanged, bit for bit, and passes the guard
    for (float r : {0.f, -0.f, 1.f, -1.f, 0.5f, 12345.75f, -77.25f, 16777216.f, -16777216.f, 268435456.f, -268435456.f, 1e-30f, -1e-30f,
                    std::numeric_limits<float>::denorm_min()}) {
        const float t = exact_range_threshold(r, &none);
        uint32_t a, b;
        std::memcpy(&a, &t, 4);
        std::memcpy(&b, &r, 4);
        CHECK(!none && a == b && passes_guard(t));
    }
    // ... and every threshold returned at all passes the guard: a sweep over the exponents on either side
    for (int e = -149; e <= 127; e++)
        for (float m : {1.f, 1.5f, 1.9999999f})
            for (float sg : {1.f, -1.f}) {
                const float r = sg * std::ldexp(m, e);
                const float t = exact_range_threshold(r, &none);
                CHECK(!none && passes_guard(t) && (std::fabs(r) > EXACT_RANGE_CLAMP ? t == sg * EXACT_RANGE_CLAMP : t == r));
            }
    CHECK(EXACT_RANGE_CLAMP > 16777216.f && EXACT_RANGE_CLAMP <= EXACT_SCAN_GUARD);

    // ---- the pass's non-strict test is a superset of the strict range test at every radius around integers
    for (float r : {9.f, 9.5f, 10.f, std::nextafter(10.f, 11.f), std::nextafter(10.f, 9.f), -3.f, -2.5f, 0.f})
        for (long dis = -12; dis <= 12; dis++)
            for (bool l2 : {true, false})
                if (exact_range_within(l2, r, (float)dis)) CHECK(pass_emits(l2, exact_range_threshold(r, &none), dis));
    // the strict edge itself
    CHECK(!exact_range_within(true, 10.f, 10.f) && exact_range_within(true, std::nextafter(10.f, 11.f), 10.f));
    CHECK(!exact_range_within(false, 10.f, 10.f) && exact_range_within(false, std::nextafter(10.f, 9.f), 10.f));
    CHECK(!exact_range_within(true, nan, 0.f) && !exact_range_within(false, nan, 0.f));

    // ---- the sort key: position order whatever the distances, invalid last
    {
        std::vector<uint64_t> v = {exact_range_key(7, 0xffffffffu), EXACT_RANGE_INVALID, exact_range_key(3, 0x7f800000u), exact_range_key(0xfffffffeu, 0u),
                                   exact_range_key(0, 5u), EXACT_RANGE_INVALID, exact_range_key(4, 0u)};
        std::sort(v.begin(), v.end());
        const uint32_t want[5] = {0, 3, 4, 7, 0xfffffffeu};
        for (int i = 0; i < 5; i++) CHECK((uint32_t)(v[i] >> 32) == want[i]);
        CHECK(v[5] == EXACT_RANGE_INVALID && v[6] == EXACT_RANGE_INVALID && (uint32_t)v[0] == 5u);
        CHECK(exact_range_key(0xfffffffeu, 0xffffffffu) != EXACT_RANGE_INVALID);
    }

    // ---- the argument checks
    int x = 0;
    const void* p = &x;
    CHECK(exact_range_args_error(true, true, 0, 5, p).empty());
    CHECK(exact_range_args_error(true, false, 0, 0, p).empty());  // n = 0 needs no rows
    CHECK(exact_range_args_error(false, true, 0, 5, p).find("null handle") != std::string::npos);
    CHECK(exact_range_args_error(true, true, 0, 5, nullptr).find("null lims") != std::string::npos);
    CHECK(exact_range_args_error(true, true, 0, 0, nullptr).find("null lims") != std::string::npos);  // lims[0] is written for n = 0 too
    CHECK(exact_range_args_error(true, false, 0, 5, p).find("null") != std::string::npos);
    CHECK(exact_range_args_error(true, true, ~(size_t)0, 2, p).find("out of bounds") != std::string::npos);
    CHECK(exact_range_args_error(true, true, ~(size_t)0, 0, p).empty());
    CHECK(exact_range_selected_args_error(true, false, true, 0, 5, p).find("null selector") != std::string::npos);
    CHECK(exact_range_selected_args_error(false, false, true, 0, 5, p).find("null handle") != std::string::npos);
    CHECK(exact_range_selected_args_error(true, true, true, 0, 5, p).empty());
    CHECK(exact_range_selected_args_error(true, true, true, 0, 5, nullptr).find("null lims") != std::string::npos);

    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("DONE\n");
    return 0;
}
