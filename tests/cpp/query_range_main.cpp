// The host-compilable half of the `_dev` entry points, as a program of its own: query_range.h's element rule and blockwise merge
// against a literal restatement of the engine's IntRange::add, and dev_io_args.h's refusals.  Built with
// -fsanitize=address,undefined (tests/test_query_range_cpu.py).
//
// IntRange::add casts (int)v, which is undefined for a v outside the range of int and for NaN: the literal loop is run only over
// arrays for which it is defined; for the others the program asserts ok == false directly.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../../auncel_amd/csrc/dev_io_args.h"
#include "../../auncel_amd/csrc/query_range.h"

using namespace amdivf;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// IntRange::add (ivf_engine.hip), word for word, from a fresh IntRange
struct Literal {
    bool ok = true;
    float lo = 0.f, hi = 0.f;
    void add(const float* x, size_t n) {
        if (!ok) return;
        float l = lo, h = hi;
        bool good = true;
        for (size_t i = 0; i < n; i++) {
            const float v = x[i];
            good &= (v == (float)(int)v) & (v >= -4095.f) & (v <= 4095.f);
            l = v < l ? v : l;
            h = v > h ? v : h;
        }
        ok = good;
        lo = l;
        hi = h;
    }
};

// whether (int)v is defined for every element
static bool cast_defined(const std::vector<float>& x) {
    for (float v : x)
        if (!(v > -2147483904.f && v < 2147483648.f)) return false;  // (NaN fails both)
    return true;
}

static const size_t BLOCKS[] = {1, 2, 3, 63, 64, 65, 255, 256, 257, 1024, 1000000};

// the shared rule, whole and split at every block size, against the literal loop (or against ok == false where it is undefined)
static void check_array(const std::vector<float>& x, const char* what) {
    const QueryRange whole = query_range_blockwise(x.data(), x.size(), x.size() + 1);
    if (cast_defined(x)) {
        Literal lit;
        lit.add(x.data(), x.size());
        if ((whole.ok != 0) != lit.ok) printf("ok differs: %s\n", what);
        CHECK((whole.ok != 0) == lit.ok);
        if (lit.ok) {
            CHECK(whole.lo == lit.lo && whole.hi == lit.hi);
            CHECK(!std::signbit(whole.lo) || whole.lo != 0.f);  // (never -0)
        }
    } else {
        if (whole.ok) printf("ok for an array the cast is undefined for: %s\n", what);
        CHECK(whole.ok == 0);
    }
    for (size_t b : BLOCKS) {
        const QueryRange parts = query_range_blockwise(x.data(), x.size(), b);
        CHECK(parts.ok == whole.ok);
        if (whole.ok) CHECK(parts.lo == whole.lo && parts.hi == whole.hi);
        CHECK(!std::isnan(parts.lo) && !std::isnan(parts.hi));
    }
}

int main() {
    std::mt19937 rng(12345);
    // ---- random arrays: bytes, signed integers within and across the bound, fractions, mixtures
    for (int round = 0; round < 200; round++) {
        const size_t n = 1 + rng() % 700;
        std::vector<float> x(n);
        const int kind = round % 5;
        for (auto& v : x) {
            if (kind == 0) v = (float)(rng() % 256);
            else if (kind == 1) v = (float)((int)(rng() % 8191) - 4095);
            else if (kind == 2) v = (float)((int)(rng() % 8201) - 4100);
            else if (kind == 3) v = (float)(rng() % 256) + ((rng() % 50) == 0 ? 0.5f : 0.f);
            else v = std::ldexp((float)((int)(rng() % 2001) - 1000), (int)(rng() % 40) - 20);
        }
        check_array(x, "random");
    }
    // ---- every edge value, alone in a byte-valued array at every place a block boundary can fall on
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float edges[] = {0.f, 255.f, 255.5f, 256.f, 4095.f, 4097.f, 4096.f, -4095.f, -4097.f, -4096.f, -0.f, 0.5f, -0.5f, 1e30f, -1e30f,
                           FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN, 1e-45f, 2147483648.f, -2147483648.f, -2147483904.f, 16777216.f, inf, -inf, nan,
                           std::nextafter(4095.f, 5000.f), std::nextafter(-4095.f, -5000.f), std::nextafter(1.f, 2.f)};
    for (float e : edges) {
        // the element rule itself
        const bool want = e >= -4095.f && e <= 4095.f && e == (float)(long long)(e >= -4095.f && e <= 4095.f ? e : 0.f);
        CHECK(query_elem_ok(e) == want);
        const size_t n = 64 * 5 + 1;
        for (size_t at : {(size_t)0, (size_t)1, (size_t)62, (size_t)63, (size_t)64, (size_t)65, (size_t)255, (size_t)256, (size_t)257, n - 1}) {
            std::vector<float> x(n);
            for (size_t i = 0; i < n; i++) x[i] = (float)(i * 37 % 256);
            x[at] = e;
            check_array(x, "edge");
        }
    }
    CHECK(query_elem_ok(-0.f) && query_elem_ok(4095.f) && query_elem_ok(-4095.f));
    CHECK(!query_elem_ok(4097.f) && !query_elem_ok(-4097.f) && !query_elem_ok(255.5f) && !query_elem_ok(nan) && !query_elem_ok(inf));
    CHECK(!query_elem_ok(1e30f) && !query_elem_ok(-1e30f));
    // ---- all-integer arrays split at every block boundary: the parts' ranges merge to the whole's
    {
        std::vector<float> x(300);
        for (size_t i = 0; i < x.size(); i++) x[i] = (float)((int)(i * 131 % 8191) - 4095);
        Literal lit;
        lit.add(x.data(), x.size());
        CHECK(lit.ok);
        for (size_t b = 1; b <= x.size() + 1; b++) {
            const QueryRange r = query_range_blockwise(x.data(), x.size(), b);
            CHECK(r.ok == 1 && r.lo == lit.lo && r.hi == lit.hi);
        }
        // a two-way split at every place, merged in both orders
        for (size_t cut = 0; cut <= x.size(); cut++) {
            QueryRange a = query_range_blockwise(x.data(), cut, cut + 1), b = query_range_blockwise(x.data() + cut, x.size() - cut, x.size() + 1);
            QueryRange ab = a, ba = b;
            query_range_merge(ab, b);
            query_range_merge(ba, a);
            CHECK(ab.ok == 1 && ba.ok == 1 && ab.lo == lit.lo && ba.lo == lit.lo && ab.hi == lit.hi && ba.hi == lit.hi);
        }
    }
    // ---- an empty set, and positive-only / negative-only sets (lo and hi start from 0)
    {
        const QueryRange e = query_range_blockwise(nullptr, 0, 64);
        CHECK(e.ok == 1 && e.lo == 0.f && e.hi == 0.f);
        std::vector<float> pos = {3.f, 7.f, 200.f}, neg = {-3.f, -7.f};
        const QueryRange p = query_range_blockwise(pos.data(), pos.size(), 2), m = query_range_blockwise(neg.data(), neg.size(), 1);
        CHECK(p.lo == 0.f && p.hi == 200.f && m.lo == -7.f && m.hi == 0.f);
    }
    CHECK(sizeof(QueryRange) == 12);

    // ---- dev_io_args.h
    {
        alignas(16) static char mem[64];
        const void* p = mem;
        const void* odd = mem + 1;
        const void* two = mem + 2;
        CHECK(dev_dtype_size(0) == 4 && dev_dtype_size(1) == 2 && dev_dtype_size(2) == 0 && dev_dtype_size(-1) == 0);
        CHECK(dev_rows_error(p, DEV_PTR_DEVICE, 0, 8, 8).empty());
        CHECK(dev_rows_error(p, DEV_PTR_DEVICE, 1, 9, 8).empty());
        CHECK(dev_rows_error(two, DEV_PTR_DEVICE, 1, 8, 8).empty());  // (aligned for fp16)
        CHECK(dev_rows_error(two, DEV_PTR_DEVICE, 0, 8, 8).find("misaligned") != std::string::npos);
        CHECK(dev_rows_error(odd, DEV_PTR_DEVICE, 1, 8, 8).find("misaligned") != std::string::npos);
        CHECK(dev_rows_error(odd, DEV_PTR_DEVICE, 0, 8, 8).find("misaligned") != std::string::npos);
        CHECK(dev_rows_error(p, DEV_PTR_DEVICE, 2, 8, 8).find("dtype") != std::string::npos);
        CHECK(dev_rows_error(p, DEV_PTR_DEVICE, -1, 8, 8).find("dtype") != std::string::npos);
        CHECK(dev_rows_error(p, DEV_PTR_DEVICE, 0, 7, 8).find("ldx") != std::string::npos);
        CHECK(dev_rows_error(nullptr, DEV_PTR_UNKNOWN, 0, 8, 8).find("null pointer") != std::string::npos);
        CHECK(dev_rows_error(p, DEV_PTR_UNKNOWN, 0, 8, 8).find("not a device pointer") != std::string::npos);
        CHECK(dev_rows_error(p, DEV_PTR_HOST, 0, 8, 8).find("not a device pointer") != std::string::npos);
        CHECK(dev_rows_error(p, DEV_PTR_OTHER_DEVICE, 0, 8, 8).find("another device") != std::string::npos);
        CHECK(dev_out_error(p, DEV_PTR_DEVICE, p, DEV_PTR_DEVICE).empty());
        CHECK(dev_out_error(nullptr, DEV_PTR_DEVICE, p, DEV_PTR_DEVICE).find("d_D: null pointer") != std::string::npos);
        CHECK(dev_out_error(p, DEV_PTR_DEVICE, nullptr, DEV_PTR_DEVICE).find("d_I: null pointer") != std::string::npos);
        CHECK(dev_out_error(p, DEV_PTR_DEVICE, mem + 4, DEV_PTR_DEVICE).find("d_I: misaligned") != std::string::npos);
        CHECK(dev_out_error(mem + 4, DEV_PTR_DEVICE, p, DEV_PTR_DEVICE).empty());
        CHECK(dev_out_error(p, DEV_PTR_HOST, p, DEV_PTR_DEVICE).find("d_D: not a device pointer") != std::string::npos);
        CHECK(dev_out_error(p, DEV_PTR_DEVICE, p, DEV_PTR_UNKNOWN).find("d_I: not a device pointer") != std::string::npos);
        CHECK(dev_call_error("search_dev", false, true, p, DEV_PTR_DEVICE, 0, 8, 8, true, p, DEV_PTR_DEVICE, p, DEV_PTR_DEVICE) == "search_dev: null handle");
        CHECK(dev_call_error("search_dev", true, true, p, DEV_PTR_DEVICE, 0, 8, 8, true, p, DEV_PTR_DEVICE, p, DEV_PTR_DEVICE).empty());
        CHECK(dev_call_error("search_dev", true, true, p, DEV_PTR_DEVICE, 0, 7, 8, true, p, DEV_PTR_DEVICE, p, DEV_PTR_DEVICE) == "search_dev: ldx must be at least d");
        // a call without rows checks only its results; one without results only its rows
        CHECK(dev_call_error("search_resident_dev", true, false, nullptr, DEV_PTR_UNKNOWN, 9, 0, 8, true, p, DEV_PTR_DEVICE, p, DEV_PTR_DEVICE).empty());
        CHECK(dev_call_error("set_queries_dev", true, true, p, DEV_PTR_DEVICE, 1, 8, 8, false, nullptr, DEV_PTR_UNKNOWN, nullptr, DEV_PTR_UNKNOWN).empty());
        CHECK(!dev_call_error("search_resident_dev", true, false, nullptr, DEV_PTR_UNKNOWN, 0, 0, 8, true, nullptr, DEV_PTR_UNKNOWN, p, DEV_PTR_DEVICE).empty());
    }
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("DONE\n");
    return 0;
}
