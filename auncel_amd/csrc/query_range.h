// The value range of a call's query rows (ivf_engine.hip: IntRange), as the device computes it for rows that are already in HBM
// (ivf_ingest.hip, the `_dev` entry points of include/auncel_amd.h): whether every element is an integer within +-4095, and the
// minimum and maximum, each starting from 0.  The element rule lives here once.  Plain C++, nothing of the device in it: the
// kernels and the host read the same definitions, and it builds on its own (tests/cpp/query_range_main.cpp, which is what the
// address and undefined-behaviour sanitizers are pointed at).
//
// IntRange::add tests v == (float)(int)v, a cast that is undefined for a v outside the range of int and for NaN.  The rule here
// tests the bounds first and truncf instead of the cast: the same predicate wherever the cast is defined, false everywhere else.
// lo / hi are what IntRange::add leaves whenever ok is true; nothing reads them otherwise.  (A NaN never replaces either: both
// comparisons are false for it, here as there.)
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define QRANGE_HD __host__ __device__
#else
#define QRANGE_HD
#endif

namespace amdivf {

constexpr float QRANGE_INT_MAX = 4095.f;  // |x|, |y| <= 4095: x - y, (x - y)^2 and x * y are exact in fp32 (IntRange)

struct QueryRange {  // 12 bytes: what the device hands back
    uint32_t ok;
    float lo, hi;
};

QRANGE_HD inline QueryRange query_range_empty() { return QueryRange{1u, 0.f, 0.f}; }

QRANGE_HD inline bool query_elem_ok(float v) { return v >= -QRANGE_INT_MAX && v <= QRANGE_INT_MAX && v == truncf(v); }

QRANGE_HD inline void query_range_add(QueryRange& r, float v) {
    r.ok &= query_elem_ok(v) ? 1u : 0u;
    r.lo = v < r.lo ? v : r.lo;
    r.hi = v > r.hi ? v : r.hi;
}

// two parts of one set of values (no part's lo / hi is ever NaN or -0: see query_range_add, which starts from +0)
QRANGE_HD inline void query_range_merge(QueryRange& r, const QueryRange& o) {
    r.ok &= o.ok;
    r.lo = o.lo < r.lo ? o.lo : r.lo;
    r.hi = o.hi > r.hi ? o.hi : r.hi;
}

// The host-compilable half of the device's reduction: parts of `block` consecutive elements each, merged in order.  (The kernel's
// parts are the elements a workgroup visits, not consecutive ones; the merge is associative and commutative, so any split of the
// elements gives this result.)
inline QueryRange query_range_blockwise(const float* x, size_t n, size_t block) {
    QueryRange all = query_range_empty();
    if (block == 0) block = 1;
    for (size_t b = 0; b < n; b += block) {
        QueryRange part = query_range_empty();
        for (size_t i = b; i < n && i < b + block; i++) query_range_add(part, x[i]);
        query_range_merge(all, part);
    }
    return all;
}

}  // namespace amdivf
