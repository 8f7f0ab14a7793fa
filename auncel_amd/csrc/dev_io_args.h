// The host side of the `_dev` entry points (include/auncel_amd.h: amd_ivf_set_queries_dev, amd_ivf_search_dev & co): what they
// refuse before anything is launched -- a null pointer, a pointer that is not device memory of the handle's device, a row stride
// below d, an element type that is neither fp32 nor fp16, a pointer misaligned for its element type.  Plain C++, nothing of the
// device in it: what the runtime says about a pointer is passed in as DevPtrKind, so this builds on its own
// (tests/cpp/query_range_main.cpp, which is what the address and undefined-behaviour sanitizers are pointed at).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace amdivf {

// what hipPointerGetAttributes reports of a pointer, as far as these calls care
enum DevPtrKind {
    DEV_PTR_DEVICE = 0,        // device memory of the handle's device
    DEV_PTR_OTHER_DEVICE = 1,  // device memory of another device
    DEV_PTR_HOST = 2,          // page-locked or registered host memory, managed memory
    DEV_PTR_UNKNOWN = 3,       // nothing the runtime knows: pageable host memory, a stale or made-up address
};

constexpr int DEV_DTYPE_F32 = 0, DEV_DTYPE_F16 = 1;

// bytes of an element of `dtype`, 0 for a dtype that does not exist
inline size_t dev_dtype_size(int dtype) { return dtype == DEV_DTYPE_F32 ? 4 : dtype == DEV_DTYPE_F16 ? 2 : 0; }

// one pointer argument `name` of elements of `elem` bytes: empty, or the refusal
inline std::string dev_ptr_error(const char* name, const void* p, DevPtrKind kind, size_t elem) {
    const std::string w(name);
    if (!p) return w + ": null pointer";
    if (kind == DEV_PTR_OTHER_DEVICE) return w + ": device memory of another device than the handle's";
    if (kind != DEV_PTR_DEVICE) return w + ": not a device pointer";
    if (elem > 1 && reinterpret_cast<uintptr_t>(p) % elem != 0) return w + ": misaligned for its element type";
    return std::string();
}

// the query rows of a call: n rows of d elements of `dtype`, row stride ldx elements
inline std::string dev_rows_error(const void* x, DevPtrKind kind, int dtype, size_t ldx, size_t d) {
    const size_t elem = dev_dtype_size(dtype);
    if (elem == 0) return "dtype must be 0 (fp32) or 1 (fp16)";
    if (ldx < d) return "ldx must be at least d";
    return dev_ptr_error("d_x", x, kind, elem);
}

// the result buffers: n x k floats and n x k int64
inline std::string dev_out_error(const void* D, DevPtrKind kind_D, const void* I, DevPtrKind kind_I) {
    const std::string e = dev_ptr_error("d_D", D, kind_D, sizeof(float));
    if (!e.empty()) return e;
    return dev_ptr_error("d_I", I, kind_I, sizeof(int64_t));
}

// everything a `_dev` call with query rows checks, in the order it reports: empty when the call may go ahead.  have_rows /
// have_out: the call takes query rows / result buffers (amd_ivf_set_queries_dev has no results, the resident calls no rows).
inline std::string dev_call_error(const char* what, bool have_handle, bool have_rows, const void* x, DevPtrKind kind_x, int dtype, size_t ldx,
                                  size_t d, bool have_out, const void* D, DevPtrKind kind_D, const void* I, DevPtrKind kind_I) {
    const std::string w = std::string(what) + ": ";
    if (!have_handle) return w + "null handle";
    std::string e;
    if (have_rows) e = dev_rows_error(x, kind_x, dtype, ldx, d);
    if (e.empty() && have_out) e = dev_out_error(D, kind_D, I, kind_I);
    return e.empty() ? e : w + e;
}

}  // namespace amdivf
