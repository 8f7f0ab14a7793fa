// The host side of amd_ivf_build_dev (include/auncel_amd.h): what it refuses before anything is launched -- a missing handle or
// result slot, a clone, a handle without centroids, rows that dev_rows_error refuses, ids or list numbers that are not aligned
// device memory of the handle's device -- and how its second sweep is cut into chunks.  Plain C++ beside dev_io_args.h, nothing of
// the device in it, so it builds on its own (tests/cpp/build_args_main.cpp, which is what the sanitizers are pointed at).
#pragma once
#include <algorithm>

#include "dev_io_args.h"

namespace amdivf {

struct BuildArgs {
    bool have_handle, have_out, is_clone, have_centroids;
    size_t n, d;
    const void* x;
    DevPtrKind kind_x;
    int dtype;
    size_t ldx;
    const void* ids;  // or null: id_base + i
    DevPtrKind kind_ids;
    const void* assign;  // or null: the handle's own assignment
    DevPtrKind kind_assign;
};

// empty when the call may go ahead.  n == 0 makes an empty index and follows no pointer, so none is looked at.
inline std::string build_args_error(const BuildArgs& a) {
    const std::string w = "build_dev: ";
    if (!a.have_handle || !a.have_out) return w + "null argument";
    if (a.is_clone) return w + "not available on a search context made by amd_ivf_clone: use the owning handle";
    if (!a.have_centroids) return w + "quantizer has no centroids";
    if (a.n == 0) return std::string();
    std::string e = dev_rows_error(a.x, a.kind_x, a.dtype, a.ldx, a.d);
    if (e.empty() && a.ids) e = dev_ptr_error("d_ids", a.ids, a.kind_ids, sizeof(int64_t));
    if (e.empty() && a.assign) e = dev_ptr_error("d_assign", a.assign, a.kind_assign, sizeof(int64_t));
    return e.empty() ? e : w + e;
}

// what a chunk's tile-by-list matrix of counts may take
constexpr uint64_t BUILD_CHUNK_BYTES = 64ull << 20;

// Tiles of `tile` rows in one chunk of the second sweep: as many as keep the chunk's tile-by-list matrix of 32-bit counts within
// budget_bytes, at least one, at most all; forced_rows != 0 (tests) asks for chunks of that many rows instead, rounded down to
// whole tiles.
inline uint64_t build_chunk_tiles(uint64_t n, uint64_t nlist, uint64_t tile, uint64_t budget_bytes, uint64_t forced_rows) {
    const uint64_t all = std::max<uint64_t>((n + tile - 1) / tile, 1);
    uint64_t tiles = forced_rows ? forced_rows / tile : budget_bytes / (4 * std::max<uint64_t>(nlist, 1));
    return std::min(std::max<uint64_t>(tiles, 1), all);
}

}  // namespace amdivf
