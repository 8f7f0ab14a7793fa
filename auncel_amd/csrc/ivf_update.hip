// In-place updates of a device-resident index (amd_ivf_update_lists, amd_ivf_remove_ids, amd_ivf_add between searches): the
// new layout is built in HBM from the old one.  Offsets move when any earlier list changes size, so every buffer family is
// rebuilt into a fresh buffer: the entries (or blocks) a list keeps are copied device to device, the written entries are scattered
// from one staged upload, and the blocks an update touched are encoded again by the same device code that builds a whole copy
// (ivf_kernels.hip / ivf_filter.hip: launch_*_list).  The copies are bandwidth work: 16-byte loads and stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ivf_dev.h"

namespace amdivf {

namespace {

constexpr int ROWS_PER_WG = 64;  // (list_of: ivf_dev.h)

// a workgroup per 64 rows of the new layout: one thread a row finds where the row comes from, then the workgroup copies the rows,
// four 16-byte pieces in flight per thread
__global__ __launch_bounds__(256) void relayout_rows_kernel(const float* __restrict__ old_codes, const int64_t* __restrict__ old_ids,
                                                            const uint64_t* __restrict__ old_off, const uint64_t* __restrict__ new_off,
                                                            uint32_t nlist, uint64_t nt_new, int dpad, float* __restrict__ codes,
                                                            int64_t* __restrict__ ids) {
    __shared__ int64_t s_src[ROWS_PER_WG];
    const uint64_t row0 = (uint64_t)blockIdx.x * ROWS_PER_WG;
    if (threadIdx.x < ROWS_PER_WG) {
        const uint64_t row = row0 + threadIdx.x;
        int64_t src = -1;
        if (row < nt_new) {
            const uint32_t l = list_of(new_off, nlist, row, 0);
            const uint64_t pos = row - new_off[l];
            if (pos < old_off[l + 1] - old_off[l]) src = (int64_t)(old_off[l] + pos);
            ids[row] = src >= 0 ? old_ids[src] : -1;
        }
        s_src[threadIdx.x] = src;
    }
    __syncthreads();
    const uint32_t nsteps = (uint32_t)dpad >> 2;
    const uint64_t nrows = nt_new - row0 < (uint64_t)ROWS_PER_WG ? nt_new - row0 : (uint64_t)ROWS_PER_WG;
    const uint32_t total = (uint32_t)nrows * nsteps;
    const float4* src4 = reinterpret_cast<const float4*>(old_codes);
    float4* dst4 = reinterpret_cast<float4*>(codes) + row0 * nsteps;
    for (uint32_t i0 = threadIdx.x; i0 < total; i0 += 4 * 256) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t i = i0 + u * 256;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < total) {
                const uint32_t r = i / nsteps;
                const int64_t s = s_src[r];
                if (s >= 0) v[u] = src4[(uint64_t)s * nsteps + (i - r * nsteps)];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t i = i0 + u * 256;
            if (i < total) dst4[i] = v[u];
        }
    }
}

// one wave per written entry
__global__ __launch_bounds__(256) void scatter_rows_kernel(const uint64_t* __restrict__ rows, const int64_t* __restrict__ wids,
                                                           const float* __restrict__ vals, uint64_t nw, int dpad, float* __restrict__ codes,
                                                           int64_t* __restrict__ ids) {
    const int lane = threadIdx.x & 63;
    const uint32_t nsteps = (uint32_t)dpad >> 2;
    for (uint64_t e = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); e < nw; e += (uint64_t)gridDim.x * 4) {
        const uint64_t row = rows[e];
        const float4* src = reinterpret_cast<const float4*>(vals) + e * nsteps;
        float4* dst = reinterpret_cast<float4*>(codes) + row * nsteps;
        for (uint32_t s = lane; s < nsteps; s += 64) dst[s] = src[s];
        if (lane == 0) ids[row] = wids[e];
    }
}

__device__ __forceinline__ void copy_pieces(const uint4* __restrict__ src, uint4* __restrict__ dst, uint64_t n16, int lane) {
    for (uint64_t i0 = lane; i0 < n16; i0 += 4 * 64) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint64_t i = i0 + u * 64;
            if (i < n16) v[u] = src[i];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint64_t i = i0 + u * 64;
            if (i < n16) dst[i] = v[u];
        }
    }
}

// one wave per block of the new layout
__global__ __launch_bounds__(256) void relayout_blocks_kernel(const uint4* __restrict__ old_main, uint4* __restrict__ new_main, uint64_t main16,
                                                              const uint4* __restrict__ old_side, uint4* __restrict__ new_side, uint64_t side16,
                                                              const uint64_t* __restrict__ old_boff, const uint64_t* __restrict__ new_boff,
                                                              uint32_t nlist, uint64_t nblk_new, int shift) {
    const uint64_t blk = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (blk >= nblk_new) return;
    const uint32_t l = list_of(new_boff, nlist, blk, shift);
    const uint64_t b = blk - (new_boff[l] >> shift), had = (old_boff[l + 1] >> shift) - (old_boff[l] >> shift);
    if (b >= had) return;  // (a block the list did not have: the update encodes it)
    const uint64_t src = (old_boff[l] >> shift) + b;
    copy_pieces(old_main + src * main16, new_main + blk * main16, main16, lane);
    if (old_side) copy_pieces(old_side + src * side16, new_side + blk * side16, side16, lane);
}

}  // namespace

void launch_relayout_rows(const float* old_codes, const int64_t* old_ids, const uint64_t* old_off, const uint64_t* new_off, uint32_t nlist,
                          uint64_t nt_new, int dpad, float* codes, int64_t* ids, hipStream_t s) {
    if (nt_new == 0) return;
    const uint64_t grid = (nt_new + ROWS_PER_WG - 1) / ROWS_PER_WG;
    LAUNCH(relayout_rows_kernel, dim3((unsigned)grid), dim3(256), 0, s, old_codes, old_ids, old_off, new_off, nlist, nt_new, dpad, codes, ids);
}

void launch_scatter_rows(const uint64_t* rows, const int64_t* wids, const float* vals, uint64_t nw, int dpad, float* codes, int64_t* ids,
                         hipStream_t s) {
    if (nw == 0) return;
    const uint64_t grid = std::min<uint64_t>((nw + 3) / 4, 65536);
    LAUNCH(scatter_rows_kernel, dim3((unsigned)grid), dim3(256), 0, s, rows, wids, vals, nw, dpad, codes, ids);
}

void launch_relayout_blocks(const void* old_main, void* new_main, uint64_t block_bytes, const void* old_side, void* new_side, uint64_t side_bytes,
                            const uint64_t* old_boff, const uint64_t* new_boff, uint32_t nlist, uint64_t nblk_new, int shift, hipStream_t s) {
    if (nblk_new == 0) return;
    if (block_bytes % 16 || side_bytes % 16) throw std::runtime_error("relayout_blocks: blocks are copied in 16-byte pieces");
    LAUNCH(relayout_blocks_kernel, dim3((unsigned)((nblk_new + 3) / 4)), dim3(256), 0, s, static_cast<const uint4*>(old_main),
           static_cast<uint4*>(new_main), block_bytes / 16, static_cast<const uint4*>(old_side), static_cast<uint4*>(new_side), side_bytes / 16,
           old_boff, new_boff, nlist, nblk_new, shift);
}

}  // namespace amdivf
