// Query rows that are already in HBM (the `_dev` entry points of include/auncel_amd.h): ingest_rows_kernel reads n
// rows of d fp32 or fp16 elements at a caller's row stride, writes the engine's query layout -- fp32 rows padded to dpad with zeros,
// what upload_rows leaves behind for rows from the host -- and in the same pass computes what IntRange::add computes over the n x d
// real elements (query_range.h: the one element rule).  Every workgroup leaves one partial range; ingest_range_kernel, one wave,
// merges them into the 12 bytes the host reads back before it chooses the arithmetic of the search.  No atomics: the merge is a
// minimum, a maximum and an AND, the order of which changes nothing, and a float atomic minimum would be a compare-and-swap loop on
// one word from every workgroup.  Nothing of the stride gap is read: an element is loaded only if its column is below d.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ivf_kernels.h"

namespace amdivf {

namespace {

__device__ __forceinline__ float ingest_f32(float v) { return v; }
__device__ __forceinline__ float ingest_f32(__half v) { return __half2float(v); }  // (exact: every fp16 value is an fp32 value)

// four consecutive elements by one load (the caller has made sure of the alignment)
__device__ __forceinline__ void ingest_load4(const float* p, float v[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
}
__device__ __forceinline__ void ingest_load4(const __half* p, float v[4]) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    const __half2 a = *reinterpret_cast<const __half2*>(&q.x), b = *reinterpret_cast<const __half2*>(&q.y);
    v[0] = __low2float(a), v[1] = __high2float(a), v[2] = __low2float(b), v[3] = __high2float(b);
}

__device__ __forceinline__ QueryRange wave_range(QueryRange r) {
    for (int off = 32; off > 0; off >>= 1) {
        QueryRange o;
        o.ok = (uint32_t)__shfl_xor((int)r.ok, off);
        o.lo = __shfl_xor(r.lo, off);
        o.hi = __shfl_xor(r.hi, off);
        query_range_merge(r, o);
    }
    return r;
}

// A lane per (row, group of four output columns), grid-strided: t = row * (dpad / 4) + group, which is also the index of the
// 16-byte store into `out`.  wide: x is aligned for a four-element load and ldx % 4 == 0, so every group that lies below d whole
// is one load; the others -- the last group of a row when d % 4 != 0, every group otherwise -- are read element by element, and
// only the elements below d.
template <class T>
__global__ __launch_bounds__(256) void ingest_rows_kernel(const T* __restrict__ x, uint64_t n, uint32_t d, uint32_t dpad, uint64_t ldx, int wide,
                                                          float* __restrict__ out, QueryRange* __restrict__ parts) {
    const uint32_t nsteps = dpad >> 2;
    const uint64_t items = n * nsteps;
    QueryRange r = query_range_empty();
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < items; t += (uint64_t)gridDim.x * 256) {
        const uint64_t i = t / nsteps;
        const uint32_t c = (uint32_t)(t - i * nsteps) * 4;
        const T* src = x + i * ldx + c;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (wide && c + 4 <= d) {
            ingest_load4(src, v);
            for (int j = 0; j < 4; j++) query_range_add(r, v[j]);
        } else {
            for (int j = 0; j < 4; j++)
                if (c + j < d) {
                    v[j] = ingest_f32(src[j]);
                    query_range_add(r, v[j]);
                }
        }
        reinterpret_cast<float4*>(out)[t] = make_float4(v[0], v[1], v[2], v[3]);
    }
    r = wave_range(r);
    __shared__ QueryRange sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        QueryRange all = sh[0];
        for (int w = 1; w < 4; w++) query_range_merge(all, sh[w]);
        parts[blockIdx.x] = all;
    }
}

// one wave: the partial ranges of the launch above -> the call's range
__global__ __launch_bounds__(64) void ingest_range_kernel(const QueryRange* __restrict__ parts, uint32_t nparts, QueryRange* __restrict__ result) {
    QueryRange r = query_range_empty();
    for (uint32_t p = threadIdx.x; p < nparts; p += 64) query_range_merge(r, parts[p]);
    r = wave_range(r);
    if (threadIdx.x == 0) *result = r;
}

template <class T> void ingest_launch(const T* x, size_t n, int d, int dpad, size_t ldx, float* out, QueryRange* parts, hipStream_t s) {
    const uint64_t items = (uint64_t)n * (uint64_t)(dpad >> 2);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((items + 255) / 256, INGEST_MAX_PARTS);
    const int wide = reinterpret_cast<uintptr_t>(x) % (4 * sizeof(T)) == 0 && ldx % 4 == 0;
    LAUNCH(ingest_rows_kernel<T>, dim3(blocks), dim3(256), 0, s, x, (uint64_t)n, (uint32_t)d, (uint32_t)dpad, (uint64_t)ldx, wide, out, parts);
    LAUNCH(ingest_range_kernel, dim3(1), dim3(64), 0, s, parts, blocks, parts + INGEST_MAX_PARTS);
}

}  // namespace

void launch_ingest_rows(const void* x, int dtype, size_t n, int d, int dpad, size_t ldx, float* out, QueryRange* parts, hipStream_t s) {
    if (n == 0) return;
    if (dtype == 0) ingest_launch(static_cast<const float*>(x), n, d, dpad, ldx, out, parts, s);
    else if (dtype == 1) ingest_launch(static_cast<const __half*>(x), n, d, dpad, ldx, out, parts, s);
    else throw std::runtime_error("ingest_rows: unknown dtype");
}

}  // namespace amdivf
