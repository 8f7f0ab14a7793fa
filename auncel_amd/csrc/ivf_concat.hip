// Device-resident indexes joined on the device (amd_ivf_concat): list l of the result is, over an ordered set of parts, a run of each
// part's list l.  Every size is known on the host, so the host makes the result's offsets and, per part, where its run of every list
// starts and how far into the joined list it reaches; the rows never leave HBM.  One pass, bound by memory traffic and driven by the
// output: a row's place is a pure function of the tables -- the same bytes on every run, whatever order the workgroups run in.
#include <hip/hip_runtime.h>

#include "ivf_dev.h"

namespace amdivf {

namespace {

constexpr int ROWS_PER_WG = 64;

// a workgroup per 64 rows of the result: one thread a row finds the row's list, the part it comes from and its source row, and writes
// its id; then the workgroup copies the rows, four 16-byte pieces in flight per thread.  The range of the values (IntRange) rides on
// the loads (RangeWatch).
__global__ __launch_bounds__(256) void concat_rows_kernel(const ConcatPart* __restrict__ parts, uint32_t nparts,
                                                          const uint64_t* __restrict__ src_start, const uint64_t* __restrict__ cum,
                                                          const uint64_t* __restrict__ new_off, uint32_t nlist, uint64_t nt, int dpad,
                                                          float* __restrict__ codes, int64_t* __restrict__ ids, uint32_t* range) {
    __shared__ const float4* s_src[ROWS_PER_WG];
    const uint32_t nsteps = (uint32_t)dpad >> 2;
    const uint64_t row0 = (uint64_t)blockIdx.x * ROWS_PER_WG;
    if (threadIdx.x < ROWS_PER_WG) {
        const uint64_t row = row0 + threadIdx.x;
        const float4* src = nullptr;
        if (row < nt) {
            const uint32_t l = list_of(new_off, nlist, row, 0);
            const uint64_t pos = row - new_off[l];
            // the first part whose run ends behind pos (pos < the list's length = the last part's entry: there is one; a part that
            // gives the list nothing repeats its predecessor's entry and is never chosen)
            uint32_t lo = 0, hi = nparts - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (cum[(uint64_t)mid * nlist + l] > pos) hi = mid;
                else lo = mid + 1;
            }
            const uint64_t before = lo ? cum[(uint64_t)(lo - 1) * nlist + l] : 0;
            const uint64_t s = src_start[(uint64_t)lo * nlist + l] + (pos - before);
            const ConcatPart p = parts[lo];
            ids[row] = (int64_t)((uint64_t)p.ids[s] + (uint64_t)p.id_add);
            src = reinterpret_cast<const float4*>(p.codes) + s * nsteps;
        }
        s_src[threadIdx.x] = src;
    }
    __syncthreads();
    const uint64_t nrows = nt - row0 < (uint64_t)ROWS_PER_WG ? nt - row0 : (uint64_t)ROWS_PER_WG;
    const uint32_t total = (uint32_t)nrows * nsteps;
    float4* dst4 = reinterpret_cast<float4*>(codes) + row0 * nsteps;
    RangeWatch watch;
    for (uint32_t i0 = threadIdx.x; i0 < total; i0 += 4 * 256) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t i = i0 + u * 256;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < total) {
                const uint32_t r = i / nsteps;
                v[u] = s_src[r][i - r * nsteps];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t i = i0 + u * 256;
            if (i < total) dst4[i] = v[u];
            watch.look(v[u]);
        }
    }
    watch.commit(range, threadIdx.x & 63);
}

}  // namespace

void launch_concat_rows(const ConcatPart* parts, uint32_t nparts, const uint64_t* src_start, const uint64_t* cum, const uint64_t* new_off,
                        uint32_t nlist, uint64_t nt, int dpad, float* codes, int64_t* ids, uint32_t* range, hipStream_t s) {
    if (nt == 0) return;
    if (nparts == 0 || dpad % 4) throw std::runtime_error("concat_rows: no parts, or rows that are not copied in 16-byte pieces");
    const uint64_t grid = (nt + ROWS_PER_WG - 1) / ROWS_PER_WG;
    LAUNCH(concat_rows_kernel, dim3((unsigned)grid), dim3(256), 0, s, parts, nparts, src_start, cum, new_off, nlist, nt, dpad, codes, ids, range);
}

}  // namespace amdivf
