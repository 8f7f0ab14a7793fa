// An index built on the device from rows that are in HBM already (amd_ivf_build_dev): n rows of a caller's tensor, each
// with a list number, grouped into nlist lists in ascending input index -- what amd_ivf_add and its first upload leave behind, without
// a row, an id or a list number crossing to the host.  It is a stable counting sort by list, cut so that no workgroup ever waits for
// another one: the order between the passes is the stream's.
//   sweep 1  build_keys_kernel     list numbers -> a 32-bit key per row (BUILD_SKIP: the row is not stored), list totals by atomics
//            build_offsets_kernel  totals -> list offsets and the block table of the padded copies
//   sweep 2  per chunk of tiles of BUILD_TILE rows (a tile a workgroup):
//            build_count_kernel    rank[i] = earlier rows of i's tile with i's key; cnt[tile][list] = rows of the tile in the list
//            build_scan_kernel     a thread per list walks the chunk's tiles: cnt -> rows of the list in earlier tiles, all chunks
//            build_place_kernel    row i goes to list_off[key] + cnt[tile][key] + rank[i], straight from the caller's tensor
// A row's place is a pure function of the keys: the same bytes on every run, whatever order the workgroups run in.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ivf_dev.h"

namespace amdivf {

namespace {

constexpr uint32_t T = BUILD_TILE;
constexpr uint32_t SKIP = BUILD_SKIP;
static_assert(T == 1024, "four rows a thread of 256, ranks in 16 bits");

// A thread per row, grid-strided by whole workgroups (every lane of a wave is in every trip).  Neighbouring lanes with one key --
// rows that arrive sorted or clustered -- add to the list's total once: the first lane of the run adds the run's length.
__global__ __launch_bounds__(256) void build_keys_kernel(const int64_t* __restrict__ assign, uint64_t n, uint32_t nlist,
                                                         uint32_t* __restrict__ keys, unsigned long long* __restrict__ total,
                                                         uint32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n; base += (uint64_t)gridDim.x * 256) {
        const uint64_t i = base + threadIdx.x;
        uint32_t key = SKIP;
        if (i < n) {
            const int64_t a = assign[i];
            if (a >= 0) {
                if ((uint64_t)a >= nlist) atomicOr(flags, BUILD_FLAG_LIST);  // (the call is refused: the row stays out of every table)
                else key = (uint32_t)a;
            }
            keys[i] = key;
        }
        const uint32_t prev = (uint32_t)__shfl_up((int)key, 1);
        const uint64_t starts = __ballot(lane == 0 || prev != key);
        if (key != SKIP && ((starts >> lane) & 1)) {
            const uint64_t above = lane == 63 ? 0ull : starts >> (lane + 1);
            const uint32_t len = above ? (uint32_t)__ffsll((unsigned long long)above) : 64u - (uint32_t)lane;
            atomicAdd(&total[key], (unsigned long long)len);
        }
    }
}

// one workgroup: the lists' totals into offsets and the block table of the padded copies (mfma_list_blocks, as upload_lists)
__global__ __launch_bounds__(256) void build_offsets_kernel(const unsigned long long* __restrict__ total, uint32_t nlist,
                                                            uint64_t* __restrict__ list_off, uint64_t* __restrict__ block_off,
                                                            uint32_t* __restrict__ flags) {
    __shared__ uint64_t s_n[256], s_b[256];
    const uint32_t t = threadIdx.x, per = (nlist + 255) / 256;
    const uint32_t l0 = t * per < nlist ? t * per : nlist, l1 = l0 + per < nlist ? l0 + per : nlist;
    uint64_t n = 0, b = 0;
    bool long_list = false;
    for (uint32_t l = l0; l < l1; l++) {
        n += total[l];
        b += mfma_list_blocks(total[l]);
        long_list |= (total[l] >> 32) != 0;
    }
    if (long_list) atomicOr(flags, BUILD_FLAG_LONG);
    s_n[t] = n;
    s_b[t] = b;
    __syncthreads();
    if (t == 0) {
        uint64_t rn = 0, rb = 0;
        for (int i = 0; i < 256; i++) {
            const uint64_t cn = s_n[i], cb = s_b[i];
            s_n[i] = rn;
            s_b[i] = rb;
            rn += cn;
            rb += cb;
        }
        list_off[nlist] = rn;
        block_off[nlist] = rb;
    }
    __syncthreads();
    n = s_n[t];
    b = s_b[t];
    for (uint32_t l = l0; l < l1; l++) {
        list_off[l] = n;
        block_off[l] = b;
        n += total[l];
        b += mfma_list_blocks(total[l]);
    }
}

// Rows 256 S .. 256 S + 255 of the tile against the thread's four rows t, t + 256, t + 512, t + 768: a row behind the segment
// counts every equal key of it, the row inside it those before itself, the rows ahead of it nothing.  Every lane reads the same
// four keys by one LDS access (a broadcast), so a trip is one read and 4 (3 - S) + 8 compares and adds a lane.
template <int S> __device__ __forceinline__ void rank_segment(const uint32_t* s_key, const uint32_t (&my)[4], uint32_t (&rank)[4], uint32_t t) {
    for (uint32_t j = 0; j < 256; j += 4) {
        const uint4 k = *reinterpret_cast<const uint4*>(s_key + S * 256 + j);
#pragma unroll
        for (int u = S + 1; u < 4; u++) rank[u] += (k.x == my[u]) + (k.y == my[u]) + (k.z == my[u]) + (k.w == my[u]);
        rank[S] += (k.x == my[S] && j < t) + (k.y == my[S] && j + 1 < t) + (k.z == my[S] && j + 2 < t) + (k.w == my[S] && j + 3 < t);
    }
}

// A workgroup per tile.  The rank of a row among its tile's earlier rows with the same key, by counting: T^2 / 2 compares on keys
// held in LDS.  A sort of key << 10 | position would give the ranks too, but in log^2 T barrier-separated LDS passes, with a second
// pass to find each run's start, and with keys cut to 22 bits; counting has one barrier, no limit on nlist, and its compares are
// well under the time the rows' own bytes take.  The tile's count of a list is the largest rank in it plus one: the
// atomics stay inside the tile's own row of cnt, which the caller has zeroed.
__global__ __launch_bounds__(256) void build_count_kernel(const uint32_t* __restrict__ keys, uint64_t n, uint64_t row0, uint32_t nlist,
                                                          uint16_t* __restrict__ rank_out, uint32_t* __restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) uint32_t s_key[T];
    const uint32_t t = threadIdx.x;
    const uint64_t tile0 = row0 + (uint64_t)blockIdx.x * T;
    uint32_t my[4], rank[4] = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint64_t i = tile0 + t + 256 * u;
        my[u] = i < n ? keys[i] : SKIP;
        s_key[t + 256 * u] = my[u];
    }
    __syncthreads();
    rank_segment<0>(s_key, my, rank, t);
    rank_segment<1>(s_key, my, rank, t);
    rank_segment<2>(s_key, my, rank, t);
    rank_segment<3>(s_key, my, rank, t);
    uint32_t* my_cnt = cnt + (uint64_t)blockIdx.x * nlist;
#pragma unroll
    for (int u = 0; u < 4; u++)
        if (my[u] != SKIP) {
            rank_out[(uint64_t)blockIdx.x * T + t + 256 * u] = (uint16_t)rank[u];
            atomicMax(&my_cnt[my[u]], rank[u] + 1);
        }
}

// A thread per list, so that a tile's counts are read and written by consecutive lanes: cnt[tile][l] becomes the rows of list l in
// the earlier tiles of this chunk and of the chunks before it (running[l], carried to the next chunk).  Eight tiles' loads are in
// flight before the first sum.
__global__ __launch_bounds__(256) void build_scan_kernel(uint32_t* __restrict__ cnt, uint32_t ntiles, uint32_t nlist, uint32_t* __restrict__ running) {
    const uint32_t l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nlist) return;
    uint32_t run = running[l];
    for (uint32_t b0 = 0; b0 < ntiles; b0 += 8) {
        uint32_t c[8];
#pragma unroll
        for (int u = 0; u < 8; u++) c[u] = b0 + u < ntiles ? cnt[(uint64_t)(b0 + u) * nlist + l] : 0u;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (b0 + u < ntiles) cnt[(uint64_t)(b0 + u) * nlist + l] = run;
            run += c[u];
        }
    }
    running[l] = run;
}

// four consecutive elements of a row as fp32, by one load where the caller's layout allows it; only columns below d are read
__device__ __forceinline__ float4 build_load4(const float* p, uint32_t c, uint32_t d, int wide) {
    if (wide && c + 4 <= d) return *reinterpret_cast<const float4*>(p + c);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < 4; j++)
        if (c + j < d) v[j] = p[c + j];
    return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ float4 build_load4(const __half* p, uint32_t c, uint32_t d, int wide) {
    if (wide && c + 4 <= d) {
        const uint2 q = *reinterpret_cast<const uint2*>(p + c);
        const __half2 a = *reinterpret_cast<const __half2*>(&q.x), b = *reinterpret_cast<const __half2*>(&q.y);
        return make_float4(__low2float(a), __high2float(a), __low2float(b), __high2float(b));  // (exact: every fp16 value is an fp32 value)
    }
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < 4; j++)
        if (c + j < d) v[j] = __half2float(p[c + j]);
    return make_float4(v[0], v[1], v[2], v[3]);
}

// A workgroup per tile: a thread a row finds the row's place and writes its id; then the workgroup moves the stored rows from the
// caller's tensor -- its stride, its element type -- into the padded fp32 rows of the lists: consecutive lanes take consecutive
// 16-byte pieces of a row and go on into the next row, four pieces in flight per lane; the padding is written as zeros and the
// stride gap is never read.  The range of the values stored (IntRange) rides on the loads (RangeWatch), one commit a wave.
template <class X>
__global__ __launch_bounds__(256) void build_place_kernel(const X* __restrict__ x, uint64_t ldx, uint32_t d, uint32_t dpad, int wide,
                                                          const int64_t* __restrict__ in_ids, int64_t id_base,
                                                          const uint32_t* __restrict__ keys, const uint16_t* __restrict__ rank,
                                                          const uint32_t* __restrict__ before, const uint64_t* __restrict__ list_off, uint64_t n,
                                                          uint64_t row0, uint32_t nlist, float* __restrict__ codes, int64_t* __restrict__ ids,
                                                          uint32_t* range) {
    __shared__ uint64_t s_dst[T];
    const uint32_t t = threadIdx.x;
    const uint64_t tile0 = row0 + (uint64_t)blockIdx.x * T;
    const uint32_t* my_before = before + (uint64_t)blockIdx.x * nlist;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint32_t r = t + 256 * u;
        const uint64_t i = tile0 + r;
        uint64_t dst = ~0ull;
        if (i < n) {
            const uint32_t key = keys[i];
            if (key != SKIP) {
                dst = list_off[key] + my_before[key] + rank[(uint64_t)blockIdx.x * T + r];
                ids[dst] = in_ids ? in_ids[i] : (int64_t)((uint64_t)id_base + i);
            }
        }
        s_dst[r] = dst;
    }
    __syncthreads();
    const uint32_t nsteps = dpad >> 2;
    const uint32_t nrows = n - tile0 < (uint64_t)T ? (uint32_t)(n - tile0) : T;
    const uint32_t total = nrows * nsteps;
    float4* codes4 = reinterpret_cast<float4*>(codes);
    RangeWatch watch;
    for (uint32_t i0 = t; i0 < total; i0 += 4 * 256) {
        float4 v[4];
        uint64_t at[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t i = i0 + u * 256;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            at[u] = ~0ull;
            if (i < total) {
                const uint32_t r = i / nsteps, g = i - r * nsteps;
                const uint64_t dst = s_dst[r];
                if (dst != ~0ull) {  // (a skipped row is not read: it leaves no trace in the range either)
                    v[u] = build_load4(x + (tile0 + r) * ldx, 4 * g, d, wide);
                    at[u] = dst * nsteps + g;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (at[u] != ~0ull) codes4[at[u]] = v[u];
            watch.look(v[u]);
        }
    }
    watch.commit(range, threadIdx.x & 63);
}

template <class X> void place_launch(const BuildPlaceArgs& a, const X* x, hipStream_t s) {
    const int wide = reinterpret_cast<uintptr_t>(x) % (4 * sizeof(X)) == 0 && a.ldx % 4 == 0;
    LAUNCH(build_place_kernel<X>, dim3(a.ntiles), dim3(256), 0, s, x, a.ldx, (uint32_t)a.d, (uint32_t)a.dpad, wide, a.in_ids, a.id_base, a.keys,
           a.rank, a.before, a.list_off, a.n, a.row0, a.nlist, a.codes, a.ids, a.range);
}

}  // namespace

void launch_build_keys(const int64_t* assign, uint64_t n, uint32_t nlist, uint32_t* keys, unsigned long long* total, uint32_t* flags, hipStream_t s) {
    if (n == 0) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 20);
    LAUNCH(build_keys_kernel, dim3(grid), dim3(256), 0, s, assign, n, nlist, keys, total, flags);
}

void launch_build_offsets(const unsigned long long* total, uint32_t nlist, uint64_t* list_off, uint64_t* block_off, uint32_t* flags, hipStream_t s) {
    LAUNCH(build_offsets_kernel, dim3(1), dim3(256), 0, s, total, nlist, list_off, block_off, flags);
}

void launch_build_count(const uint32_t* keys, uint64_t n, uint64_t row0, uint32_t ntiles, uint32_t nlist, uint16_t* rank, uint32_t* cnt, hipStream_t s) {
    if (ntiles == 0) return;
    LAUNCH(build_count_kernel, dim3(ntiles), dim3(256), 0, s, keys, n, row0, nlist, rank, cnt);
}

void launch_build_scan(uint32_t* cnt, uint32_t ntiles, uint32_t nlist, uint32_t* running, hipStream_t s) {
    if (ntiles == 0 || nlist == 0) return;
    LAUNCH(build_scan_kernel, dim3((nlist + 255) / 256), dim3(256), 0, s, cnt, ntiles, nlist, running);
}

void launch_build_place(const BuildPlaceArgs& a, hipStream_t s) {
    if (a.ntiles == 0) return;
    if (a.dpad % 4 || a.d > a.dpad || a.ldx < (uint64_t)a.d) throw std::runtime_error("build_place: rows that are not stored in 16-byte pieces");
    if (a.dtype == 0) place_launch(a, static_cast<const float*>(a.x), s);
    else if (a.dtype == 1) place_launch(a, static_cast<const __half*>(a.x), s);
    else throw std::runtime_error("build_place: unknown dtype");
}

}  // namespace amdivf
