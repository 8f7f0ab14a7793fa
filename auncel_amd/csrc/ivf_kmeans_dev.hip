// Clustering::train with the training rows in HBM (amd_ivf_kmeans_dev): what amd_ivf_kmeans does on the host between
// two assignment passes -- the finite check, sub-sampling, the centroid install, grouping, the centroid update, void-cluster
// splitting, post-processing, the objective -- as kernels on one stream, each in the reference's order of operations.
//   set-up          finite_kernel (all n rows), sample_kernel (rows perm[i] -> the fp32 sample at stride dpad, its IntRange),
//                   rows_kernel (the seeds, or the corner nx == k)
//   an iteration    reset / install / normmax: the centroids into the handle's layout, their IntRange and norm bound
//                   (the assignment: coarse_dev)
//                   objective_kernel: the running fp32 sum of the distances in point order
//                   launch_build_keys / _offsets / _count / _scan (ivf_build.hip) and place_kernel: idx grouped by centroid, stable
//                   order_kernel + update_kernel: the means, long runs first
//                   split_kernel, post_kernel
// No workgroup waits for another; the order between the kernels is the stream's.  No float atomics, no sum reassociated.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ivf_dev.h"

namespace amdivf {

namespace {

constexpr uint32_t T = BUILD_TILE;
constexpr uint32_t SKIP = BUILD_SKIP;
constexpr uint32_t STAGE = 512;     // entries of a run's idx a workgroup of update_kernel holds in LDS at a time
constexpr int UNROLL = 8;           // row loads a thread of update_kernel keeps in flight
constexpr uint32_t POP_LDS = 8192;  // split_kernel: populations of up to this many clusters live in LDS
constexpr uint32_t OBJ_CHUNK = 4096;

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__half v) { return __half2float(v); }  // (exact: every fp16 value is an fp32 value)

// four consecutive elements of a row as fp32, by one load where the caller's layout allows it; only columns below d are read
__device__ __forceinline__ float4 load4(const float* p, uint32_t c, uint32_t d, int wide) {
    if (wide && c + 4 <= d) return *reinterpret_cast<const float4*>(p + c);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < 4; j++)
        if (c + j < d) v[j] = p[c + j];
    return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ float4 load4(const __half* p, uint32_t c, uint32_t d, int wide) {
    if (wide && c + 4 <= d) {
        const uint2 q = *reinterpret_cast<const uint2*>(p + c);
        const __half2 a = *reinterpret_cast<const __half2*>(&q.x), b = *reinterpret_cast<const __half2*>(&q.y);
        return make_float4(__low2float(a), __high2float(a), __low2float(b), __high2float(b));
    }
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < 4; j++)
        if (c + j < d) v[j] = __half2float(p[c + j]);
    return make_float4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ bool not_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// ---- set-up
// A lane per (row, group of four columns) of the caller's tensor, grid-strided: any NaN or infinity raises *flag.
template <class X>
__global__ __launch_bounds__(256) void finite_kernel(const X* __restrict__ x, uint64_t n, uint32_t d, uint64_t ldx, int wide, uint32_t* flag) {
    const uint32_t nsteps = (d + 3) >> 2;
    const uint64_t items = n * nsteps;
    bool bad = false;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < items; t += (uint64_t)gridDim.x * 256) {
        const uint64_t i = t / nsteps;
        const float4 v = load4(x + i * ldx, (uint32_t)(t - i * nsteps) * 4, d, wide);
        bad |= not_finite(v.x) | not_finite(v.y) | not_finite(v.z) | not_finite(v.w);
    }
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// Sample row i <- row perm[i] of the caller's tensor (perm null: row i), as fp32 at stride dpad with the padding written as zeros;
// the sample's IntRange rides on the loads (RangeWatch; a padding zero moves none of its three results).
template <class X>
__global__ __launch_bounds__(256) void sample_kernel(const X* __restrict__ x, uint64_t ldx, uint32_t d, uint32_t dpad, int wide,
                                                     const int* __restrict__ perm, uint64_t nx, float* __restrict__ out, uint32_t* range) {
    const uint32_t nsteps = dpad >> 2;
    const uint64_t items = nx * nsteps;
    RangeWatch watch;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < items; t += (uint64_t)gridDim.x * 256) {
        const uint64_t i = t / nsteps;
        const uint64_t row = perm ? (uint64_t)perm[i] : i;
        const float4 v = load4(x + row * ldx, (uint32_t)(t - i * nsteps) * 4, d, wide);
        reinterpret_cast<float4*>(out)[t] = v;
        watch.look(v);
    }
    watch.commit(range, threadIdx.x & 63);
}

// m compact rows of d floats: out row i <- row perm[i] (perm null: row i) of x.  The seeds (from the sample) and the corner nx == k
// (the caller's first k rows): k rows, once a call.
template <class X>
__global__ __launch_bounds__(256) void rows_kernel(const X* __restrict__ x, uint64_t ldx, uint32_t d, const int* __restrict__ perm, uint64_t m,
                                                   float* __restrict__ out) {
    const uint64_t items = m * d;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < items; t += (uint64_t)gridDim.x * 256) {
        const uint64_t i = t / d;
        const uint64_t row = perm ? (uint64_t)perm[i] : i;
        out[t] = to_f32(x[row * ldx + (t - i * d)]);
    }
}

// ---- the centroids into the handle's layout
// state: words 0..2 the centroids' range as RangeWatch commits it, 3 the call's error flags (kept), 4..5 the norm bound
__global__ __launch_bounds__(64) void reset_kernel(uint32_t* state, uint32_t* cinfo) {
    const uint32_t t = threadIdx.x;
    if (t < 3) state[t] = t == 0 ? 0u : fkey(0.f);
    if (t == 4 || t == 5) state[t] = 0u;
    if (t >= 8 && t < 12) cinfo[t - 8] = 0u;
}

// k x d compact -> k x dpad zero padded, and the range of the values
__global__ __launch_bounds__(256) void install_kernel(const float* __restrict__ cen, uint32_t k, uint32_t d, uint32_t dpad, float* __restrict__ out,
                                                      uint32_t* range) {
    const uint64_t items = (uint64_t)k * dpad;
    RangeWatch watch;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < items; t += (uint64_t)gridDim.x * 256) {
        const uint64_t i = t / dpad;
        const uint32_t j = (uint32_t)(t - i * dpad);
        const float v = j < d ? cen[i * d + j] : 0.f;
        out[t] = v;
        watch.look(v);
    }
    watch.commit(range, threadIdx.x & 63);
}

// max over the rows of the double sum of squares in element order (amd_ivf_set_centroids' loop; the padding adds +0).  Sums of
// squares are not negative, so their bit patterns order as integers do.
__global__ __launch_bounds__(256) void normmax_kernel(const float* __restrict__ c, uint32_t k, uint32_t dpad, unsigned long long* out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    double sq = 0;
    if (i < k) {
        const float4* row = reinterpret_cast<const float4*>(c + (uint64_t)i * dpad);
        for (uint32_t g = 0; g < dpad >> 2; g++) {
            const float4 v = row[g];
            sq += (double)v.x * (double)v.x;
            sq += (double)v.y * (double)v.y;
            sq += (double)v.z * (double)v.z;
            sq += (double)v.w * (double)v.w;
        }
    }
    unsigned long long key = (unsigned long long)__double_as_longlong(sq);
    for (int off = 32; off; off >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)key, off);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key != 0) atomicMax(out, key);
}

// ---- grouping: the last step of ivf_build.hip's counting sort with nothing to move but the point's number
__global__ __launch_bounds__(256) void place_kernel(const uint32_t* __restrict__ keys, const uint16_t* __restrict__ rank,
                                                    const uint32_t* __restrict__ before, const uint64_t* __restrict__ list_off, uint64_t n,
                                                    uint64_t row0, uint32_t nlist, uint32_t* __restrict__ idx_sorted, uint32_t* flags) {
    const uint32_t* my_before = before + (uint64_t)blockIdx.x * nlist;
    bool bad = false;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint32_t r = threadIdx.x + 256 * u;
        const uint64_t i = row0 + (uint64_t)blockIdx.x * T + r;
        if (i >= n) continue;
        const uint32_t key = keys[i];
        if (key == SKIP) {  // (an assignment outside [0, k): the point is in no run, the call is refused)
            bad = true;
            continue;
        }
        const uint64_t dst = list_off[key] + my_before[key] + rank[(uint64_t)blockIdx.x * T + r];
        if (dst < n) idx_sorted[dst] = (uint32_t)i;
        else bad = true;
    }
    if (bad) atomicOr(flags, 1u);
}

// ---- the update
// The centroids ordered by the length class of their runs, longest first (class = bit length of the run), so that update_kernel's
// grid starts its long chains first and ends on the short ones.  One workgroup; the order inside a class is whatever the LDS
// atomics give, which decides when a mean is computed, never what it is.
__global__ __launch_bounds__(256) void order_kernel(const uint64_t* __restrict__ list_off, uint32_t k, uint32_t* __restrict__ order) {
    __shared__ uint32_t s_at[33];
    const uint32_t t = threadIdx.x;
    if (t < 33) s_at[t] = 0;
    __syncthreads();
    for (uint32_t c = t; c < k; c += 256) {
        const uint32_t len = (uint32_t)(list_off[c + 1] - list_off[c]);
        atomicAdd(&s_at[len ? 32 - __clz(len) : 0], 1u);
    }
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int b = 32; b >= 0; b--) {
            const uint32_t c = s_at[b];
            s_at[b] = run;
            run += c;
        }
    }
    __syncthreads();
    for (uint32_t c = t; c < k; c += 256) {
        const uint32_t len = (uint32_t)(list_off[c + 1] - list_off[c]);
        order[atomicAdd(&s_at[len ? 32 - __clz(len) : 0], 1u)] = c;
    }
}

template <int VEC> __device__ __forceinline__ void loadv(const float* p, float (&v)[VEC]);
template <> __device__ __forceinline__ void loadv<1>(const float* p, float (&v)[1]) { v[0] = *p; }
template <> __device__ __forceinline__ void loadv<2>(const float* p, float (&v)[2]) {
    const float2 q = *reinterpret_cast<const float2*>(p);
    v[0] = q.x, v[1] = q.y;
}
template <> __device__ __forceinline__ void loadv<4>(const float* p, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
}

// A workgroup per (centroid, slab of blockDim.x * VEC columns).  A centroid's mean is the fp32 sum of its points in ascending point
// order divided by their count: the adds of one (centroid, column) are a chain, everything around them is not.  The workgroup stages
// its run of idx through LDS in coalesced pieces of STAGE entries; a thread owns VEC neighbouring columns (VEC chosen by the launch
// so that a wave's lanes cover the row: a wave reads 256 bytes of a row or more by one load each lane), requests the rows of the
// next UNROLL points before it adds the UNROLL it holds, and adds in order.  The row address depends on LDS only, not on a load from
// memory, so UNROLL loads are in flight while the chain advances.
template <int VEC>
__global__ __launch_bounds__(256) void update_kernel(const float* __restrict__ x, uint32_t dpad, uint32_t d, const uint32_t* __restrict__ idx,
                                                     const uint64_t* __restrict__ list_off, const uint32_t* __restrict__ order,
                                                     float* __restrict__ cen) {
    __shared__ uint32_t s_idx[STAGE];
    const uint32_t c = order[blockIdx.x];
    const uint64_t b = list_off[c], e = list_off[c + 1];
    const uint32_t col = (blockIdx.y * blockDim.x + threadIdx.x) * VEC;
    const bool active = col < dpad;
    const float* xc = x + col;
    float s[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) s[j] = 0.f;
    for (uint64_t p0 = b; p0 < e; p0 += STAGE) {
        const uint32_t m = e - p0 < (uint64_t)STAGE ? (uint32_t)(e - p0) : STAGE;
        __syncthreads();  // (the piece before this one has been read)
        for (uint32_t q = threadIdx.x; q < m; q += blockDim.x) s_idx[q] = idx[p0 + q];
        __syncthreads();
        if (!active) continue;
        const uint32_t full = m / UNROLL * UNROLL;
        float cur[UNROLL][VEC] = {}, nxt[UNROLL][VEC] = {};
        if (full) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) loadv<VEC>(xc + (uint64_t)s_idx[u] * dpad, cur[u]);
        }
        for (uint32_t q = 0; q < full; q += UNROLL) {
            if (q + UNROLL < full) {
#pragma unroll
                for (int u = 0; u < UNROLL; u++) loadv<VEC>(xc + (uint64_t)s_idx[q + UNROLL + u] * dpad, nxt[u]);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
#pragma unroll
                for (int j = 0; j < VEC; j++) {
                    s[j] += cur[u][j];
                    cur[u][j] = nxt[u][j];
                }
            }
        }
        for (uint32_t q = full; q < m; q++) {
            float v[VEC];
            loadv<VEC>(xc + (uint64_t)s_idx[q] * dpad, v);
#pragma unroll
            for (int j = 0; j < VEC; j++) s[j] += v[j];
        }
    }
    if (!active) return;
    const float ni = (float)(e - b);
#pragma unroll
    for (int j = 0; j < VEC; j++)
        if (col + j < d) cen[(uint64_t)c * d + col + j] = ni != 0 ? s[j] / ni : 0.f;
}

// ---- void clusters (kmeans_host.h: split_void_clusters is the specification)
__device__ __forceinline__ uint32_t mt_mix(uint32_t a, uint32_t b) {
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
// The next 624 words of std::mt19937, by the whole workgroup.  Word i takes word i + 397 (mod 624), which from i = 227 on is a word
// of the new generation, and words i and i + 1 of the old one (word 623: the new word 0): three passes of 227 words, each reading
// before any of it writes.
__device__ __forceinline__ void mt_twist(uint32_t* mt, uint32_t t) {
    for (uint32_t pass = 0; pass < 3; pass++) {
        const uint32_t i = pass * 227 + t;
        const bool mine = t < 227 && i < 624;
        uint32_t v = 0;
        if (mine) v = mt[i >= 227 ? i - 227 : i + 397] ^ mt_mix(mt[i], mt[i == 623 ? 0 : i + 1]);
        __syncthreads();
        if (mine) mt[i] = v;
        __syncthreads();
    }
}

// One workgroup.  The reference walks the clusters round-robin from 0 with one draw of a generator seeded 1234 per candidate donor
// and stops at the first draw below the candidate's share; the populations do not change during a walk, so draw j of the walk
// tests cluster j mod k whoever computes it: the workgroup tests up to 256 consecutive draws at once -- the generator's state in
// LDS, tempered by the lane that reads it, the share in double arithmetic rounded to float -- and takes the first that hits; the
// draws after it stay for the next walk.  Then populations are halved by one lane and the donor's row is copied and nudged
// (float *= double: one rounding) by all.  Leaves at once when no cluster is empty.  A population table that does not sum to n (an
// assignment outside [0, k), which the grouping has flagged) would let a walk run for ever: it raises the flag instead.
__global__ __launch_bounds__(256) void split_kernel(float* __restrict__ cen, const unsigned long long* __restrict__ total, uint32_t k, uint32_t d,
                                                    uint64_t n, uint32_t* __restrict__ pop_global, uint32_t* flags) {
    __shared__ uint32_t s_mt[624];
    __shared__ uint32_t s_pop[POP_LDS];
    __shared__ unsigned long long s_sum;
    __shared__ uint32_t s_first;
    uint32_t* pop = k <= POP_LDS ? s_pop : pop_global;
    const uint32_t t = threadIdx.x;
    if (t == 0) s_sum = 0;
    __syncthreads();
    int zero = 0;
    unsigned long long sum = 0;
    for (uint32_t c = t; c < k; c += 256) {
        const unsigned long long v = total[c];
        pop[c] = (uint32_t)v;
        zero |= v == 0;
        sum += v;
    }
    atomicAdd(&s_sum, sum);
    if (!__syncthreads_or(zero)) return;
    if (s_sum != n || n <= k) {
        if (t == 0) atomicOr(flags, 1u);
        return;
    }
    if (t == 0) {
        s_mt[0] = 1234u;
        for (uint32_t i = 1; i < 624; i++) s_mt[i] = 1812433253u * (s_mt[i - 1] ^ (s_mt[i - 1] >> 30)) + i;
    }
    __syncthreads();
    const double nudge = 1.0 / 1024.0;
    const float denom = (float)(n - k);
    uint32_t mti = 624, next = 0;  // (the same in every thread)
    for (;;) {
        while (next < k && pop[next] != 0) next++;
        if (next >= k) return;
        uint32_t cand = 0, donor = 0;
        for (;;) {
            if (mti == 624) {
                mt_twist(s_mt, t);
                mti = 0;
            }
            const uint32_t m = 624 - mti < 256u ? 624 - mti : 256u;
            bool hit = false;
            if (t < m) {
                const float share = (float)(((double)pop[(cand + t) % k] - 1.0) / (double)denom);
                uint32_t y = s_mt[mti + t];
                y ^= y >> 11;
                y ^= (y << 7) & 0x9d2c5680u;
                y ^= (y << 15) & 0xefc60000u;
                y ^= y >> 18;
                hit = (float)y / 4294967296.f < share;  // (mt() / float(mt.max()): 2^32 - 1 rounds to 2^32)
            }
            __syncthreads();  // (the round before has read s_first)
            if (t == 0) s_first = 0xffffffffu;
            __syncthreads();
            if (hit) atomicMin(&s_first, t);
            __syncthreads();
            const uint32_t first = s_first;
            if (first != 0xffffffffu) {
                donor = (cand + first) % k;
                mti += first + 1;
                break;
            }
            mti += m;
            cand = (cand + m) % k;
        }
        if (t == 0) {  // (every lane's reads of the populations lie before the walk's last barrier)
            const uint32_t half = pop[donor] / 2;
            pop[next] = half;
            pop[donor] -= half;
        }
        for (uint32_t j = t; j < d; j += 256) {
            const bool even = (j & 1) == 0;
            const float v = cen[(uint64_t)donor * d + j];
            cen[(uint64_t)next * d + j] = (float)((double)v * (even ? 1 + nudge : 1 - nudge));
            cen[(uint64_t)donor * d + j] = (float)((double)v * (even ? 1 - nudge : 1 + nudge));
        }
        __syncthreads();  // (the populations and the rows as the next walk finds them)
        next++;
    }
}

// ---- post-processing (kmeans_host.h: post_process): a wave per centroid.  Spherical: the norm in the reference's 4-lane SSE order
// -- lane l of the first four sums the squares of elements l, l + 4, ... in order, then (s0 + s1) + (s2 + s3) -- from the row staged
// through LDS; inv = (float)(1.0 / sqrtf(nr)) with the division in double; then roundf for int_centroids.
__global__ __launch_bounds__(64) void post_kernel(float* __restrict__ cen, uint32_t d, int spherical, int int_centroids) {
    __shared__ float s_row[1024];
    float* row = cen + (uint64_t)blockIdx.x * d;
    const uint32_t lane = threadIdx.x;
    float inv = 1.f;
    bool scale = false;
    if (spherical) {
        float s = 0.f;
        for (uint32_t c0 = 0; c0 < d; c0 += 1024) {
            const uint32_t m = d - c0 < 1024u ? d - c0 : 1024u;
            __syncthreads();
            for (uint32_t j = lane; j < m; j += 64) s_row[j] = row[c0 + j];
            __syncthreads();
            if (lane < 4)
                for (uint32_t j = lane; j < m; j += 4) {
                    const float v = s_row[j];
                    s += v * v;
                }
        }
        const float s0 = __shfl(s, 0), s1 = __shfl(s, 1), s2 = __shfl(s, 2), s3 = __shfl(s, 3);
        const float nr = (s0 + s1) + (s2 + s3);
        if (nr > 0) {
            inv = (float)(1.0 / (double)sqrtf(nr));
            scale = true;
        }
    }
    for (uint32_t j = lane; j < d; j += 64) {
        float v = row[j];
        if (scale) v *= inv;
        if (int_centroids) v = roundf(v);
        row[j] = v;
    }
}

// ---- the objective: the reference's running fp32 sum of the distances in point order.  One workgroup: waves 1..3 stage the next
// OBJ_CHUNK distances into one half of LDS while lane 0 adds the other half in order, four values an LDS read.
__global__ __launch_bounds__(256) void objective_kernel(const float* __restrict__ dis, uint64_t n, float* out) {
    __shared__ __attribute__((aligned(16))) float s_d[2][OBJ_CHUNK];
    const uint32_t t = threadIdx.x;
    const uint64_t nchunks = (n + OBJ_CHUNK - 1) / OBJ_CHUNK;
    float err = 0.f;
    for (uint32_t j = t; j < OBJ_CHUNK && j < n; j += 256) s_d[0][j] = dis[j];
    for (uint64_t ci = 0; ci < nchunks; ci++) {
        __syncthreads();  // (chunk ci is staged; the other half has been added)
        const uint64_t at = (ci + 1) * OBJ_CHUNK;
        if (t >= 64)
            for (uint32_t j = t - 64; j < OBJ_CHUNK && at + j < n; j += 192) s_d[(ci + 1) & 1][j] = dis[at + j];
        if (t == 0) {
            const float* cur = s_d[ci & 1];
            const uint64_t left = n - ci * OBJ_CHUNK;
            const uint32_t m = left < (uint64_t)OBJ_CHUNK ? (uint32_t)left : OBJ_CHUNK;
            uint32_t j = 0;
            // blocks of 32 values in two register sets: a block's eight LDS reads are requested before the block ahead of it is
            // added, and no value moves between registers (v holds block j whenever j + 32 <= m)
            float4 v[8] = {}, w[8] = {};
            auto fetch = [&](float4(&r)[8], uint32_t at) {
#pragma unroll
                for (int u = 0; u < 8; u++) r[u] = *reinterpret_cast<const float4*>(cur + at + 4 * u);
            };
            auto add = [&](const float4(&r)[8]) {
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    err += r[u].x;
                    err += r[u].y;
                    err += r[u].z;
                    err += r[u].w;
                }
            };
            if (m >= 32) fetch(v, 0);
            for (; j + 64 <= m; j += 64) {
                fetch(w, j + 32);
                add(v);
                if (j + 96 <= m) fetch(v, j + 64);
                add(w);
            }
            if (j + 32 <= m) {
                add(v);
                j += 32;
            }
            for (; j + 4 <= m; j += 4) {
                const float4 q = *reinterpret_cast<const float4*>(cur + j);
                err += q.x;
                err += q.y;
                err += q.z;
                err += q.w;
            }
            for (; j < m; j++) err += cur[j];
        }
    }
    if (t == 0) *out = err;
}

uint32_t stride_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 1u << 16); }

template <class X> int wide_rows(const X* x, uint64_t ldx) { return reinterpret_cast<uintptr_t>(x) % (4 * sizeof(X)) == 0 && ldx % 4 == 0; }

template <int VEC>
void update_launch(const float* x, uint32_t dpad, uint32_t d, const uint32_t* idx, const uint64_t* list_off, const uint32_t* order, uint32_t k,
                   float* cen, hipStream_t s) {
    const uint32_t lanes = (dpad + VEC - 1) / VEC;                        // threads that cover a row
    const uint32_t block = std::min<uint32_t>((lanes + 63) / 64 * 64, 256);
    LAUNCH(update_kernel<VEC>, dim3(k, (lanes + block - 1) / block), dim3(block), 0, s, x, dpad, d, idx, list_off, order, cen);
}

}  // namespace

void launch_kmeans_dev_finite(const void* x, int dtype, uint64_t n, int d, uint64_t ldx, uint32_t* flag, hipStream_t s) {
    if (n == 0) return;
    const uint32_t grid = stride_grid(n * (uint64_t)((d + 3) / 4));
    if (dtype == 0) {
        const float* p = static_cast<const float*>(x);
        LAUNCH(finite_kernel<float>, dim3(grid), dim3(256), 0, s, p, n, (uint32_t)d, ldx, wide_rows(p, ldx), flag);
    } else if (dtype == 1) {
        const __half* p = static_cast<const __half*>(x);
        LAUNCH(finite_kernel<__half>, dim3(grid), dim3(256), 0, s, p, n, (uint32_t)d, ldx, wide_rows(p, ldx), flag);
    } else {
        throw std::runtime_error("kmeans_dev: unknown dtype");
    }
}

void launch_kmeans_dev_sample(const void* x, int dtype, uint64_t ldx, int d, int dpad, const int* perm, uint64_t nx, float* out, uint32_t* range,
                              hipStream_t s) {
    if (nx == 0) return;
    if (dpad % 4 || d > dpad || ldx < (uint64_t)d) throw std::runtime_error("kmeans_dev: rows that are not stored in 16-byte pieces");
    const uint32_t grid = stride_grid(nx * (uint64_t)(dpad / 4));
    if (dtype == 0) {
        const float* p = static_cast<const float*>(x);
        LAUNCH(sample_kernel<float>, dim3(grid), dim3(256), 0, s, p, ldx, (uint32_t)d, (uint32_t)dpad, wide_rows(p, ldx), perm, nx, out, range);
    } else if (dtype == 1) {
        const __half* p = static_cast<const __half*>(x);
        LAUNCH(sample_kernel<__half>, dim3(grid), dim3(256), 0, s, p, ldx, (uint32_t)d, (uint32_t)dpad, wide_rows(p, ldx), perm, nx, out, range);
    } else {
        throw std::runtime_error("kmeans_dev: unknown dtype");
    }
}

void launch_kmeans_dev_rows(const void* x, int dtype, uint64_t ldx, int d, const int* perm, uint64_t m, float* out, hipStream_t s) {
    if (m == 0) return;
    const uint32_t grid = stride_grid(m * (uint64_t)d);
    if (dtype == 0) LAUNCH(rows_kernel<float>, dim3(grid), dim3(256), 0, s, static_cast<const float*>(x), ldx, (uint32_t)d, perm, m, out);
    else if (dtype == 1) LAUNCH(rows_kernel<__half>, dim3(grid), dim3(256), 0, s, static_cast<const __half*>(x), ldx, (uint32_t)d, perm, m, out);
    else throw std::runtime_error("kmeans_dev: unknown dtype");
}

void launch_kmeans_dev_install(const float* cen, uint32_t k, int d, int dpad, float* out, uint32_t* state, uint32_t* cinfo, hipStream_t s) {
    LAUNCH(reset_kernel, dim3(1), dim3(64), 0, s, state, cinfo);
    LAUNCH(install_kernel, dim3(stride_grid((uint64_t)k * dpad)), dim3(256), 0, s, cen, k, (uint32_t)d, (uint32_t)dpad, out, state);
    LAUNCH(normmax_kernel, dim3((k + 255) / 256), dim3(256), 0, s, out, k, (uint32_t)dpad, reinterpret_cast<unsigned long long*>(state + 4));
}

void launch_kmeans_dev_place(const uint32_t* keys, const uint16_t* rank, const uint32_t* before, const uint64_t* list_off, uint64_t n, uint64_t row0,
                             uint32_t ntiles, uint32_t nlist, uint32_t* idx_sorted, uint32_t* flags, hipStream_t s) {
    if (ntiles == 0) return;
    LAUNCH(place_kernel, dim3(ntiles), dim3(256), 0, s, keys, rank, before, list_off, n, row0, nlist, idx_sorted, flags);
}

void launch_kmeans_dev_update(const float* x, int dpad, int d, const uint32_t* idx_sorted, const uint64_t* list_off, uint32_t k, uint32_t* order,
                              float* cen, hipStream_t s) {
    LAUNCH(order_kernel, dim3(1), dim3(256), 0, s, list_off, k, order);
    // the columns a lane owns: as few as fill a wave with the row, so that short rows still keep every lane loading
    if (dpad <= 64) update_launch<1>(x, (uint32_t)dpad, (uint32_t)d, idx_sorted, list_off, order, k, cen, s);
    else if (dpad <= 128) update_launch<2>(x, (uint32_t)dpad, (uint32_t)d, idx_sorted, list_off, order, k, cen, s);
    else update_launch<4>(x, (uint32_t)dpad, (uint32_t)d, idx_sorted, list_off, order, k, cen, s);
}

void launch_kmeans_dev_split(float* cen, const unsigned long long* total, uint32_t k, int d, uint64_t n, uint32_t* pop, uint32_t* flags,
                             hipStream_t s) {
    LAUNCH(split_kernel, dim3(1), dim3(256), 0, s, cen, total, k, (uint32_t)d, n, pop, flags);
}

void launch_kmeans_dev_post(float* cen, uint32_t k, int d, int spherical, int int_centroids, hipStream_t s) {
    if (!spherical && !int_centroids) return;
    LAUNCH(post_kernel, dim3(k), dim3(64), 0, s, cen, (uint32_t)d, spherical, int_centroids);
}

void launch_kmeans_dev_objective(const float* dis, uint64_t n, float* out, hipStream_t s) {
    LAUNCH(objective_kernel, dim3(1), dim3(256), 0, s, dis, n, out);
}

}  // namespace amdivf
