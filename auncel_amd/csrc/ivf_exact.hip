// Exact k-NN over the whole index (amd_ivf_search_exact): every query probes every list, so nothing is planned -- the
// byte fragments of all lists are ONE stream of 32-vector blocks, a workgroup owns a tile of up to 256 queries and a slab of
// consecutive blocks, and a block that has been fetched is contracted with every query block of the tile before it is let go.
//   scan_all_kernel      the list pass: emits, per query, every stored entry at or within the query's threshold (the k-th distance of
//                        a seed search of the same lists) as (global position, distance)
//   exact_select_kernel  a wave per query: the candidates in (distance, position) order; the result is read off them when no two
//                        neighbours of the best k + 1 are equal (exact_args.h: exact_window_tied), else the query is flagged and
//                        the caller searches it the general way
// The arithmetic is scan_mfma_pair_kernel's (ivf_kernels.hip): v_mfma_i32_32x32x32_i8 on re-centred bytes, the threshold folded into
// the accumulators' start values, a v_max3 pre-test in front of the epilogue.  Every distance is the same exact integer.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "exact_args.h"
#include "ivf_dev.h"

namespace amdivf {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// per 32-vector block of the fragment copy: (global position of its first slot, slots that hold an entry).  A list is padded to an
// even number of blocks: the block in which a list ends holds fewer than 32 entries, the padding block behind it none.
__global__ __launch_bounds__(256) void exact_blocks_kernel(const uint64_t* __restrict__ list_off, const uint64_t* __restrict__ block_off,
                                                           uint32_t nlist, uint64_t nblk, uint2* __restrict__ out) {
    const uint64_t blk = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (blk >= nblk) return;
    uint32_t lo = 0, hi = nlist;  // largest l with block_off[l] <= blk
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (block_off[mid] <= blk) lo = mid;
        else hi = mid;
    }
    const uint64_t p = (blk - block_off[lo]) * 32, size = list_off[lo + 1] - list_off[lo];
    const uint64_t left = p < size ? size - p : 0;
    out[blk] = make_uint2((uint32_t)(list_off[lo] + p), (uint32_t)(left < 32 ? left : 32));
}

// keys[i][l] = l: the ranking under which the general way visits every list in list-number order
__global__ __launch_bounds__(256) void identity_keys_kernel(int64_t* __restrict__ keys, uint64_t total, uint32_t nlist) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) keys[i] = (int64_t)(i % nlist);
}

// The list pass.  Grid: (slabs of the block stream, tiles of 256 queries).  Wave w of a workgroup holds the A operands of query
// blocks 2 w and 2 w + 1 of the tile in registers for the whole slab; the four waves request the same list block, which reaches
// the compute unit once (the later requests are served by its vector cache) and is contracted with all eight query blocks.  No
// workgroup barrier anywhere: a wave whose query blocks do not exist leaves at once.
// A candidate of query q is an entry with dis <= T[q] (L2) / dis >= T[q] (IP), T = the seed's k-th distance: the EQUALITY is wanted,
// it is how a tie at the k-th is seen.  The pre-test is the pair kernel's strict one against T + 1 (L2: made even, so loosened by at
// most one more) / T - 1 (IP); a register that passes it recomputes the distance and tests it exactly.  Slots behind a list's end
// (ExactScanArgs::blk says how many of a block's 32 are entries) never pass: their bound is INT_MAX.
template <int METRIC, int NKS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) void scan_all_kernel(ExactScanArgs a) {
    static_assert(NKS >= 1 && NKS <= 4, "query operands resident in registers");
    __shared__ int s_init[4][64];
    __shared__ int s_cx[4][64];
    __shared__ int s_u[4][64];
    __shared__ int s_T[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 31, h = lane >> 5;
    constexpr size_t qstride = (size_t)NKS * 32;
    constexpr size_t block_bytes = (size_t)NKS * 1024;
    const uint32_t qbase = blockIdx.y * 256u + (uint32_t)wave * 64u;
    if (qbase >= a.n) return;
    const uint32_t nq = a.n - qbase < 64u ? a.n - qbase : 64u;  // query slots of this wave that hold a query
    const bool two = nq > 32;                                  // (wave-uniform)
    const uint64_t B0 = (uint64_t)blockIdx.x * a.slab;
    const uint64_t B1 = B0 + a.slab < a.nblk ? B0 + a.slab : a.nblk;  // (slab and nblk are even)
    if (B0 >= B1) return;

    // ---- per query slot (slot = lane): threshold and start value
    {
        const bool sok = (uint32_t)lane < nq;
        const uint32_t q = qbase + (sok ? (uint32_t)lane : 0u);
        const int cx = a.query_cx[q];
        const size_t last = (size_t)q * a.k + (a.k - 1);
        const float tau = a.seed_D[last];
        const bool have = sok && a.seed_I[last] >= 0 && tau == tau && fabsf(tau) <= 1073741824.f;
        int T = METRIC == METRIC_L2 ? -1 : 0x7fffffff, u = 0, init = -1073741824;  // (no threshold: nothing passes either test)
        if (have) {
            if (METRIC == METRIC_L2) {
                T = (int)floorf(tau);          // dis <= tau <=> dis <= floor(tau) <=> dis < T + 1
                u = (cx - (T + 1)) & ~1;       // keep <=> 2 x.y - |y|^2 > |x|^2 - (T + 1) >= u
                init = -(u >> 1);
            } else {
                T = (int)ceilf(tau);           // dis >= tau <=> dis >= ceil(tau) <=> dis > T - 1
                u = (T - 1) - cx;              // keep <=> x.y + cy > (T - 1) - cx
                init = -u;
            }
        }
        s_init[wave][lane] = init;
        s_cx[wave][lane] = cx;
        s_u[wave][lane] = u;
        s_T[wave][lane] = T;
    }
    // ---- the A operands: lane (m, h) of query block g holds the bytes of query slot 32 g + m
    v4i af0[NKS], af1[NKS];
    {
        const bool qok0 = (uint32_t)m < nq, qok1 = (uint32_t)(32 + m) < nq;
        const int8_t* q0p = a.queries8 + (size_t)(qbase + (qok0 ? (uint32_t)m : 0u)) * qstride + (size_t)h * (size_t)(16 * NKS);
        const int8_t* q1p = a.queries8 + (size_t)(qbase + (qok1 ? 32u + (uint32_t)m : 0u)) * qstride + (size_t)h * (size_t)(16 * NKS);
#pragma unroll
        for (int s = 0; s < NKS; s++) af0[s] = qok0 ? *reinterpret_cast<const v4i*>(q0p + 16 * s) : v4i{0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < NKS; s++) af1[s] = qok1 ? *reinterpret_cast<const v4i*>(q1p + 16 * s) : v4i{0, 0, 0, 0};
    }
    wave_sync();

    // ---- the block stream: two blocks in flight per wave, block i + 2 requested right behind the MFMAs of block i
    v4i b0[NKS], b1[NKS];
    int cy0 = 0, cy1 = 0;
    uint2 bi0 = make_uint2(0, 0), bi1 = make_uint2(0, 0);
    auto fetch = [&](v4i (&b)[NKS], int& cy, uint2& bi, uint64_t blk) {
        const uint8_t* bp = a.codes_frag + blk * block_bytes + (size_t)lane * 16;
#pragma unroll
        for (int s = 0; s < NKS; s++) b[s] = *reinterpret_cast<const v4i*>(bp + (size_t)s * 1024);
        cy = a.code_cy[blk * 32 + m];
        bi = a.blk[blk];
    };
    fetch(b0, cy0, bi0, B0);
    fetch(b1, cy1, bi1, B0 + 1);

    auto step = [&](v4i (&b)[NKS], int& cyv, uint2& biv, uint64_t i) {
        __builtin_amdgcn_sched_barrier(0);
        // register 4 g + c of lane half h belongs to query 8 g + 4 h + c of its block: the start values, LDS -> accumulator
        v16i acc0, acc1;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const v4i t0 = *reinterpret_cast<const v4i*>(&s_init[wave][8 * g + 4 * h]);
            const v4i t1 = *reinterpret_cast<const v4i*>(&s_init[wave][32 + 8 * g + 4 * h]);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                acc0[4 * g + c] = t0[c];
                acc1[4 * g + c] = t1[c];
            }
        }
#pragma unroll
        for (int s = 0; s < NKS; s++) acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af0[s], b[s], acc0, 0, 0, 0);
        if (two) {
#pragma unroll
            for (int s = 0; s < NKS; s++) acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af1[s], b[s], acc1, 0, 0, 0);
        }
        // what the epilogue needs of the block's constants is taken before their registers are requested again
        const bool vok = (uint32_t)m < biv.y;  // (a slot behind the list's end emits nothing)
        int hc = !vok ? 0x7fffffff : METRIC == METRIC_L2 ? cyv >> 1 : -cyv;
        uint32_t pos = biv.x + (uint32_t)m;
        int cy;
        asm volatile("v_mov_b32 %0, %1" : "=v"(cy) : "v"(cyv));
        asm volatile("" : "+v"(hc), "+v"(pos));
        __builtin_amdgcn_sched_barrier(0);
        fetch(b, cyv, biv, i + 2 < B1 ? i + 2 : i);  // (past the slab's end: its own block again, never used)
        __builtin_amdgcn_sched_barrier(0);
        auto epilogue = [&](const v16i& acc, auto QB) {
            constexpr int qb = decltype(QB)::value;
            static_for(std::make_integer_sequence<int, 2>{}, [&](auto H) {
                constexpr int r0 = decltype(H)::value * 8;
                // eight registers at a time: their largest value against the bound first (v_max3): most groups hold no candidate
                int mx = max(max(acc[r0], acc[r0 + 1]), acc[r0 + 2]);
                mx = max(max(mx, acc[r0 + 3]), acc[r0 + 4]);
                mx = max(max(mx, acc[r0 + 5]), acc[r0 + 6]);
                mx = max(mx, acc[r0 + 7]);
                if (__ballot(mx > hc) == 0) return;
                static_for(std::make_integer_sequence<int, 8>{}, [&](auto R) {
                    constexpr int reg = r0 + decltype(R)::value;
                    constexpr int q0 = qb + (reg & 3) + 8 * (reg >> 2);  // query slot of lane half 0; half 1: q0 + 4
                    if (acc[reg] > hc) {
                        const int sl = q0 + 4 * h;
                        const int cq = s_cx[wave][sl], uq = s_u[wave][sl], Tq = s_T[wave][sl];
                        // the contraction itself: acc = x.y - floor(u / 2) (L2) | x.y - u (IP)
                        const int t = METRIC == METRIC_L2 ? 2 * (acc[reg] + (uq >> 1)) - cy : acc[reg] + uq + cy;
                        const int dis = METRIC == METRIC_L2 ? cq - t : cq + t;
                        const bool keep = (uint32_t)sl < nq && (METRIC == METRIC_L2 ? dis <= Tq : dis >= Tq);
                        if (keep) {
                            const uint32_t q = qbase + (uint32_t)sl;
                            const uint32_t slot = atomicAdd(&a.cnt[q], 1u);  // (beyond cap only the counter moves)
                            if (slot < a.cap) a.cand[(size_t)q * a.cap + slot] = make_uint2(pos, __float_as_uint((float)dis));
                        }
                    }
                });
            });
        };
        epilogue(acc0, std::integral_constant<int, 0>{});
        if (two) epilogue(acc1, std::integral_constant<int, 32>{});
    };
    for (uint64_t i = B0; i < B1; i += 2) {
        step(b0, cy0, bi0, i);
        step(b1, cy1, bi1, i + 1);
    }
}

// A wave per query: its candidates sorted by (distance, global position) in LDS (a bitonic network over the next power of two), then
// the tie rule.  flag[q]: 0 the result was written, 1 equal distances met in the window, 2 anything else (no threshold: the seed's
// result was not full; more candidates than slots).  totals: [0..2] queries by flag, [3] candidates emitted.
__global__ __launch_bounds__(64) void exact_select_kernel(ExactSelectArgs a) {
    extern __shared__ unsigned long long s_key[];
    const uint32_t q = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t cnt = a.cnt[q], k = a.k;
    const bool have = a.seed_I[(size_t)q * k + (k - 1)] >= 0;
    uint32_t flag = (!have || cnt > a.cap || cnt < k) ? 2u : 0u;  // (wave-uniform)
    if (!flag) {
        uint32_t P = 2;
        while (P < cnt) P <<= 1;
        for (uint32_t i = lane; i < P; i += 64) {
            unsigned long long key = ~0ull;
            if (i < cnt) {
                const uint2 c = a.cand[(size_t)q * a.cap + i];
                const uint32_t fk = fkey(__uint_as_float(c.y));
                key = exact_key(a.metric == METRIC_L2 ? fk : ~fk, c.x);
            }
            s_key[i] = key;
        }
        for (uint32_t kk = 2; kk <= P; kk <<= 1)
            for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                __syncthreads();
                for (uint32_t i = lane; i < P; i += 64) {
                    const uint32_t l = i ^ j;
                    if (l > i) {
                        const unsigned long long x = s_key[i], y = s_key[l];
                        if ((x > y) == ((i & kk) == 0)) {
                            s_key[i] = y;
                            s_key[l] = x;
                        }
                    }
                }
            }
        __syncthreads();
        const bool tied = exact_window_tied(reinterpret_cast<const uint64_t*>(s_key), cnt, k, lane, 64);
        if (__ballot(tied)) {
            flag = 1;
        } else {
            for (uint32_t j = lane; j < k; j += 64) {
                const unsigned long long key = s_key[j];
                const uint32_t fk = (uint32_t)(key >> 32);
                a.D[(size_t)q * k + j] = fkey_inv(a.metric == METRIC_L2 ? fk : ~fk);
                a.I[(size_t)q * k + j] = a.ids[(uint32_t)key];
            }
        }
    }
    if (lane == 0) {
        a.flag[q] = flag;
        atomicAdd(&a.totals[flag], 1ull);
        atomicAdd(&a.totals[3], (unsigned long long)cnt);
    }
}

}  // namespace

void launch_exact_blocks(const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, uint64_t nblk, uint2* out, hipStream_t s) {
    if (nblk == 0) return;
    LAUNCH(exact_blocks_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, s, list_off, block_off, nlist, nblk, out);
}

void launch_identity_keys(int64_t* keys, size_t rows, uint32_t nlist, hipStream_t s) {
    const uint64_t total = (uint64_t)rows * nlist;
    if (total == 0) return;
    LAUNCH(identity_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, keys, total, nlist);
}

uint32_t exact_slab_blocks(uint64_t nblk, uint32_t n) {
    // about 2048 workgroups in all (eight per compute unit), a slab never shorter than 8 blocks; an even number of blocks
    const uint64_t tiles = ((uint64_t)n + 255) / 256;
    const uint64_t slabs = std::max<uint64_t>(1, 2048 / std::max<uint64_t>(tiles, 1));
    uint64_t slab = (nblk + slabs - 1) / slabs;
    slab = std::max<uint64_t>(8, (slab + 1) & ~(uint64_t)1);
    return (uint32_t)std::min<uint64_t>(slab, 1u << 30);
}

void launch_scan_all(const ExactScanArgs& a, hipStream_t s) {
    if (a.n == 0 || a.nblk == 0) return;
    const int ks = (int)mfma_ksteps(a.d);
    if (ks < 1 || ks > 4 || a.slab == 0 || (a.slab & 1) || (a.nblk & 1)) throw std::runtime_error("scan_all_kernel: shape not supported");
    const dim3 grid((unsigned)((a.nblk + a.slab - 1) / a.slab), (unsigned)((a.n + 255) / 256)), block(256);
    auto go = [&](auto kern) { LAUNCH(kern, grid, block, 0, s, a); };
    if (a.metric == METRIC_L2) {
        switch (ks) {
            case 1: return go(scan_all_kernel<METRIC_L2, 1>);
            case 2: return go(scan_all_kernel<METRIC_L2, 2>);
            case 3: return go(scan_all_kernel<METRIC_L2, 3>);
            default: return go(scan_all_kernel<METRIC_L2, 4>);
        }
    }
    switch (ks) {
        case 1: return go(scan_all_kernel<METRIC_IP, 1>);
        case 2: return go(scan_all_kernel<METRIC_IP, 2>);
        case 3: return go(scan_all_kernel<METRIC_IP, 3>);
        default: return go(scan_all_kernel<METRIC_IP, 4>);
    }
}

void launch_exact_select(const ExactSelectArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    uint32_t P = 2;
    while (P < a.cap) P <<= 1;
    LAUNCH(exact_select_kernel, dim3(a.n), dim3(64), (size_t)P * 8, s, a);
}

}  // namespace amdivf
