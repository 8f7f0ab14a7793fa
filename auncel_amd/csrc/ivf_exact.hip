// Exact k-NN over the whole index (amd_ivf_search_exact): every query probes every list, so nothing is planned -- the
// byte fragments of all lists are ONE stream of 32-vector blocks, a workgroup owns a tile of up to 256 queries and a slab of
// consecutive blocks, and a block that has been fetched is contracted with every query block of the tile before it is let go.
//   scan_all_kernel      the list pass: emits, per query, every stored entry at or within the query's threshold (the k-th distance of
//                        a seed search of the same lists) as (global position, distance)
//   scan_all_wide_i8_kernel  the same pass for byte lists of 128 < d <= 1024 (option "exact_wide_bytes"): the query operand through LDS
//   exact_blocks_kernel  the block table the pass reads; <KEEP>, of a call under an id selector: the mask of a block's slots that hold a
//                        MEMBER, so the same pass (KEEP) emits members only with nothing added to its loop
//   exact_select_kernel  a wave per query: the candidates in (distance, position) order; the result is read off them when no two
//                        neighbours of the best k + 1 are equal (exact_args.h: exact_window_tied), else the query is flagged and
//                        the caller searches it the general way
//   exact_range_collect_kernel / exact_range_fill_kernel  the exact range search (amd_ivf_range_search_exact): the same
//                        passes with the radius as every query's threshold; a query's candidates tested strictly against the radius,
//                        sorted by global position -- the reference's order -- and written out as (id, distance) runs
// The arithmetic is scan_mfma_pair_kernel's (ivf_kernels.hip): v_mfma_i32_32x32x32_i8 on re-centred bytes, the threshold folded into
// the accumulators' start values, a v_max3 pre-test in front of the epilogue.  Every distance is the same exact integer.
// What two passes share exists once: exact_i8_slot / exact_i8_emit (a query slot's constants, the epilogue of an accumulator tile)
// for the two byte passes, exact_f16_slot / exact_f16_emit for the two fp16 passes, the workgroup
// tile of both wide passes in mfma_tile.h, and launch_exact_wide.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "exact_args.h"
#include "mfma_tile.h"

namespace amdivf {

namespace {

// per 32-vector block of the fragment copy: (global position of its first slot, slots that hold an entry).  A list is padded to an
// even number of blocks: the block in which a list ends holds fewer than 32 entries, the padding block behind it none.
// KEEP, the table of a call under a selector: (global position of the block's first slot, VALID MASK) -- bit m is set iff slot m holds
// an entry and the selector keeps it (exact_args.h: exact_block_valid_mask).  keep: the selector's words, a bit per slot of the padded
// layout, so block b's 32 bits are half b & 1 of word b >> 1.  The list pass reads the mask where it read the count: a non-member is
// a slot behind the list's end to it, and nothing is added to its loop.
template <bool KEEP>
__global__ __launch_bounds__(256) void exact_blocks_kernel(const uint64_t* __restrict__ list_off, const uint64_t* __restrict__ block_off,
                                                           uint32_t nlist, uint64_t nblk, uint2* __restrict__ out,
                                                           const unsigned long long* __restrict__ keep) {
    const uint64_t blk = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (blk >= nblk) return;
    const uint32_t lo = list_of_block(block_off, nlist, blk);
    const uint64_t p = (blk - block_off[lo]) * 32, size = list_off[lo + 1] - list_off[lo];
    const uint64_t left = p < size ? size - p : 0;
    const uint32_t y = KEEP ? exact_block_valid_mask(left, exact_block_keep_half(keep[blk >> 1], blk)) : (uint32_t)(left < 32 ? left : 32);
    out[blk] = make_uint2((uint32_t)(list_off[lo] + p), y);
}

// keys[i][l] = l: the ranking under which the general way visits every list in list-number order
__global__ __launch_bounds__(256) void identity_keys_kernel(int64_t* __restrict__ keys, uint64_t total, uint32_t nlist) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) keys[i] = (int64_t)(i % nlist);
}

// What the two byte list passes below share: a query slot's constants and the epilogue of an accumulator tile.
// Every partial sum stays within int32.  A re-centred byte is in [-128, 127], so a product is at most 2^14 in magnitude and a dot
// product over d <= 1024 dimensions, complete or partial, at most 2^24.  The start value is -(u >> 1) (L2) or -u (IP) with
// u = cx - (T + 1) or (T - 1) - cx, |T| <= 2^30 and |cx| <= 2^24 (L2: a sum of d squares) or < 2^25 (IP: 128 sum - 16384 d), so it is
// below 2^30 + 2^25 + 2 in magnitude -- the value of a slot without a threshold is -2^30 --, and start value + partial sum below
// 2^30 + 2^25 + 2^24 + 2 < 2^31.  The epilogue undoes the start value first: acc + (u >> 1) / acc + u is x.y itself, and the
// distance is the byte scans' integer, at most 2^24 under the byte rule d m^2 <= 2^24.
// A query slot's threshold T, what the pre-test compares with (u) and the accumulators' start value (ok false: no query in the slot,
// then q is any valid query).  No full seed result, a NaN or a threshold beyond 2^30 in magnitude: nothing passes either test.
// Returns (init, cx, u, T).
template <int METRIC> __device__ __forceinline__ int4 exact_i8_slot(const ExactScanArgs& a, uint32_t q, bool ok) {
    const int cx = a.query_cx[q];
    const size_t last = (size_t)q * a.k + (a.k - 1);
    const float tau = a.seed_D[last];
    const bool have = ok && a.seed_I[last] >= 0 && tau == tau && fabsf(tau) <= 1073741824.f;
    int T = METRIC == METRIC_L2 ? -1 : 0x7fffffff, u = 0, init = -1073741824;
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
    return make_int4(init, cx, u, T);
}
// The start of one 32 x 32 accumulator tile of the wide pass: register 4 g + c of lane half h belongs to query slot
// QB0 + 8 g + 4 h + c, whose start value (s_init: exact_i8_slot's, by slot) goes from LDS into the accumulator.  h4 = 4 h.
// (scan_all_kernel keeps its own fold of its two tiles: through this function, in a one-tile or a several-tile form, its sixteen
// instantiations came out with other registers in 406 - 832 lines and missed the timing rule at one point: DESIGN.md 13.6)
template <int QB0> __device__ __forceinline__ void exact_i8_start(v16i& acc, const int* s_init, int h4) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const v4i t = *reinterpret_cast<const v4i*>(&s_init[QB0 + 8 * g + h4]);
#pragma unroll
        for (int c = 0; c < 4; c++) acc[4 * g + c] = t[c];
    }
}
// The epilogue of that tile for qbase's nq queries (s_cx, s_u, s_T: exact_i8_slot's values by slot); lane m holds the entry at `pos`,
// cy its constant, hc the bound of the pre-test: cy >> 1 (L2) / -cy (IP), INT_MAX where nothing may be emitted.  Eight registers at
// a time: their largest value against the bound first (v_max3), since most groups hold no candidate; a register that passes
// recomputes the distance and tests it exactly, NON-strictly; one returning atomic add per candidate.
template <int METRIC, int QB0>
__device__ __forceinline__ void exact_i8_emit(const ExactScanArgs& a, const v16i& acc, const int* s_cx, const int* s_u, const int* s_T, int h4,
                                              uint32_t qbase, uint32_t nq, int hc, int cy, uint32_t pos) {
    static_for(std::make_integer_sequence<int, 2>{}, [&](auto H) __attribute__((always_inline)) {
        constexpr int r0 = decltype(H)::value * 8;
        int mx = max(max(acc[r0], acc[r0 + 1]), acc[r0 + 2]);
        mx = max(max(mx, acc[r0 + 3]), acc[r0 + 4]);
        mx = max(max(mx, acc[r0 + 5]), acc[r0 + 6]);
        mx = max(mx, acc[r0 + 7]);
        if (__ballot(mx > hc) == 0) return;
        static_for(std::make_integer_sequence<int, 8>{}, [&](auto R) __attribute__((always_inline)) {
            constexpr int reg = r0 + decltype(R)::value;
            constexpr int q0 = QB0 + (reg & 3) + 8 * (reg >> 2);  // query slot of lane half 0; half 1: q0 + 4
            if (acc[reg] > hc) {
                const int sl = q0 + h4;
                const int cq = s_cx[sl], uq = s_u[sl], Tq = s_T[sl];
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
}

// The list pass.  Grid: (slabs of the block stream, tiles of 256 queries).  Wave w of a workgroup holds the A operands of query
// blocks 2 w and 2 w + 1 of the tile in registers for the whole slab; the four waves request the same list block, which reaches
// the compute unit once (the later requests are served by its vector cache) and is contracted with all eight query blocks.  No
// workgroup barrier anywhere: a wave whose query blocks do not exist leaves at once.
// A candidate of query q is an entry with dis <= T[q] (L2) / dis >= T[q] (IP), T = the seed's k-th distance: the EQUALITY is wanted,
// it is how a tie at the k-th is seen.  The pre-test is the pair kernel's strict one against T + 1 (L2: made even, so loosened by at
// most one more) / T - 1 (IP); a register that passes it recomputes the distance and tests it exactly.  Slots behind a list's end
// (ExactScanArgs::blk says how many of a block's 32 are entries) never pass: their bound is INT_MAX.
// KEEP (a call under a selector): blk.y is the mask of the slots that hold a MEMBER (exact_blocks_kernel<true>) and a slot is live iff
// its bit is set -- a non-member is treated exactly as a slot behind the list's end: it emits nothing, takes no candidate slot and
// moves no counter.  KEEP = false is the unfiltered pass, instruction for instruction what it was before the parameter existed.
template <int METRIC, int NKS, bool KEEP>
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
        const int4 v = exact_i8_slot<METRIC>(a, qbase + (sok ? (uint32_t)lane : 0u), sok);
        s_init[wave][lane] = v.x;
        s_cx[wave][lane] = v.y;
        s_u[wave][lane] = v.z;
        s_T[wave][lane] = v.w;
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
        const bool vok = KEEP ? ((biv.y >> m) & 1u) != 0 : (uint32_t)m < biv.y;  // (a slot behind the list's end, a non-member: nothing)
        int hc = !vok ? 0x7fffffff : METRIC == METRIC_L2 ? cyv >> 1 : -cyv;
        uint32_t pos = biv.x + (uint32_t)m;
        int cy;
        asm volatile("v_mov_b32 %0, %1" : "=v"(cy) : "v"(cyv));
        asm volatile("" : "+v"(hc), "+v"(pos));
        __builtin_amdgcn_sched_barrier(0);
        fetch(b, cyv, biv, i + 2 < B1 ? i + 2 : i);  // (past the slab's end: its own block again, never used)
        __builtin_amdgcn_sched_barrier(0);
        exact_i8_emit<METRIC, 0>(a, acc0, s_cx[wave], s_u[wave], s_T[wave], 4 * h, qbase, nq, hc, cy, pos);
        if (two) exact_i8_emit<METRIC, 32>(a, acc1, s_cx[wave], s_u[wave], s_T[wave], 4 * h, qbase, nq, hc, cy, pos);
    };
    for (uint64_t i = B0; i < B1; i += 2) {
        step(b0, cy0, bi0, i);
        step(b1, cy1, bi1, i + 1);
    }
}

// What the two fp16 list passes below share: a query slot's constants and the epilogue of an accumulator tile.
// A query slot's side of the keep rule: u = what an entry's side is compared with, +inf where nothing may pass (ok false: no query
// in the slot, then q is any valid query; no threshold), c = the factor of |y|.  Returns (u, c).
template <bool L2> __device__ __forceinline__ float2 exact_f16_slot(const ExactScanF16Args& a, float C, uint32_t q, bool ok) {
    const size_t last = (size_t)q * a.k + (a.k - 1);
    const float tau = a.seed_D[last], xn = a.xn[q];
    const bool have = ok && a.seed_I[last] >= 0 && tau == tau;
    return make_float2(have ? exact_float_bound(L2, C, xn, tau) : __builtin_inff(), exact_float_slack(L2, C, xn));
}
// The epilogue of one 32 x 32 accumulator tile: register 4 g + c of lane half h belongs to query slot QB0 + 8 g + 4 h + c of
// qbase's nq (s_u, s_c: exact_f16_slot's values by slot), lane m to the entry at `pos` (vok: it may be emitted; yn: its norm).  Four
// registers at a time, most hold nothing: exact_float_keep, a ballot, one returning atomic add per candidate.  h4 = 4 h.
template <bool L2, int QB0>
__device__ __forceinline__ void exact_f16_emit(const ExactScanF16Args& a, const v16f& acc, const float* s_u, const float* s_c, int h4, uint32_t qbase,
                                               uint32_t nq, float C, float ps, bool vok, float yn, uint32_t pos) {
    static_for(std::make_integer_sequence<int, 4>{}, [&](auto G) __attribute__((always_inline)) {
        constexpr int g = decltype(G)::value;
        const v4f tu = *reinterpret_cast<const v4f*>(&s_u[QB0 + 8 * g + h4]);
        const v4f tc = *reinterpret_cast<const v4f*>(&s_c[QB0 + 8 * g + h4]);
        bool keep[4];
        bool any = false;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            keep[c] = vok && exact_float_keep(L2, C, ps * acc[4 * g + c], yn, tu[c], tc[c]);  // (ps: a power of two, exact)
            any |= keep[c];
        }
        if (__ballot(any) == 0) return;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int sl = QB0 + 8 * g + h4 + c;
            if (keep[c] && (uint32_t)sl < nq) {
                const uint32_t q = qbase + (uint32_t)sl;
                const uint32_t slot = atomicAdd(&a.cnt[q], 1u);  // (beyond cap only the counter moves)
                if (slot < a.cap) a.cand[(size_t)q * a.cap + slot] = make_uint2(pos, 0u);
            }
        }
    });
}

// The list pass over float lists: the same grid, slabs, query tiles and block stream, on the fp16 copy the filter keeps (ivf_filter.hip:
// a block is NJ pieces of 1 KiB, 16 dimensions each, in the operand order of v_mfma_f32_32x32x16_f16; the query rows are
// filter_queries16_kernel's).  Wave w holds the A operands of its two query blocks -- NJ pieces of four registers each -- for the
// whole slab, two list blocks are in flight, no workgroup barrier.  An accumulator times ps is x.y up to the filter's bound, and the
// keep rule is exact_args.h's exact_float_keep, NON-strict: every stored entry whose reference distance is at or within the query's
// threshold is emitted, with others the bound lets through; exact_rescore_kernel computes the reference's value of
// each and the selection drops what lies beyond the threshold.  Emitted: (global position, -).
// Registers (hipcc -O3, gfx950, --save-temps): NJ = 8 is the largest form, 2 x 32 operand registers of the queries, 2 x 32 of the
// blocks in flight, 2 x 16 accumulators; no instantiation uses scratch (DESIGN.md 13 has the table).
// KEEP: as in scan_all_kernel, blk.y is the members' mask; a non-member is never emitted, so it is never rescored either.
template <int METRIC, int NJ, bool KEEP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_all_f16_kernel(ExactScanF16Args a) {
    static_assert(NJ == 4 || NJ == 6 || NJ == 8, "the piece counts of filter_steps16 up to 128 dimensions");
    constexpr bool L2 = METRIC == METRIC_L2;
    __shared__ float s_u[4][64];
    __shared__ float s_c[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 31, h = lane >> 5;
    constexpr size_t qstride = (size_t)NJ * 8;      // floats of a query row (16 NJ halves)
    constexpr size_t block_floats = (size_t)NJ * 256;
    const uint32_t qbase = blockIdx.y * 256u + (uint32_t)wave * 64u;
    if (qbase >= a.n) return;
    const uint32_t nq = a.n - qbase < 64u ? a.n - qbase : 64u;  // query slots of this wave that hold a query
    const bool two = nq > 32;                                  // (wave-uniform)
    const uint64_t B0 = (uint64_t)blockIdx.x * a.slab;
    const uint64_t B1 = B0 + a.slab < a.nblk ? B0 + a.slab : a.nblk;  // (slab and nblk are even)
    if (B0 >= B1) return;
    const FilterParams fp = *a.params;
    const float C = fp.C, ps = fp.ps;

    // ---- per query slot (slot = lane): what the keep rule compares with; +inf where nothing may pass (no query, no threshold)
    {
        const bool sok = (uint32_t)lane < nq;
        const float2 uc = exact_f16_slot<L2>(a, C, qbase + (sok ? (uint32_t)lane : 0u), sok);
        s_u[wave][lane] = uc.x;
        s_c[wave][lane] = uc.y;
    }
    // ---- the A operands: lane (m, h) of query block g holds halves 16 j + 8 h .. + 7 of query slot 32 g + m, piece j
    v4f af0[NJ], af1[NJ];
    {
        const bool qok0 = (uint32_t)m < nq, qok1 = (uint32_t)(32 + m) < nq;
        const float* q0p = a.xf + (size_t)(qbase + (qok0 ? (uint32_t)m : 0u)) * qstride + (size_t)h * 4;
        const float* q1p = a.xf + (size_t)(qbase + (qok1 ? 32u + (uint32_t)m : 0u)) * qstride + (size_t)h * 4;
#pragma unroll
        for (int j = 0; j < NJ; j++) af0[j] = qok0 ? *reinterpret_cast<const v4f*>(q0p + 8 * j) : v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; j++) af1[j] = qok1 ? *reinterpret_cast<const v4f*>(q1p + 8 * j) : v4f{0.f, 0.f, 0.f, 0.f};
    }
    wave_sync();

    // ---- the block stream: two blocks in flight per wave, block i + 2 requested right behind the MFMAs of block i
    v4f b0[NJ], b1[NJ];
    float yn0 = 0.f, yn1 = 0.f;
    uint2 bi0 = make_uint2(0, 0), bi1 = make_uint2(0, 0);
    auto fetch = [&](v4f (&b)[NJ], float& yn, uint2& bi, uint64_t blk) {
        const float* bp = a.codes_frag + blk * block_floats + (size_t)lane * 4;
#pragma unroll
        for (int j = 0; j < NJ; j++) b[j] = *reinterpret_cast<const v4f*>(bp + (size_t)j * 256);
        yn = a.yn[blk * 32 + m];
        bi = a.blk[blk];
    };
    fetch(b0, yn0, bi0, B0);
    fetch(b1, yn1, bi1, B0 + 1);

    auto step = [&](v4f (&b)[NJ], float& ynv, uint2& biv, uint64_t i) {
        __builtin_amdgcn_sched_barrier(0);
        v16f acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; r++) acc0[r] = acc1[r] = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; j++)
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, af0[j]), __builtin_bit_cast(v8h, b[j]), acc0, 0, 0, 0);
        if (two) {
#pragma unroll
            for (int j = 0; j < NJ; j++)
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, af1[j]), __builtin_bit_cast(v8h, b[j]), acc1, 0, 0, 0);
        }
        // what the epilogue needs of the block's constants is taken before their registers are requested again
        const bool vok = KEEP ? ((biv.y >> m) & 1u) != 0 : (uint32_t)m < biv.y;  // (a slot behind the list's end, a non-member: nothing)
        uint32_t pos = biv.x + (uint32_t)m;
        float yn;
        asm volatile("v_mov_b32 %0, %1" : "=v"(yn) : "v"(ynv));
        asm volatile("" : "+v"(pos));
        __builtin_amdgcn_sched_barrier(0);
        fetch(b, ynv, biv, i + 2 < B1 ? i + 2 : i);  // (past the slab's end: its own block again, never used)
        __builtin_amdgcn_sched_barrier(0);
        exact_f16_emit<L2, 0>(a, acc0, s_u[wave], s_c[wave], 4 * h, qbase, nq, C, ps, vok, yn, pos);
        if (two) exact_f16_emit<L2, 32>(a, acc1, s_u[wave], s_c[wave], 4 * h, qbase, nq, C, ps, vok, yn, pos);
    };
    for (uint64_t i = B0; i < B1; i += 2) {
        step(b0, yn0, bi0, i);
        step(b1, yn1, bi1, i + 1);
    }
}

// The fp16 list pass beyond 128 dimensions (option "exact_wide").  At J = filter_steps16(d) = 10 .. 64 pieces the
// query operand no longer fits a wave's registers, so the tile is scan_filter_wide_kernel's (ivf_filter.hip), over the exact pass's
// block stream.  Grid: (slabs of the block stream, tiles of 128 queries).  The four waves walk the slab in chunks of four
// consecutive blocks; wave w owns block w of the chunk, whose pieces stream from HBM once, straight into a register ring of SP
// pieces (the slot of piece j is refilled with piece j + SP right behind its MFMAs; behind a chunk's last stage the slots take the
// first SP pieces of the wave's block of the NEXT chunk, so the ring stays full across chunks).  The tile's query operand -- up to
// four query blocks of filter_queries16_kernel's rows, wave w staging the rows of query block w -- goes through LDS in stages of SP
// pieces, double-buffered, one LDS-only barrier per stage; the stages do not depend on the chunk, so the stage written behind a
// chunk's last is stage 0 again and the buffers simply alternate along the whole slab.  Four accumulator tiles per wave, the K
// loop compiled per count of query blocks.  The per-query constants of the keep rule are written to LDS once per workgroup.  The
// epilogue is scan_all_f16_kernel's: exact_float_keep (non-strict), the block table's count or (KEEP) members' mask, a ballot per
// four registers, one returning atomic add per candidate, (position, -) stored while the slot is below cap.
// Straight-line code (mfma_tile.h says why): every wave runs the same loads, stages and barriers whatever its share -- a wave without
// a query block stages the tile's first row (nothing reads it), a wave without a block in the stream's last chunk (nblk % 4 == 2)
// recomputes the chunk's first block and drops the result, a piece index past J reads piece J - 1 and its stage slot is written as
// zero.  Nothing is read past nblk x J KiB of the copy or past row n - 1.
#ifndef AUNCEL_EXACT_WIDE_SP
#define AUNCEL_EXACT_WIDE_SP 6  // (as AUNCEL_FILTER_WIDE_SP, ivf_filter.hip: that kernel spilled at 8)
#endif
constexpr int EXACT_WIDE_SP = AUNCEL_EXACT_WIDE_SP;
constexpr int EXACT_WIDE_QB = (int)(EXACT_WIDE_QUERIES / 32);
constexpr size_t EXACT_WIDE_LDS = wide_lds_bytes(EXACT_WIDE_QB, EXACT_WIDE_SP, 2);  // (the stages + bound and slack per query)
static_assert(EXACT_WIDE_SP >= 2 && EXACT_WIDE_SP % 2 == 0 && EXACT_WIDE_SP <= 10, "pieces are taken in pairs; a stage is not longer than the fewest pieces");
static_assert(2 * EXACT_WIDE_LDS <= 160 * 1024, "two workgroups per compute unit");

template <int METRIC, bool KEEP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_all_wide_f16_kernel(ExactScanF16Args a) {
    constexpr bool L2 = METRIC == METRIC_L2;
    constexpr int QB = EXACT_WIDE_QB, SP = EXACT_WIDE_SP;
    extern __shared__ __align__(16) unsigned char exact_wide_smem[];
    float* s_a = reinterpret_cast<float*>(exact_wide_smem);  // [2 buffers][query block][piece of the stage][lane][4]
    float* s_u = s_a + 2 * wide_stage_words(QB, SP);
    float* s_c = s_u + EXACT_WIDE_QUERIES;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 31, h = lane >> 5;
    const int J = (int)filter_steps16(a.d);
    const int S = exact_wide_stages(J, SP);
    const size_t qstride = (size_t)J * 8;
    const size_t block_floats = (size_t)J * 256;
    const uint32_t qbase = blockIdx.y * EXACT_WIDE_QUERIES;
    const uint64_t B0 = (uint64_t)blockIdx.x * a.slab;
    const uint64_t B1 = B0 + a.slab < a.nblk ? B0 + a.slab : a.nblk;  // (slab: a multiple of 4; nblk is even)
    if (qbase >= a.n || B0 >= B1) return;                            // (the same for the whole workgroup)
    const uint32_t nq = a.n - qbase < EXACT_WIDE_QUERIES ? a.n - qbase : EXACT_WIDE_QUERIES;  // query slots of the tile that hold a query
    const int nqb = (int)((nq + 31) >> 5);
    const FilterParams fp = *a.params;
    const float C = fp.C, ps = fp.ps;

    // ---- per query slot, once for the slab: what the keep rule compares with; +inf where nothing may pass (no query, no threshold).
    // (slot = thread & 127: the upper two waves write what the lower two write)
    {
        const uint32_t sl = threadIdx.x & (EXACT_WIDE_QUERIES - 1);
        const bool sok = sl < nq;
        const float2 uc = exact_f16_slot<L2>(a, C, qbase + (sok ? sl : 0u), sok);
        s_u[sl] = uc.x;
        s_c[sl] = uc.y;
    }
    // ---- the query operand: this wave stages the rows of query block `wave`, lane (m, h) halves 16 j + 8 h .. + 7 of query slot
    // 32 wave + m, piece j (a slot without a query: the tile's first row; its bound is +inf)
    const uint32_t qslot = (uint32_t)wave * 32u + (uint32_t)m;
    const WideTile<TileFloat<true>, SP, QB> tile{s_a, a.xf + (size_t)(qbase + (qslot < nq ? qslot : 0u)) * qstride + (size_t)h * 4, J, wave, lane};
    v4f st[SP];
    tile.stage_load(0, st);
    tile.stage_write(0, 0, st);
    // ---- this wave's block, a ring of SP pieces
    const float* fbase = a.codes_frag + (size_t)lane * 4;
    v4f br[SP];
    {
        const float* b0 = fbase + exact_wide_wave_block(B0, B1, (uint32_t)wave) * block_floats;
#pragma unroll
        for (int jj = 0; jj < SP; jj++) br[jj] = *(gv4f)(uintptr_t)(b0 + (size_t)jj * 256);  // (SP <= 10 <= J)
    }
    lds_barrier();  // stage 0 and the per-query constants are in LDS

    auto run = [&](auto NQBc) __attribute__((always_inline)) {
        constexpr int NQB = decltype(NQBc)::value;
        int buf = 0;
        for (uint64_t c = B0; c < B1; c += EXACT_WIDE_CHUNK) {
            const bool active = (uint32_t)wave < exact_wide_chunk_blocks(c, B1);
            const uint64_t cur = exact_wide_wave_block(c, B1, (uint32_t)wave);
            const uint64_t cn = c + EXACT_WIDE_CHUNK < B1 ? c + EXACT_WIDE_CHUNK : c;  // (no next chunk: this one again, never used)
            const float* bbase = fbase + cur * block_floats;
            const float* nbase = fbase + exact_wide_wave_block(cn, B1, (uint32_t)wave) * block_floats;
            const float yn = a.yn[cur * 32 + (uint64_t)m];
            const uint2 bi = a.blk[cur];
            v16f acc[NQB];
#pragma unroll
            for (int q = 0; q < NQB; q++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[q][r] = 0.f;
            for (int s = 0; s < S; s++) {
                const bool lasts = s + 1 == S;
                // the refill of ring slot jj: piece j + SP of this block (past J: J - 1 again, multiplied by a zero stage slot), or
                // behind the last stage piece jj of the wave's block of the next chunk
                auto refill = [&](int j, int jj, v4f& bv) __attribute__((always_inline)) {
                    const float* src = lasts ? nbase + (size_t)jj * 256 : bbase + (size_t)(j + SP < J ? j + SP : J - 1) * 256;
                    bv = *(gv4f)(uintptr_t)src;
                };
                tile.stage<NQB>(buf, s, lasts ? 0 : s + 1, st, acc, br, refill);  // (behind a chunk's last stage: stage 0, for the next chunk)
                buf ^= 1;
            }
            // ---- epilogue: register 4 g + c of lane half h of tile qb belongs to query slot 32 qb + 8 g + 4 h + c, lane m to slot m
            // of the block; a slot behind the list's end, a non-member, a block computed in another wave's stead: nothing
            const bool vok = active && (KEEP ? ((bi.y >> m) & 1u) != 0 : (uint32_t)m < bi.y);
            const uint32_t pos = bi.x + (uint32_t)m;
            // (opaque per chunk: a tile's 64 query numbers, their tests against nq and the counter and buffer addresses do not change
            // along the slab, and hoisted out of the chunk loop they were 64 vector and 128 scalar registers, spilled)
            int h4 = 4 * h;
            asm volatile("" : "+v"(h4));
            static_for(std::make_integer_sequence<int, NQB>{}, [&](auto T) __attribute__((always_inline)) {
                constexpr int t = decltype(T)::value;
                exact_f16_emit<L2, 32 * t>(a, acc[t], s_u, s_c, h4, qbase, nq, C, ps, vok, yn, pos);
            });
        }
    };
    switch (nqb) {
        case 1: run(std::integral_constant<int, 1>{}); break;
        case 2: run(std::integral_constant<int, 2>{}); break;
        case 3: run(std::integral_constant<int, 3>{}); break;
        default: run(std::integral_constant<int, 4>{}); break;
    }
}

// The byte list pass beyond 128 dimensions (option "exact_wide_bytes"): scan_all_kernel's arithmetic and epilogue on
// scan_all_wide_f16_kernel's tile.  At J = mfma_ksteps(d) = 5 .. 32 pieces of 32 dimensions the query operand no longer fits a wave's
// registers.  Grid: (slabs of the block stream, tiles of 128 queries).  The four waves walk the slab in chunks of four consecutive
// blocks; wave w owns block w of the chunk, whose J pieces of 1 KiB stream from the byte fragments once, straight into a register
// ring of SP pieces (the slot of piece j is refilled with piece j + SP right behind its MFMAs; behind a chunk's last stage with the
// first SP pieces of the wave's block of the next chunk).  The query operand -- up to four query blocks of byte_queries' rows, wave w
// staging the rows of query block w -- goes through LDS in stages of SP pieces, double-buffered, one LDS-only barrier per stage.
// Per-query threshold, start value, u and cx are written to LDS once per workgroup (exact_i8_slot); the start values are folded into
// the accumulators (exact_i8_start) and the epilogue is exact_i8_emit, with the block table's count or (KEEP) members' mask.
// Straight-line code (mfma_tile.h says why): every wave runs the same loads, stages and barriers -- a wave without a query block
// stages the tile's first row (nothing reads it), a wave without a block in the stream's last chunk recomputes the chunk's first
// block and drops the result, a piece index past J reads piece J - 1 and its stage slot is written as zero.  Nothing is read past
// nblk x J KiB of the fragments or past row n - 1.
#ifndef AUNCEL_EXACT_WIDE_I8_SP
#define AUNCEL_EXACT_WIDE_I8_SP 6  // (the fp16 tile's; a stage is not longer than the fewest pieces, J = 5, rounded up to a pair)
#endif
constexpr int EXACT_WIDE_I8_SP = AUNCEL_EXACT_WIDE_I8_SP;
constexpr size_t EXACT_WIDE_I8_LDS = wide_lds_bytes(EXACT_WIDE_QB, EXACT_WIDE_I8_SP, 4);  // (the stages + start value, cx, u and T per query)
static_assert(EXACT_WIDE_I8_SP >= 2 && EXACT_WIDE_I8_SP % 2 == 0 && EXACT_WIDE_I8_SP <= 6, "pieces are taken in pairs; the ring's first fill reads pieces 0 .. SP - 1 of J >= 5 (past J: J - 1)");
static_assert(2 * EXACT_WIDE_I8_LDS <= 160 * 1024, "two workgroups per compute unit");

template <int METRIC, bool KEEP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_all_wide_i8_kernel(ExactScanArgs a) {
    constexpr int QB = EXACT_WIDE_QB, SP = EXACT_WIDE_I8_SP;
    extern __shared__ __align__(16) unsigned char exact_wide_i8_smem[];
    int* s_a = reinterpret_cast<int*>(exact_wide_i8_smem);  // [2 buffers][query block][piece of the stage][lane][4]
    int* s_init = s_a + 2 * wide_stage_words(QB, SP);
    int* s_cx = s_init + EXACT_WIDE_QUERIES;
    int* s_u = s_cx + EXACT_WIDE_QUERIES;
    int* s_T = s_u + EXACT_WIDE_QUERIES;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 31, h = lane >> 5;
    const int J = (int)mfma_ksteps(a.d);
    const int S = exact_wide_stages(J, SP);
    const size_t qstride = (size_t)J * 32;
    const size_t block_bytes = (size_t)J * 1024;
    const uint32_t qbase = blockIdx.y * EXACT_WIDE_QUERIES;
    const uint64_t B0 = (uint64_t)blockIdx.x * a.slab;
    const uint64_t B1 = B0 + a.slab < a.nblk ? B0 + a.slab : a.nblk;  // (slab: a multiple of 4; nblk is even)
    if (qbase >= a.n || B0 >= B1) return;                            // (the same for the whole workgroup)
    const uint32_t nq = a.n - qbase < EXACT_WIDE_QUERIES ? a.n - qbase : EXACT_WIDE_QUERIES;  // query slots of the tile that hold a query
    const int nqb = (int)((nq + 31) >> 5);

    // ---- per query slot, once for the slab: threshold and start value (slot = thread & 127: the upper two waves write what the
    // lower two write)
    {
        const uint32_t sl = threadIdx.x & (EXACT_WIDE_QUERIES - 1);
        const bool sok = sl < nq;
        const int4 v = exact_i8_slot<METRIC>(a, qbase + (sok ? sl : 0u), sok);
        s_init[sl] = v.x;
        s_cx[sl] = v.y;
        s_u[sl] = v.z;
        s_T[sl] = v.w;
    }
    // ---- the query operand: this wave stages the rows of query block `wave`, lane (m, h) bytes 16 J h + 16 j .. + 15 of query slot
    // 32 wave + m, piece j (a slot without a query: the tile's first row; nothing of its accumulators is emitted)
    const uint32_t qslot = (uint32_t)wave * 32u + (uint32_t)m;
    const WideTile<TileI8, SP, QB> tile{s_a, a.queries8 + (size_t)(qbase + (qslot < nq ? qslot : 0u)) * qstride + (size_t)h * (size_t)(16 * J), J, wave, lane};
    v4i st[SP];
    tile.stage_load(0, st);
    tile.stage_write(0, 0, st);
    // ---- this wave's block, a ring of SP pieces
    const uint8_t* fbase = a.codes_frag + (size_t)lane * 16;
    v4i br[SP];
    {
        const uint8_t* b0 = fbase + exact_wide_wave_block(B0, B1, (uint32_t)wave) * block_bytes;
#pragma unroll
        for (int jj = 0; jj < SP; jj++) br[jj] = *(gv4i)(uintptr_t)(b0 + (size_t)(jj < J ? jj : J - 1) * 1024);  // (J = 5: slot 5 is multiplied by zero)
    }
    lds_barrier();  // stage 0 and the per-query constants are in LDS

    auto run = [&](auto NQBc) __attribute__((always_inline)) {
        constexpr int NQB = decltype(NQBc)::value;
        int buf = 0;
        for (uint64_t c = B0; c < B1; c += EXACT_WIDE_CHUNK) {
            const bool active = (uint32_t)wave < exact_wide_chunk_blocks(c, B1);
            const uint64_t cur = exact_wide_wave_block(c, B1, (uint32_t)wave);
            const uint64_t cn = c + EXACT_WIDE_CHUNK < B1 ? c + EXACT_WIDE_CHUNK : c;  // (no next chunk: this one again, never used)
            const uint8_t* bbase = fbase + cur * block_bytes;
            const uint8_t* nbase = fbase + exact_wide_wave_block(cn, B1, (uint32_t)wave) * block_bytes;
            const int cy = a.code_cy[cur * 32 + (uint64_t)m];
            const uint2 bi = a.blk[cur];
            v16i acc[NQB];
            static_for(std::make_integer_sequence<int, NQB>{}, [&](auto T) __attribute__((always_inline)) {
                exact_i8_start<32 * decltype(T)::value>(acc[decltype(T)::value], s_init, 4 * h);
            });
            for (int s = 0; s < S; s++) {
                const bool lasts = s + 1 == S;
                // the refill of ring slot jj: piece j + SP of this block (past J: J - 1 again, multiplied by a zero stage slot), or
                // behind the last stage piece jj of the wave's block of the next chunk
                auto refill = [&](int j, int jj, v4i& bv) __attribute__((always_inline)) {
                    const uint8_t* src = lasts ? nbase + (size_t)(jj < J ? jj : J - 1) * 1024 : bbase + (size_t)(j + SP < J ? j + SP : J - 1) * 1024;
                    bv = *(gv4i)(uintptr_t)src;
                };
                tile.template stage<NQB>(buf, s, lasts ? 0 : s + 1, st, acc, br, refill);  // (behind a chunk's last stage: stage 0, for the next chunk)
                buf ^= 1;
            }
            // ---- epilogue: lane m holds slot m of the block; a slot behind the list's end, a non-member, a block computed in another
            // wave's stead: nothing (the bound no accumulator exceeds)
            const bool vok = active && (KEEP ? ((bi.y >> m) & 1u) != 0 : (uint32_t)m < bi.y);
            const int hc = !vok ? 0x7fffffff : METRIC == METRIC_L2 ? cy >> 1 : -cy;
            const uint32_t pos = bi.x + (uint32_t)m;
            // (opaque per chunk, as in scan_all_wide_f16_kernel: nothing of the epilogue's addressing is hoisted out of the chunk loop)
            int h4 = 4 * h;
            asm volatile("" : "+v"(h4));
            static_for(std::make_integer_sequence<int, NQB>{}, [&](auto T) __attribute__((always_inline)) {
                constexpr int t = decltype(T)::value;
                exact_i8_emit<METRIC, 32 * t>(a, acc[t], s_cx, s_u, s_T, h4, qbase, nq, hc, cy, pos);
            });
        }
    };
    switch (nqb) {
        case 1: run(std::integral_constant<int, 1>{}); break;
        case 2: run(std::integral_constant<int, 2>{}); break;
        case 3: run(std::integral_constant<int, 3>{}); break;
        default: run(std::integral_constant<int, 4>{}); break;
    }
}

// The candidates of the fp16 pass recomputed from the fp32 rows in the reference's rounding sequence (ivf_dev.h: exact_distance; as in
// rescore_kernel four neighbouring lanes take one candidate, lane l running sum l, then (s0 + s1) + (s2 + s3)): the distance's bits
// replace the candidate's second word.  A workgroup per query, 64 candidates a trip.
template <int METRIC> __global__ __launch_bounds__(256) void exact_rescore_kernel(ExactRescoreArgs a) {
    const uint32_t q = blockIdx.x;
    const uint32_t n = a.cnt[q] < a.cap ? a.cnt[q] : a.cap;
    const uint32_t sub = threadIdx.x & 3;
    const float* x = a.queries + (size_t)q * a.dpad;
    for (uint32_t i = threadIdx.x >> 2; i < n; i += 64) {
        uint2* slot = a.cand + (size_t)q * a.cap + i;
        const float* y = a.codes + (size_t)slot->x * a.dpad;
        float sl = 0.f;
        for (int c = (int)sub; c < a.dpad; c += 4) {
            if (METRIC == METRIC_L2) {
                const float t = y[c] - x[c];
                sl += t * t;
            } else {
                sl += y[c] * x[c];
            }
        }
        const float pair = sl + __shfl_xor(sl, 1);    // lanes 0/1: s0 + s1, lanes 2/3: s2 + s3
        const float ex = pair + __shfl_xor(pair, 2);  // (s0 + s1) + (s2 + s3)
        if (sub == 0) slot->y = __float_as_uint(ex);
    }
}

// A wave per query: its candidates sorted by (distance, global position) in LDS (a bitonic network over the next power of two), then
// the tie rule.  flag[q]: 0 the result was written, 1 equal distances met in the window, 2 anything else (no threshold: the seed's
// result was not full; more candidates than slots).  totals: [0..2] queries by flag, [3] candidates emitted, [4] candidates at or
// within the threshold, [5] the largest emitted count of one query.
// RESCORED (the fp16 pass): a candidate's distance is the reference's value, recomputed; one that lies strictly beyond the threshold
// was let through by the bound only -- its key is the largest there is, so it sorts behind every other, and it is not counted: the
// window and the test for "fewer than k" see the VALID candidates.  The keys are the distances' bit patterns through fkey, an order
// only without NaN and -0: neither occurs.
template <bool RESCORED> __global__ __launch_bounds__(64) void exact_select_kernel(ExactSelectArgs a) {
    extern __shared__ unsigned long long s_key[];
    const uint32_t q = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t emitted = a.cnt[q], k = a.k;
    const bool have = a.seed_I[(size_t)q * k + (k - 1)] >= 0;
    uint32_t cnt = emitted;  // the valid candidates
    if (RESCORED) {
        const uint32_t stored = emitted < a.cap ? emitted : a.cap;
        const float tau = a.seed_D[(size_t)q * k + (k - 1)];
        uint32_t mine = 0;
        if (have)
            for (uint32_t i = lane; i < stored; i += 64) {
                const float dis = __uint_as_float(a.cand[(size_t)q * a.cap + i].y);
                mine += a.metric == METRIC_L2 ? dis <= tau : dis >= tau;
            }
        cnt = wave_sum_u32(mine);
    }
    uint32_t flag = (!have || emitted > a.cap || cnt < k) ? 2u : 0u;  // (wave-uniform)
    if (!flag) {
        uint32_t P = 2;
        while (P < emitted) P <<= 1;
        const float tau = RESCORED ? a.seed_D[(size_t)q * k + (k - 1)] : 0.f;
        for (uint32_t i = lane; i < P; i += 64) {
            unsigned long long key = ~0ull;
            if (i < emitted) {
                const uint2 c = a.cand[(size_t)q * a.cap + i];
                const float dis = __uint_as_float(c.y);
                const uint32_t fk = fkey(dis);
                if (!RESCORED || (a.metric == METRIC_L2 ? dis <= tau : dis >= tau)) key = exact_key(a.metric == METRIC_L2 ? fk : ~fk, c.x);
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
        atomicAdd(&a.totals[3], (unsigned long long)emitted);
        atomicAdd(&a.totals[4], (unsigned long long)cnt);
        atomicMax(&a.totals[5], (unsigned long long)emitted);
    }
}

// Exact range search (amd_ivf_range_search_exact): a query's candidates -- what the list pass emitted for the radius
// as threshold, in the order the atomics fell -- become the reference's run.  A candidate is valid iff the reference's strict compare
// holds for the caller's radius on its distance (the byte pass's exact integer, or the rescored reference value); the key of a valid
// one is its global position above its distance's bits, of any other the largest there is, and a bitonic network over the next power
// of two puts the valid ones first, in position order: positions are unique, so that order is determined, and it is the reference's
// (lists in list-number order, entries in position order).  The run is written back to the head of the query's slots.
// One workgroup per query, in two forms that share the grid: 64 threads -- ONE wave -- take the queries with up to 256 candidates
// (and mark the ones with more candidates than slots: flag 2, nothing sorted), 256 threads the ones beyond; the other form's
// queries are left at once.  Every barrier is between two stages of the network in LDS; memory is read once, before the first, and
// written once, behind the last.  totals: as exact_select_kernel's.
constexpr uint32_t EXACT_RANGE_WAVE_MAX = 256;
template <int THREADS> __global__ __launch_bounds__(THREADS) void exact_range_collect_kernel(ExactRangeArgs a) {
    extern __shared__ unsigned long long s_rkey[];
    __shared__ uint32_t s_valid;
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    const uint32_t emitted = a.cnt[q];
    const bool over = emitted > a.cap, large = emitted > EXACT_RANGE_WAVE_MAX;
    if (THREADS == 64 ? (large && !over) : (!large || over)) return;  // (the same for the whole workgroup)
    uint32_t valid = 0;
    if (!over && emitted) {
        uint32_t P = 2;
        while (P < emitted) P <<= 1;  // (<= the next power of two of cap: what the launch reserved)
        if (t == 0) s_valid = 0;
        const bool l2 = a.metric == METRIC_L2;
        for (uint32_t i = t; i < P; i += THREADS) {
            unsigned long long key = EXACT_RANGE_INVALID;
            if (i < emitted) {
                const uint2 c = a.cand[(size_t)q * a.cap + i];
                if (exact_range_within(l2, a.radius, __uint_as_float(c.y))) key = exact_range_key(c.x, c.y);
            }
            s_rkey[i] = key;
        }
        for (uint32_t kk = 2; kk <= P; kk <<= 1)
            for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                __syncthreads();
                for (uint32_t i = t; i < P; i += THREADS) {
                    const uint32_t l = i ^ j;
                    if (l > i) {
                        const unsigned long long x = s_rkey[i], y = s_rkey[l];
                        if ((x > y) == ((i & kk) == 0)) {
                            s_rkey[i] = y;
                            s_rkey[l] = x;
                        }
                    }
                }
            }
        __syncthreads();
        // the valid run ends where the largest key begins (at most one thread sees the edge; none: no valid candidate)
        for (uint32_t i = t; i < P; i += THREADS)
            if (s_rkey[i] != EXACT_RANGE_INVALID && (i + 1 == P || s_rkey[i + 1] == EXACT_RANGE_INVALID)) s_valid = i + 1;
        __syncthreads();
        valid = s_valid;
        for (uint32_t i = t; i < valid; i += THREADS) {
            const unsigned long long key = s_rkey[i];
            a.cand[(size_t)q * a.cap + i] = make_uint2((uint32_t)(key >> 32), (uint32_t)key);
        }
    }
    if (t == 0) {
        const uint32_t flag = over ? 2u : 0u;
        a.valid[q] = valid;
        a.flag[q] = flag;
        atomicAdd(&a.totals[flag], 1ull);
        atomicAdd(&a.totals[3], (unsigned long long)emitted);
        atomicAdd(&a.totals[4], (unsigned long long)valid);
        atomicMax(&a.totals[5], (unsigned long long)emitted);
    }
}

// (id, distance) of every answered query's run, at the query's place in the call's result
__global__ __launch_bounds__(64) void exact_range_fill_kernel(ExactRangeFillArgs a) {
    const uint32_t q = blockIdx.x;
    if (a.flag[q]) return;
    const uint32_t n = a.valid[q];
    const uint64_t at = a.off[q];
    for (uint32_t j = threadIdx.x; j < n; j += 64) {
        const uint2 c = a.cand[(size_t)q * a.cap + j];
        a.labels[at + j] = a.ids[c.x];
        a.dist[at + j] = __uint_as_float(c.y);
    }
}

}  // namespace

void launch_exact_range_collect(const ExactRangeArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    uint32_t P = 2;
    while (P < a.cap) P <<= 1;
    LAUNCH(exact_range_collect_kernel<64>, dim3(a.n), dim3(64), (size_t)std::min(P, EXACT_RANGE_WAVE_MAX) * 8, s, a);
    if (a.cap > EXACT_RANGE_WAVE_MAX) LAUNCH(exact_range_collect_kernel<256>, dim3(a.n), dim3(256), (size_t)P * 8, s, a);
}

void launch_exact_range_fill(const ExactRangeFillArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    LAUNCH(exact_range_fill_kernel, dim3(a.n), dim3(64), 0, s, a);
}

void launch_exact_blocks(const uint64_t* list_off, const uint64_t* block_off, const unsigned long long* keep, uint32_t nlist, uint64_t nblk,
                         uint2* out, hipStream_t s) {
    if (nblk == 0) return;
    const dim3 grid((unsigned)((nblk + 255) / 256)), block(256);
    if (keep) LAUNCH(exact_blocks_kernel<true>, grid, block, 0, s, list_off, block_off, nlist, nblk, out, keep);
    else LAUNCH(exact_blocks_kernel<false>, grid, block, 0, s, list_off, block_off, nlist, nblk, out, keep);
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

// f(metric, keep as compile-time constants): the instantiation of a list pass for a call's metric and table variant
template <class F> static void with_metric_keep(int metric, bool keep, F&& f) {
    auto pick = [&](auto K) {
        if (metric == METRIC_L2) f(std::integral_constant<int, METRIC_L2>{}, K);
        else f(std::integral_constant<int, METRIC_IP>{}, K);
    };
    if (keep) pick(std::true_type{});
    else pick(std::false_type{});
}

void launch_scan_all(const ExactScanArgs& a, bool keep, hipStream_t s) {
    if (a.n == 0 || a.nblk == 0) return;
    const int ks = (int)mfma_ksteps(a.d);
    if (ks < 1 || ks > 4 || a.slab == 0 || (a.slab & 1) || (a.nblk & 1)) throw std::runtime_error("scan_all_kernel: shape not supported");
    const dim3 grid((unsigned)((a.nblk + a.slab - 1) / a.slab), (unsigned)((a.n + 255) / 256)), block(256);
    auto go = [&](auto kern) { LAUNCH(kern, grid, block, 0, s, a); };
    with_metric_keep(a.metric, keep, [&](auto M, auto K) {
        constexpr int METRIC = decltype(M)::value;
        constexpr bool KEEP = decltype(K)::value;
        switch (ks) {
            case 1: return go(scan_all_kernel<METRIC, 1, KEEP>);
            case 2: return go(scan_all_kernel<METRIC, 2, KEEP>);
            case 3: return go(scan_all_kernel<METRIC, 3, KEEP>);
            default: return go(scan_all_kernel<METRIC, 4, KEEP>);
        }
    });
}

void launch_scan_all_f16(const ExactScanF16Args& a, bool keep, hipStream_t s) {
    if (a.n == 0 || a.nblk == 0) return;
    const int J = a.d >= 1 && a.d <= 128 ? (int)filter_steps16(a.d) : 0;
    if (J == 0 || a.slab == 0 || (a.slab & 1) || (a.nblk & 1)) throw std::runtime_error("scan_all_f16_kernel: shape not supported");
    const dim3 grid((unsigned)((a.nblk + a.slab - 1) / a.slab), (unsigned)((a.n + 255) / 256)), block(256);
    auto go = [&](auto kern) { LAUNCH(kern, grid, block, 0, s, a); };
    with_metric_keep(a.metric, keep, [&](auto M, auto K) {
        constexpr int METRIC = decltype(M)::value;
        constexpr bool KEEP = decltype(K)::value;
        switch (J) {
            case 4: return go(scan_all_f16_kernel<METRIC, 4, KEEP>);
            case 6: return go(scan_all_f16_kernel<METRIC, 6, KEEP>);
            default: return go(scan_all_f16_kernel<METRIC, 8, KEEP>);
        }
    });
}

// the launch of a wide pass (Args: its argument struct; pick(metric, keep): its instantiation; lds: its dynamic LDS)
template <class Args, class Pick> static void launch_exact_wide(const char* name, size_t lds, const Args& a, bool keep, hipStream_t s, Pick&& pick) {
    if (a.n == 0 || a.nblk == 0) return;
    if (a.d <= EXACT_NARROW_MAX_D || a.d > EXACT_WIDE_MAX_D || a.slab == 0 || (a.slab & (EXACT_WIDE_CHUNK - 1)) || (a.nblk & 1))
        throw std::runtime_error(std::string(name) + ": shape not supported");
    const dim3 grid((unsigned)((a.nblk + a.slab - 1) / a.slab), (unsigned)((a.n + EXACT_WIDE_QUERIES - 1) / EXACT_WIDE_QUERIES)), block(256);
    with_metric_keep(a.metric, keep, [&](auto M, auto K) {
        void (*kern)(Args) = pick(M, K);
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) throw std::runtime_error(std::string(name) + ": cannot reserve LDS: " + hipGetErrorString(e));
        LAUNCH(kern, grid, block, lds, s, a);
    });
}

void launch_scan_all_wide_f16(const ExactScanF16Args& a, bool keep, hipStream_t s) {
    launch_exact_wide("scan_all_wide_f16_kernel", EXACT_WIDE_LDS, a, keep, s, [](auto M, auto K) { return scan_all_wide_f16_kernel<decltype(M)::value, decltype(K)::value>; });
}

void launch_scan_all_wide_i8(const ExactScanArgs& a, bool keep, hipStream_t s) {
    launch_exact_wide("scan_all_wide_i8_kernel", EXACT_WIDE_I8_LDS, a, keep, s, [](auto M, auto K) { return scan_all_wide_i8_kernel<decltype(M)::value, decltype(K)::value>; });
}

void launch_exact_rescore(const ExactRescoreArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    if (a.metric == METRIC_L2) LAUNCH(exact_rescore_kernel<METRIC_L2>, dim3(a.n), dim3(256), 0, s, a);
    else LAUNCH(exact_rescore_kernel<METRIC_IP>, dim3(a.n), dim3(256), 0, s, a);
}

void launch_exact_select(const ExactSelectArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    uint32_t P = 2;
    while (P < a.cap) P <<= 1;
    if (a.rescored) LAUNCH(exact_select_kernel<true>, dim3(a.n), dim3(64), (size_t)P * 8, s, a);
    else LAUNCH(exact_select_kernel<false>, dim3(a.n), dim3(64), (size_t)P * 8, s, a);
}

}  // namespace amdivf
