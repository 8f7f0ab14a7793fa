// gfx950 (MI355X, CDNA4): the nearest centroid of every row in one fused matrix-core pass.
//
// Index::assign is a ranking of length one.  coarse_dev serves it as any other ranking: every exact distance to HBM (n x nlist
// floats), then a heap of one that reads them back.  An arg-min needs neither: a row needs one running minimum, and the exact
// answer needs only the few centroids whose approximate value lies within the known error bound of that minimum.
//
//   assign_min_kernel      x.c of 32 rows x 32 centroids per v_mfma_f32_32x32x16_f16 chain on scaled fp16 operands (the operands
//                          and the error constant of coarse_gemm16_kernel / ivf_filter.hip's fp16 form), nothing stored but, per
//                          row, the <= ASSIGN_CAND centroids that can be the exact nearest;
//   assign_rescore_kernel  those candidates' distances in the reference's rounding sequence (four lanes a candidate), the best
//                          (distance, centroid) per row, the lowest centroid number between bit-equal distances -- what the
//                          reference's heap of one, which admits only a strictly better value, keeps.
// Rows the pass cannot decide -- more candidates than slots, a candidate distance that is not finite, a row without a usable fp16
// scale -- are FLAGGED and listed; the caller sends them through coarse_dev (ivf_engine.hip: assign_fused).  Beyond 128 dimensions
// assign_rows16_kernel + assign_wide_kernel (below) take assign_min_kernel's place; the table and the rescoring are the same.
//
// Split of work.  A workgroup of four waves owns 4 x QB x 32 rows for the whole sweep over the centroids.  A wave's rows are read
// once, scaled and rounded to fp16 and kept in registers as the N operand (JP pieces of 4 VGPRs per 32-row block).  The centroid
// table, laid out once per centroid set in fragment order (launch_assign_table: a block of 32 centroids = JP pieces of 64 lanes x
// 16 bytes, then the 32 terms |c|^2), streams through LDS, double-buffered, one fetch of a block for all four waves, one LDS-only
// barrier a block.  The centroids are the M operand: a lane's 16 accumulators are then 16 centroids of ONE row (lane l: row
// l & 31, centroids (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the block), so a row's running minimum is one register of its two lanes
// and the only cross-lane step is the merge of the two lane halves behind the sweep.
//
// The ranked value drops the row's constant: v = |c|^2 - 2 x.c (L2), v = -x.c (inner product), one fma on the accumulator.
//
// Candidates.  Two identical sweeps.  The first leaves m = min v.  With r_c the reference's distance and eps the bound on
// |v_c + |x|^2 - r_c| (L2: C16 (|x|^2 + max |c|^2); inner product, on -r_c: C16 |x| max |c|; C16 = (2 d + 32) 2^-24 + 2^-10 + 2^-12,
// ivf_filter.hip's head comment), let c* be ANY centroid of least reference distance and a the arg-min of v:
//     v_c* + |x|^2 <= r_c* + eps <= r_a + eps <= v_a + |x|^2 + 2 eps,   i.e.   v_c* <= m + 2 eps.
// The second sweep emits every centroid with v <= m + 2.125 eps (the eighth covers the rounding of the sum itself: |m| <= 2 S and
// eps >= 34 u S) into the row's slots, an LDS counter per row handing them out: a superset of all centroids of least reference
// distance, the lowest-numbered one included.  The second sweep recomputes the products (cheap here) instead of keeping lane-private
// lists, so the loop stays straight-line (mfma_tile.h: no load under a condition) and the first sweep keeps no centroid number at all.
//
// Scales.  The centroids' scale is the table's one power of two (half_scale_of on the range launch_amax left in d_cinfo).  A row
// is ranked on its own, so it takes its OWN power of two (largest magnitude into [2^14, 2^15), the rule of half_scale_of applied to
// the one row: the bound's condition that no row be tiny beside its matrix's largest holds by construction), and a row with a NaN,
// an infinity or a magnitude outside 2^+-24 costs only itself a trip through the exact path.  Within those magnitudes nothing on
// the way overflows and every norm is inside the range the bound assumes (ivf_filter.hip: FILTER_TINY / FILTER_HUGE).
#include "ivf_dev.h"
#include "mfma_tile.h"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace amdivf {

constexpr uint32_t ASSIGN_FLAG = 0xffffffffu;  // a row's candidate count: the row has no usable scale

// ---------------------------------------------------------------------------------------------
// centroid rows (stride dpad) -> blocks of JP pieces (lane (v = l & 31, h = l >> 5) of piece j: elements 16 j + 8 h .. + 7 of
// centroid 32 b + v as fp16(sy * value), zero beyond d) followed by the block's 32 terms: |c|^2 accumulated in double and rounded
// once (L2), 0 (inner product), +inf for the centroids that pad the last block (never a minimum, never a candidate).  One wave a block.
__global__ __launch_bounds__(64) void assign_table_kernel(const float* centroids, uint32_t nlist, int d, int dpad, int metric, float sy, int JP,
                                                          float* table) {
    const int lane = threadIdx.x, v = lane & 31, h = lane >> 5;
    const uint32_t c = blockIdx.x * 32 + v;
    const bool ok = c < nlist;
    const float* src = centroids + (size_t)(ok ? c : 0) * dpad;
    float* blk = table + (size_t)blockIdx.x * (JP * 256 + 32);
    double sq = 0.0;
    for (int j = 0; j < JP; j++) {
        v8h piece;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            const int col = 16 * j + 8 * h + w;
            const float val = ok && col < d ? src[col] : 0.f;
            piece[w] = (_Float16)(val * sy);
            sq += (double)val * (double)val;
        }
        *reinterpret_cast<v8h*>(blk + j * 256 + lane * 4) = piece;
    }
    sq += __shfl_xor(sq, 32);
    if (h == 0) blk[JP * 256 + v] = !ok ? __builtin_inff() : metric == METRIC_L2 ? (float)sq : 0.f;
}
uint32_t assign_pieces(int d) { return ((uint32_t)(d + 15) / 16 + 1u) & ~1u; }
size_t assign_table_bytes(uint32_t nlist, int d) { return (size_t)((nlist + 31) / 32) * (assign_pieces(d) * 256 + 32) * sizeof(float); }
void launch_assign_table(const float* centroids, uint32_t nlist, int d, int dpad, int metric, float sy, float* table, hipStream_t s) {
    LAUNCH(assign_table_kernel, dim3((nlist + 31) / 32), dim3(64), 0, s, centroids, nlist, d, dpad, metric, sy, (int)assign_pieces(d), table);
}

// ---------------------------------------------------------------------------------------------
// the fused pass: cnt[row] = the row's candidates (more than ASSIGN_CAND: the first ASSIGN_CAND to arrive are in cand, the row is
// the rescoring's to flag) or ASSIGN_FLAG
template <int METRIC, int JP, int QB> __global__ __launch_bounds__(256) void assign_min_kernel(AssignArgs a) {
    constexpr int NV = JP * 64 + 8;  // 16-byte vectors of a block of the table
    constexpr int NL = (NV + 255) / 256;
    __shared__ v4f s_blk[2][NV];
    __shared__ uint32_t s_cnt[4 * QB * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane & 31, hh = lane >> 5;
    const uint32_t nblk = (a.nlist + 31) / 32;
    const gv4f table = (gv4f)(uintptr_t)a.table;

    // a block of the table: global -> registers -> LDS, every thread the same NL loads (the last ones of a block past its end
    // read its last vector again and are not written)
    v4f st[NL];
    auto fetch = [&](uint32_t b) {
#pragma unroll
        for (int i = 0; i < NL; i++) {
            const int idx = tid + 256 * i;
            st[i] = table[(size_t)b * NV + (idx < NV ? idx : NV - 1)];
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NL; i++) {
            const int idx = tid + 256 * i;
            if (idx < NV) s_blk[buf][idx] = st[i];
        }
    };
    fetch(0);

    // the wave's rows: range, scale, |x|^2, fp16 pieces.  Rows past the end are the last row again (nothing of them is written).
    v8h xq[QB][JP];
    float mul[QB], xn[QB];
    bool bad[QB], live[QB];
    size_t row[QB];
#pragma unroll
    for (int qb = 0; qb < QB; qb++) {
        const size_t r = (((size_t)blockIdx.x * 4 + wave) * QB + qb) * 32 + q;
        live[qb] = r < a.n;
        row[qb] = live[qb] ? r : a.n - 1;
        const float* xr = a.x + row[qb] * (size_t)a.dpad;
        v4f raw[JP][2];
#pragma unroll
        for (int j = 0; j < JP; j++)
#pragma unroll
            for (int w = 0; w < 2; w++) {
                const int col = 16 * j + 8 * hh + 4 * w;  // (dpad % 4 == 0: four columns are inside the row or outside together)
                const v4f t = *(gv4f)(uintptr_t)(xr + (col < a.dpad ? col : 0));
                raw[j][w] = col < a.dpad ? t : v4f{0.f, 0.f, 0.f, 0.f};
            }
        uint32_t mx = 0;
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < JP; j++)
#pragma unroll
            for (int w = 0; w < 2; w++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float val = raw[j][w][e], av = fabsf(val);
                    const uint32_t bits = av == av ? __float_as_uint(av) : 0x7f800000u;  // (a NaN counts as an infinity)
                    mx = bits > mx ? bits : mx;
                    sq = __builtin_fmaf(val, val, sq);
                }
        const uint32_t mo = (uint32_t)__shfl_xor((int)mx, 32);
        mx = mo > mx ? mo : mx;
        sq += __shfl_xor(sq, 32);
        // largest magnitude in [2^(e-1), 2^e), e = be - 126: usable for -24 <= e <= 24, scale 2^(15 - e); a row of zeros is held as it is
        const uint32_t be = mx >> 23;
        bad[qb] = mx != 0 && (be < 102u || be > 150u);
        const float sx = mx == 0 ? 1.f : __uint_as_float((268u - be) << 23), inv_sx = mx == 0 ? 1.f : __uint_as_float((be - 14u) << 23);
        const float ps = inv_sx * a.inv_sy;  // (powers of two: exact)
        mul[qb] = bad[qb] ? 0.f : METRIC == METRIC_L2 ? -2.f * ps : -ps;
        xn[qb] = sq;
#pragma unroll
        for (int j = 0; j < JP; j++)
#pragma unroll
            for (int w = 0; w < 2; w++)
#pragma unroll
                for (int e = 0; e < 4; e++) xq[qb][j][4 * w + e] = bad[qb] ? (_Float16)0.f : (_Float16)(raw[j][w][e] * sx);
    }

    for (int i = tid; i < 4 * QB * 32; i += 256) s_cnt[i] = 0;
    stage(0);
    __syncthreads();

    float mn[QB], thr[QB];
#pragma unroll
    for (int qb = 0; qb < QB; qb++) mn[qb] = __builtin_inff(), thr[qb] = -__builtin_inff();

    // one sweep over the table; `it` counts the blocks of both sweeps (the LDS buffer of a block is it & 1), and the last block of a
    // sweep fetches the first again: the second sweep starts on a full pipeline, the last fetch of all is read by nobody
    uint32_t it = 0;
    auto sweep = [&](auto emit) {
        constexpr bool EMIT = decltype(emit)::value;
        for (uint32_t b = 0; b < nblk; b++, it++) {
            const int buf = (int)(it & 1u);
            fetch(b + 1 < nblk ? b + 1 : 0);
            const v4f* blk = s_blk[buf];
            v16f acc[QB];
#pragma unroll
            for (int qb = 0; qb < QB; qb++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[qb][r] = 0.f;
#pragma unroll
            for (int j = 0; j < JP; j++) {
                const v8h cf = __builtin_bit_cast(v8h, blk[j * 64 + lane]);
#pragma unroll
                for (int qb = 0; qb < QB; qb++) acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cf, xq[qb][j], acc[qb], 0, 0, 0);
            }
            v4f term[4];  // of this lane's centroids 8 g + 4 hh .. + 3
#pragma unroll
            for (int g = 0; g < 4; g++) term[g] = blk[JP * 64 + 2 * g + hh];
#pragma unroll
            for (int qb = 0; qb < QB; qb++) {
                float v[16];
#pragma unroll
                for (int r = 0; r < 16; r++) v[r] = __builtin_fmaf(mul[qb], acc[qb][r], term[r >> 2][r & 3]);
                float bm = v[0];
#pragma unroll
                for (int r = 1; r < 16; r++) bm = __builtin_fminf(bm, v[r]);
                if constexpr (!EMIT) {
                    mn[qb] = __builtin_fminf(mn[qb], bm);
                } else if (bm <= thr[qb]) {  // (rare: a block that holds a candidate of this row)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const uint32_t c = b * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                        if (v[r] <= thr[qb] && c < a.nlist) {
                            const uint32_t slot = atomicAdd(&s_cnt[(wave * QB + qb) * 32 + q], 1u);
                            if (slot < ASSIGN_CAND && live[qb]) a.cand[row[qb] * ASSIGN_CAND + slot] = c;
                        }
                    }
                }
            }
            stage(buf ^ 1);  // (last read one block ago: every wave is past that barrier)
            lds_barrier();
        }
    };
    sweep(std::false_type{});
#pragma unroll
    for (int qb = 0; qb < QB; qb++) {
        const float m = __builtin_fminf(mn[qb], __shfl_xor(mn[qb], 32));
        const float eps = METRIC == METRIC_L2 ? a.C * (xn[qb] + a.cmax) : a.C * sqrtf(xn[qb]) * sqrtf(a.cmax);
        const float t = m + 2.125f * eps;
        bad[qb] = bad[qb] || !(fabsf(t) < 3.0e38f);
        thr[qb] = bad[qb] ? -__builtin_inff() : t;
    }
    sweep(std::true_type{});
#pragma unroll
    for (int qb = 0; qb < QB; qb++)
        if (hh == 0 && live[qb]) a.cnt[row[qb]] = bad[qb] ? ASSIGN_FLAG : s_cnt[(wave * QB + qb) * 32 + q];
}

template <int METRIC, int QB> static void launch_assign_min_jp(const AssignArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.n + 128 * QB - 1) / (128 * QB)));
    switch (assign_pieces(a.d)) {
        case 2: LAUNCH((assign_min_kernel<METRIC, 2, QB>), grid, dim3(256), 0, s, a); break;
        case 4: LAUNCH((assign_min_kernel<METRIC, 4, QB>), grid, dim3(256), 0, s, a); break;
        case 6: LAUNCH((assign_min_kernel<METRIC, 6, QB>), grid, dim3(256), 0, s, a); break;
        default: LAUNCH((assign_min_kernel<METRIC, 8, QB>), grid, dim3(256), 0, s, a); break;
    }
}
void launch_assign_min(const AssignArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    if (a.metric == METRIC_L2) launch_assign_min_jp<METRIC_L2, ASSIGN_QB>(a, s);
    else launch_assign_min_jp<METRIC_IP, ASSIGN_QB>(a, s);
}

// ---------------------------------------------------------------------------------------------
// Beyond 128 dimensions (option "assign_wide").  At J = assign_pieces(d) = 10 .. 64 pieces a wave cannot keep its
// rows' fragments in registers (64 pieces x 4 VGPRs x QB), so the roles of assign_min_kernel's two operands in memory are swapped:
// the ROWS are laid out as fragments, once per chunk of the call, and go through LDS; the centroid table streams into registers.
//
//   assign_rows16_kernel  a wave per block of 32 rows: the row's power of two, |x|^2 and the bad flag exactly as assign_min_kernel
//                         computes them (the same lanes hold the same columns, the same fma chain), into an AssignRowRec; the
//                         row as J pieces of 64 lanes x 16 bytes in the table's fragment order.  The rows are read twice (range,
//                         then conversion): J x 8 floats a lane do not fit registers either.  Rows that pad the last workgroup's
//                         128 are the chunk's last row again, so that every block a workgroup stages holds valid data.
//   assign_wide_kernel    <METRIC, EMIT>, launched twice per chunk, on mfma_tile.h's WideTile: a workgroup owns 4 x 32 rows for the
//                         whole sweep; tile t is centroid blocks 4 t .. 4 t + 3, wave w owns block 4 t + w, which streams from the
//                         table into its ring of SP pieces (a slot refilled right behind its MFMAs; behind a tile's last stage
//                         with the first pieces of the wave's block of the NEXT tile); the workgroup's rows go through LDS in
//                         stages of SP pieces, double-buffered, wave w staging row block w, one lds_barrier() a stage; the stages
//                         do not depend on the tile, so the buffers alternate along the whole sweep.  Straight-line code: a wave
//                         whose block lies past the table recomputes the tile's first and drops the result, pieces at or past J
//                         are staged as zero.  The tile epilogue is assign_min_kernel's, with the row's multiplier and threshold
//                         read from two LDS tables.  EMIT = false leaves every row's minimum in wmin (the lane halves joined by a
//                         shuffle, the four waves -- which saw different centroids of the same rows -- through LDS); EMIT = true
//                         hands out the row's candidate slots through ONE LDS counter per row, shared by the four waves.
// The bound is the narrow pass's at this d: C16 grows with d (exact_float_constant), nothing else changes -- DESIGN.md 18.1 says why
// no partial sum overflows and why the eighth of eps still covers the rounding of the sum at 1024 products.
#ifndef AUNCEL_ASSIGN_WIDE_SP
#define AUNCEL_ASSIGN_WIDE_SP 6  // (as AUNCEL_EXACT_WIDE_SP, ivf_exact.hip)
#endif
constexpr int ASSIGN_WIDE_SP = AUNCEL_ASSIGN_WIDE_SP;
constexpr int ASSIGN_WIDE_QB = (int)(ASSIGN_WIDE_ROWS / 32);
constexpr size_t ASSIGN_WIDE_LDS = wide_lds_bytes(ASSIGN_WIDE_QB, ASSIGN_WIDE_SP, 3);  // (the stages + multiplier, threshold and counter per row)
static_assert(ASSIGN_WIDE_QB == 4, "wave w stages row block w");
static_assert(ASSIGN_WIDE_SP >= 2 && ASSIGN_WIDE_SP % 2 == 0 && ASSIGN_WIDE_SP <= 10, "pieces are taken in pairs; a stage is not longer than the fewest pieces");
static_assert(2 * ASSIGN_WIDE_LDS <= 160 * 1024, "two workgroups per compute unit");

__global__ __launch_bounds__(256) void assign_rows16_kernel(AssignArgs a, int J) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane & 31, hh = lane >> 5;
    const size_t blk = (size_t)blockIdx.x * 4 + wave, r = blk * 32 + q;
    const float* xr = a.x + (r < a.n ? r : a.n - 1) * (size_t)a.dpad;
    // the lane's eight columns of piece j (dpad % 4 == 0: four columns are inside the row or outside together)
    auto load = [&](int j, int w) {
        const int col = 16 * j + 8 * hh + 4 * w;
        const v4f t = *(gv4f)(uintptr_t)(xr + (col < a.dpad ? col : 0));
        return col < a.dpad ? t : v4f{0.f, 0.f, 0.f, 0.f};
    };
    uint32_t mx = 0;
    float sq = 0.f;
    for (int j = 0; j < J; j++)
#pragma unroll
        for (int w = 0; w < 2; w++) {
            const v4f raw = load(j, w);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float val = raw[e], av = fabsf(val);
                const uint32_t bits = av == av ? __float_as_uint(av) : 0x7f800000u;  // (a NaN counts as an infinity)
                mx = bits > mx ? bits : mx;
                sq = __builtin_fmaf(val, val, sq);
            }
        }
    const uint32_t mo = (uint32_t)__shfl_xor((int)mx, 32);
    mx = mo > mx ? mo : mx;
    sq += __shfl_xor(sq, 32);
    // (assign_min_kernel's rule: largest magnitude in [2^(e-1), 2^e), e = be - 126, usable for -24 <= e <= 24, scale 2^(15 - e))
    const uint32_t be = mx >> 23;
    const bool bad = mx != 0 && (be < 102u || be > 150u);
    const float sx = mx == 0 ? 1.f : __uint_as_float((268u - be) << 23), inv_sx = mx == 0 ? 1.f : __uint_as_float((be - 14u) << 23);
    const float ps = inv_sx * a.inv_sy;  // (powers of two: exact)
    float* out = a.rows16 + blk * (size_t)J * 256 + (size_t)lane * 4;
    for (int j = 0; j < J; j++) {
        v8h piece;
#pragma unroll
        for (int w = 0; w < 2; w++) {
            const v4f raw = load(j, w);
#pragma unroll
            for (int e = 0; e < 4; e++) piece[4 * w + e] = bad ? (_Float16)0.f : (_Float16)(raw[e] * sx);
        }
        *reinterpret_cast<v8h*>(out + (size_t)j * 256) = piece;
    }
    if (hh == 0) a.rec[r] = AssignRowRec{sq, bad ? 0.f : a.metric == METRIC_L2 ? -2.f * ps : -ps, bad ? 1u : 0u, 0u};
}

template <int METRIC, bool EMIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void assign_wide_kernel(AssignArgs a, int J) {
    constexpr int QB = ASSIGN_WIDE_QB, SP = ASSIGN_WIDE_SP;
    extern __shared__ __align__(16) unsigned char assign_wide_smem[];
    float* s_a = reinterpret_cast<float*>(assign_wide_smem);  // [2 buffers][row block][piece of the stage][lane][4]
    float* s_mul = s_a + 2 * wide_stage_words(QB, SP);
    float* s_thr = s_mul + ASSIGN_WIDE_ROWS;
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_thr + ASSIGN_WIDE_ROWS);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane & 31, hh = lane >> 5;
    const int S = (J + SP - 1) / SP;
    const uint32_t nblk = (a.nlist + 31) / 32, ntile = (nblk + 3) / 4;
    const size_t block_floats = (size_t)J * 256 + 32;  // of the table: the pieces, then the 32 terms
    const size_t rbase = (size_t)blockIdx.x * ASSIGN_WIDE_ROWS;

    // ---- per row of the workgroup, once: multiplier, threshold, counter (slot = thread & 127: the upper two waves write what the
    // lower two write).  A row past n is the copy of a valid one and is never written out; nothing of it may take a slot.
    const uint32_t sl = threadIdx.x & (ASSIGN_WIDE_ROWS - 1);
    const bool slive = rbase + sl < a.n;
    const AssignRowRec rec = a.rec[rbase + sl];
    bool sbad = rec.bad != 0;
    s_mul[sl] = rec.mul;
    s_cnt[sl] = 0;
    if constexpr (EMIT) {
        const float m = a.wmin[rbase + sl];
        const float eps = METRIC == METRIC_L2 ? a.C * (rec.xn + a.cmax) : a.C * sqrtf(rec.xn) * sqrtf(a.cmax);
        const float t = m + 2.125f * eps;
        sbad = sbad || !(fabsf(t) < 3.0e38f);
        s_thr[sl] = sbad || !slive ? -__builtin_inff() : t;
    }
    // ---- the row operand: this wave stages row block `wave` of the workgroup's four
    const WideTile<TileAssign, SP, QB> tile{s_a, a.rows16 + (rbase / 32 + (size_t)wave) * (size_t)J * 256 + (size_t)lane * 4, J, wave, lane};
    v4f st[SP];
    tile.stage_load(0, st);
    tile.stage_write(0, 0, st);
    // ---- this wave's centroid block, a ring of SP pieces (a block past the table: the tile's first again)
    const float* fbase = a.table + (size_t)lane * 4;
    auto wave_block = [&](uint32_t t) { return 4 * t + (uint32_t)wave < nblk ? 4 * t + (uint32_t)wave : 4 * t; };
    v4f br[SP];
    {
        const float* b0 = fbase + wave_block(0) * block_floats;
#pragma unroll
        for (int jj = 0; jj < SP; jj++) br[jj] = *(gv4f)(uintptr_t)(b0 + (size_t)jj * 256);  // (SP <= 10 <= J)
    }
    lds_barrier();  // stage 0 and the per-row tables are in LDS

    float mn[QB];
#pragma unroll
    for (int qb = 0; qb < QB; qb++) mn[qb] = __builtin_inff();
    int buf = 0;
    for (uint32_t t = 0; t < ntile; t++) {
        const bool active = 4 * t + (uint32_t)wave < nblk;
        const uint32_t cur = wave_block(t);
        const float* bbase = fbase + cur * block_floats;
        const float* nbase = fbase + wave_block(t + 1 < ntile ? t + 1 : t) * block_floats;  // (no next tile: this one again, never used)
        v4f term[4];  // of this lane's centroids 8 g + 4 hh .. + 3
#pragma unroll
        for (int g = 0; g < 4; g++) term[g] = *(gv4f)(uintptr_t)(a.table + cur * block_floats + (size_t)J * 256 + (size_t)(2 * g + hh) * 4);
        v16f acc[QB];
#pragma unroll
        for (int qb = 0; qb < QB; qb++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[qb][r] = 0.f;
        for (int s = 0; s < S; s++) {
            const bool lasts = s + 1 == S;
            // the refill of ring slot jj: piece j + SP of this block (past J: J - 1 again, multiplied by a zero stage slot), or behind
            // the last stage piece jj of the wave's block of the next tile
            auto refill = [&](int j, int jj, v4f& bv) __attribute__((always_inline)) {
                const float* src = lasts ? nbase + (size_t)jj * 256 : bbase + (size_t)(j + SP < J ? j + SP : J - 1) * 256;
                bv = *(gv4f)(uintptr_t)src;
            };
            tile.template stage<QB>(buf, s, lasts ? 0 : s + 1, st, acc, br, refill);  // (behind a tile's last stage: stage 0, for the next tile)
            buf ^= 1;
        }
        // ---- epilogue: register r of lane (q, hh) of tile qb is centroid (r & 3) + 8 (r >> 2) + 4 hh of the block, row 32 qb + q
#pragma unroll
        for (int qb = 0; qb < QB; qb++) {
            const float mul = s_mul[32 * qb + q];
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; r++) v[r] = __builtin_fmaf(mul, acc[qb][r], term[r >> 2][r & 3]);
            float bm = v[0];
#pragma unroll
            for (int r = 1; r < 16; r++) bm = __builtin_fminf(bm, v[r]);
            if constexpr (!EMIT) {
                mn[qb] = __builtin_fminf(mn[qb], active ? bm : __builtin_inff());
            } else {
                const float thr = s_thr[32 * qb + q];
                if (active && bm <= thr) {  // (rare: a block that holds a candidate of this row)
                    const size_t row = rbase + 32 * qb + q;
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const uint32_t c = cur * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                        if (v[r] <= thr && c < a.nlist) {
                            const uint32_t slot = atomicAdd(&s_cnt[32 * qb + q], 1u);
                            if (slot < ASSIGN_CAND && row < a.n) a.cand[row * ASSIGN_CAND + slot] = c;
                        }
                    }
                }
            }
        }
    }
    if constexpr (!EMIT) {
        // the stage buffers are free behind the sweep's last barrier: [wave][row] minima
#pragma unroll
        for (int qb = 0; qb < QB; qb++) {
            const float m = __builtin_fminf(mn[qb], __shfl_xor(mn[qb], 32));
            if (hh == 0) s_a[wave * (int)ASSIGN_WIDE_ROWS + 32 * qb + q] = m;
        }
        __syncthreads();
        if (threadIdx.x < ASSIGN_WIDE_ROWS && slive) {
            float m = s_a[sl];
#pragma unroll
            for (int w = 1; w < 4; w++) m = __builtin_fminf(m, s_a[w * (int)ASSIGN_WIDE_ROWS + sl]);
            a.wmin[rbase + sl] = m;
        }
    } else {
        __syncthreads();
        if (threadIdx.x < ASSIGN_WIDE_ROWS && slive) a.cnt[rbase + sl] = sbad ? ASSIGN_FLAG : s_cnt[sl];
    }
}

size_t assign_wide_chunk_rows(int d) {
    return ASSIGN_WIDE_WORKSPACE / ((size_t)assign_pieces(d) * 32) / ASSIGN_WIDE_ROWS * ASSIGN_WIDE_ROWS;  // (32 bytes a piece and row)
}
template <int METRIC, bool EMIT> static void launch_assign_wide_sweep(const AssignArgs& a, int J, hipStream_t s) {
    void (*kern)(AssignArgs, int) = assign_wide_kernel<METRIC, EMIT>;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ASSIGN_WIDE_LDS);
    if (e != hipSuccess) throw std::runtime_error(std::string("assign_wide_kernel: cannot reserve LDS: ") + hipGetErrorString(e));
    LAUNCH(kern, dim3((unsigned)((a.n + ASSIGN_WIDE_ROWS - 1) / ASSIGN_WIDE_ROWS)), dim3(256), ASSIGN_WIDE_LDS, s, a, J);
}
void launch_assign_wide(const AssignArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    const int J = (int)assign_pieces(a.d);
    if (a.dpad <= ASSIGN_MAX_DPAD || a.dpad > ASSIGN_WIDE_MAX_DPAD || a.n > assign_wide_chunk_rows(a.d)) throw std::runtime_error("assign_wide_kernel: shape not supported");
    LAUNCH(assign_rows16_kernel, dim3((unsigned)((a.n + ASSIGN_WIDE_ROWS - 1) / ASSIGN_WIDE_ROWS)), dim3(256), 0, s, a, J);
    if (a.metric == METRIC_L2) {
        launch_assign_wide_sweep<METRIC_L2, false>(a, J, s);
        launch_assign_wide_sweep<METRIC_L2, true>(a, J, s);
    } else {
        launch_assign_wide_sweep<METRIC_IP, false>(a, J, s);
        launch_assign_wide_sweep<METRIC_IP, true>(a, J, s);
    }
}

// ---------------------------------------------------------------------------------------------
// The candidates' distances in the reference's sequence (utils_simd.cpp:391-443: four running sums over the elements 4 i + l, each
// accumulated in order, then (s0 + s1) + (s2 + s3)): four neighbouring lanes take one candidate, lane l its sum l, eight steps of
// the chain requested per trip (coarse_pick_kernel's scheme); 32 lanes a row, the row's ASSIGN_CAND candidates side by side, and the
// best of them by (order key of the distance, centroid number) -- between bit-equal distances the lowest number.  stat[0] += the
// flagged rows (listed in flagged[]), stat[2..3] (64 bits) += the candidates recomputed: one atomic per wave of a resident grid.
template <int METRIC> __global__ __launch_bounds__(256) void assign_rescore_kernel(AssignArgs a) {
    constexpr bool Ascending = METRIC == METRIC_L2;
    const uint32_t tid = threadIdx.x, g = tid & 31, k = g >> 2, sub = g & 3;
    uint32_t done = 0;
    for (size_t r0 = (size_t)blockIdx.x * 8; r0 < a.n; r0 += (size_t)gridDim.x * 8) {
        const size_t row = r0 + (tid >> 5);
        const bool live = row < a.n;
        const uint32_t cn = live ? a.cnt[row] : 0u;
        const bool undecided = cn == 0u || cn > ASSIGN_CAND;  // (ASSIGN_FLAG included; no candidate at all cannot be, and is not trusted)
        const bool have = !undecided && k < cn;
        const uint32_t c = have ? a.cand[row * ASSIGN_CAND + k] : 0u;
        float sl = 0.f;
        if (have) {
            const float* xr = a.x + row * (size_t)a.dpad;
            const float* y = a.centroids + (size_t)c * a.dpad;
            int e = (int)sub;
            for (; e + 28 < a.dpad; e += 32) {
                float yv[8], xv[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    yv[u] = y[e + 4 * u];
                    xv[u] = xr[e + 4 * u];
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    if (METRIC == METRIC_L2) {
                        const float t = yv[u] - xv[u];
                        sl += t * t;
                    } else {
                        sl += yv[u] * xv[u];
                    }
                }
            }
            for (; e < a.dpad; e += 4) {
                if (METRIC == METRIC_L2) {
                    const float t = y[e] - xr[e];
                    sl += t * t;
                } else {
                    sl += y[e] * xr[e];
                }
            }
        }
        const float pair = sl + __shfl_xor(sl, 1);    // lanes 0/1: s0 + s1, lanes 2/3: s2 + s3 (the sum is commutative bit for bit)
        const float ex = pair + __shfl_xor(pair, 2);  // (s0 + s1) + (s2 + s3)
        const bool wild = have && !(fabsf(ex) < 3.0e38f);  // NaN, an infinity, FLT_MAX: what the reference's heap does with them is the exact path's to say
        unsigned long long best = have ? ((unsigned long long)(Ascending ? fkey(ex) : ~fkey(ex)) << 32) | c : ~0ull;
#pragma unroll
        for (int off = 4; off < 32; off <<= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o < best ? o : best;
        }
        const uint32_t wild_rows = (uint32_t)(__ballot(wild) >> (tid & 32u));  // (this row's 32 lanes)
        if (g == 0 && live) {
            if (undecided || wild_rows) {
                a.flagged[atomicAdd(&a.stat[0], 1u)] = (uint32_t)row;
            } else {
                const uint32_t kk = (uint32_t)(best >> 32);
                a.out_dis[row] = fkey_inv(Ascending ? kk : ~kk);
                a.out_keys[row] = (int64_t)(uint32_t)best;
            }
        }
        done += have && sub == 0;
    }
    done = wave_sum_u32(done);
    if ((tid & 63u) == 0 && done) atomicAdd(reinterpret_cast<unsigned long long*>(a.stat + 2), (unsigned long long)done);
}
void launch_assign_rescore(const AssignArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    const dim3 grid((unsigned)std::min<size_t>((a.n + 7) / 8, 4096));
    if (a.metric == METRIC_L2) LAUNCH(assign_rescore_kernel<METRIC_L2>, grid, dim3(256), 0, s, a);
    else LAUNCH(assign_rescore_kernel<METRIC_IP>, grid, dim3(256), 0, s, a);
}

}  // namespace amdivf
