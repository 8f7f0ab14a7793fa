// The matrix-core tile of the list passes (gfx950): the operand types, and the workgroup tile beyond 128 dimensions that
// scan_filter_wide_kernel (ivf_filter.hip: fp16 / fp32), scan_all_wide_f16_kernel and scan_all_wide_i8_kernel (ivf_exact.hip: fp16,
// int8) are built from.
//
// The workgroup tile.  Four waves share up to QB query blocks of 32 rows.  Wave w owns one 32-vector block of the list, whose pieces
// (1 KiB: 64 lanes x 16 bytes) stream from HBM once, straight into a register ring of SP pieces: the slot of a piece is refilled
// right behind its MFMAs, so SP KiB per wave are on their way at any time.  The query operand, which every wave needs, goes through
// LDS in stages of SP pieces, double-buffered -- s_a[2 buffers][QB][SP][lane][4] -- wave w staging the rows of query block w through
// registers: the load of the next stage in front of a stage's MFMAs, its write behind them, one LDS-only barrier per stage.
//
// STRAIGHT-LINE DISCIPLINE.  Every wave runs the same sequence of loads, stages and barriers whatever its share of the work, and
// no load sits under a condition: the compiler's wait counts are exact only in straight-line code -- with the loads under
// conditions it waited for the youngest load of the ring at every stage.  So a wave without a query block stages some valid row
// (nothing reads it), a wave without a block of the list recomputes another and drops the result, a piece index at or past J reads
// piece J - 1 and its stage slot is written as zero.  What the callers pass in (row, block, refill) must keep to that.
#pragma once
#include "ivf_dev.h"

namespace amdivf {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
// (explicitly global: a generic pointer makes these flat loads, which count on both wait counters and force full waits)
typedef const v4f __attribute__((address_space(1)))* gv4f;
typedef const v4i __attribute__((address_space(1)))* gv4i;

// workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every global load in flight (one counter for
// loads and stores on this ISA), which would drain the list prefetch ring at every stage
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// one piece of both operands into a 32 x 32 accumulator tile: HALF one v_mfma_f32_32x32x16_f16 (16 dimensions), else four
// v_mfma_f32_32x32x2_f32 (element i of both 4-vectors: k = lane half)
template <bool HALF> __device__ __forceinline__ void filter_mac(v16f& acc, const v4f& av, const v4f& bv) {
    if constexpr (HALF) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, av), __builtin_bit_cast(v8h, bv), acc, 0, 0, 0);
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], acc, 0, 0, 0);
    }
}

// 4-byte words of one buffer of the staged query operand, and the dynamic LDS of a kernel that keeps `tables` words per query behind it
constexpr size_t wide_stage_words(int QB, int SP) { return (size_t)QB * SP * 256; }
constexpr size_t wide_lds_bytes(int QB, int SP, int tables) { return (2 * wide_stage_words(QB, SP) + (size_t)tables * QB * 32) * 4; }

// The operand kinds of the tile.  word: what LDS and a piece are counted in; vec / gvec: a lane's 16 bytes of a piece; acc_t: a
// 32 x 32 accumulator tile; row: the scalar of a query row, in which a lane's pieces lie `step` apart (the filter's rows: 8 floats,
// the other lane half's 4 between them; the byte scans' rows: a lane half's pieces contiguous); mac: one piece of both operands
// into the NQB tiles.
template <bool HALF> struct TileFloat {
    typedef float word;
    typedef v4f vec;
    typedef gv4f gvec;
    typedef v16f acc_t;
    typedef float row;
    static constexpr int step = 8;
    template <int NQB> static __device__ __forceinline__ void mac(v16f* acc, const v4f (&af)[NQB], const v4f& bv) {
        if constexpr (HALF) {
#pragma unroll
            for (int q = 0; q < NQB; q++) filter_mac<true>(acc[q], af[q], bv);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int q = 0; q < NQB; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q][e], bv[e], acc[q], 0, 0, 0);
        }
    }
};
struct TileI8 {
    typedef int word;
    typedef v4i vec;
    typedef gv4i gvec;
    typedef v16i acc_t;
    typedef int8_t row;
    static constexpr int step = 16;
    // (v_mfma_i32_32x32x32_i8: 32 dimensions a piece)
    template <int NQB> static __device__ __forceinline__ void mac(v16i* acc, const v4i (&af)[NQB], const v4i& bv) {
#pragma unroll
        for (int q = 0; q < NQB; q++) acc[q] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[q], bv, acc[q], 0, 0, 0);
    }
};

// A wave's hold on the query operand of a tile of J pieces: qp = its lane's part of the row it stages; st = the staging registers,
// the caller's.  SP even: pieces are taken in pairs.
template <class OP, int SP, int QB> struct WideTile {
    typedef typename OP::vec vec;
    typedef typename OP::acc_t acc_t;
    typedef typename OP::word word;
    word* s_a;
    const typename OP::row* qp;
    int J, wave, lane;

    __device__ __forceinline__ word* slot(int buf, int qb, int jj) const { return s_a + ((size_t)(buf * QB + qb) * SP + jj) * 256 + (size_t)lane * 4; }
    // stage s of this wave's row: global -> registers ...
    __device__ __forceinline__ void stage_load(int s, vec (&st)[SP]) const {
#pragma unroll
        for (int jj = 0; jj < SP; jj++) {
            const int j = s * SP + jj;
            st[jj] = *(typename OP::gvec)(uintptr_t)(qp + OP::step * (j < J ? j : J - 1));
        }
    }
    // ... -> LDS buffer `buf` (pieces that pad the last stage contribute 0 x y)
    __device__ __forceinline__ void stage_write(int s, int buf, const vec (&st)[SP]) const {
#pragma unroll
        for (int jj = 0; jj < SP; jj++) *reinterpret_cast<vec*>(slot(buf, wave, jj)) = s * SP + jj < J ? st[jj] : vec{};
    }
    template <int NQB> __device__ __forceinline__ void load_a(int buf, int jj, vec (&af)[NQB]) const {
#pragma unroll
        for (int q = 0; q < NQB; q++) af[q] = *reinterpret_cast<const vec*>(slot(buf, q, jj));
    }
    // One stage: the SP pieces of stage s in LDS buffer `buf` times ring slots br[0 .. SP) into the NQB accumulator tiles, stage sn
    // loaded in front and written to the other buffer behind (last read one stage ago: every wave is past that barrier), then the
    // barrier.  The operands of an even and an odd piece are read from LDS one MFMA group ahead.  refill(j, jj, br[jj]) requests what
    // ring slot jj holds next, right behind the MFMAs of piece j = s SP + jj; the scheduling barriers keep every load where it is written.
    // (buf comes first on purpose: arguments are evaluated left to right, and the filter's kernels compile to what they were before
    // this header existed only with `s & 1` ahead of `s + 1`: DESIGN.md 13.3)
    template <int NQB, class Refill> __device__ __forceinline__ void stage(int buf, int s, int sn, vec (&st)[SP], acc_t* acc, vec (&br)[SP], Refill&& refill) const {
        vec afA[NQB], afB[NQB];
        stage_load(sn, st);
#pragma unroll
        for (int jj = 0; jj < SP; jj += 2) {
            const int j = s * SP + jj;
            if (jj == 0) load_a(buf, 0, afA);
            load_a(buf, jj + 1, afB);
            __builtin_amdgcn_sched_barrier(0);
            OP::template mac<NQB>(acc, afA, br[jj]);
            __builtin_amdgcn_sched_barrier(0);
            refill(j, jj, br[jj]);
            if (jj + 2 < SP) load_a(buf, jj + 2, afA);
            __builtin_amdgcn_sched_barrier(0);
            OP::template mac<NQB>(acc, afB, br[jj + 1]);
            __builtin_amdgcn_sched_barrier(0);
            refill(j + 1, jj + 1, br[jj + 1]);
        }
        stage_write(sn, buf ^ 1, st);
        lds_barrier();
    }
};

}  // namespace amdivf
