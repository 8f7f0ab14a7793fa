// Device-side data structures and kernel launch wrappers of the gfx950 IVF-Flat engine.
// (internal: the public boundary is include/auncel_amd.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <stdexcept>
#include <string>

#include "query_range.h"
#include "selector_args.h"

namespace amdivf {

// A launch the runtime rejects (grid, LDS or register limits) leaves nothing on the stream, and the later synchronisation
// succeeds: without this check a search would return untouched output buffers as if they were results.
inline void check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw std::runtime_error(std::string("kernel launch failed: ") + what + ": " + hipGetErrorString(e));
    // AUNCEL_AMD_SYNC_LAUNCH=1 (debugging): name every launch and wait for it, so that a device fault points at its kernel
    static const bool sync_each = getenv("AUNCEL_AMD_SYNC_LAUNCH") != nullptr;
    if (sync_each) {
        fprintf(stderr, "[launch] %.100s\n", what);
        const hipError_t s = hipDeviceSynchronize();
        if (s != hipSuccess) throw std::runtime_error(std::string("kernel failed: ") + what + ": " + hipGetErrorString(s));
    }
}
// (the error state is per thread and sticky: an unrelated earlier call, e.g. the elapsed time of an event pair that was
// never recorded, must not be taken for this launch's)
#define LAUNCH(...)                     \
    do {                                \
        (void)hipGetLastError();        \
        hipLaunchKernelGGL(__VA_ARGS__); \
        ::amdivf::check_launch(#__VA_ARGS__); \
    } while (0)

constexpr int METRIC_IP = 0;
constexpr int METRIC_L2 = 1;

// ---------------------------------------------------------------------------- distance tiles
// One workgroup (256 threads = 4 waves) computes the distances between up to QG*RQ queries and
// up to (4/QG)*64*RV consecutive vectors of one inverted list (or of the centroid table).
constexpr int SCAN_RQ = 8;    // queries per wave (query operands live in SGPRs)
constexpr int SCAN_RV = 2;    // vectors per lane
#ifndef AUNCEL_SCAN_DC
#define AUNCEL_SCAN_DC 16
#endif
constexpr int SCAN_DC = AUNCEL_SCAN_DC;   // dimensions staged through LDS per step
constexpr int SCAN_WAVE_VECS = 64 * SCAN_RV;

// fp32 tiles: vec_base carries two numbers -- bits 0..39 the global index of the tile's first vector (into `codes`), bits 40..63
// the tile's first 64-vector block in the lane-ordered copy of the lists (ScanArgs::lanes; 0 where there is none)
constexpr int SCAN_VB_BITS = 40;
constexpr uint64_t SCAN_VB_MASK = (1ull << SCAN_VB_BITS) - 1;
inline __host__ __device__ uint64_t scan_vec_base(uint64_t first_vector, uint64_t first_block32_of_list, uint32_t pos_in_list) {
    return first_vector | (((first_block32_of_list >> 1) + pos_in_list / 64u) << SCAN_VB_BITS);
}

struct ScanItem {
    uint64_t vec_base;   // global index (into codes) of the tile's first vector (fp32 tiles: see scan_vec_base)
    uint32_t nvec;       // vectors in the tile
    uint32_t vec_off;    // position of the tile's first vector inside its list
    uint32_t pair_begin; // first entry of this tile in the pair arrays
    uint32_t npair;      // queries in the tile (<= qg * SCAN_RQ)
    uint32_t qg;         // query groups per workgroup: 1, 2, 4 or 8
    uint32_t qgroup;     // index of the tile's first 8-query group in the packed query tiles
};

struct ScanArgs {
    const float* codes;       // vectors, row-major, row stride d floats (d % 4 == 0)
    const float* queries;     // query matrix, row stride d floats
    const ScanItem* items;
    const uint32_t* pair_query;  // query row of each pair
    const uint64_t* pair_out;    // offset of each pair's distance row in `dist`
    float* dist;
    const float* qtile;       // packed query operands: [group][d/4][8 queries][4 floats] (pack_queries)
    int d;
    int metric;
    int fused;  // 1: fma(t, t, acc) -- only when the operands make it bit-identical to mul + add (see engine)
    // threshold mode (non-null thr): store only distances that beat thr[query row] and write one mask bit per
    // candidate (mask[i / 64] covers dist[i .. i + 63]); rows of `dist` start on multiples of 64
    const float* thr;
    unsigned long long* mask;
    int xcd_chunks;     // 1: XCD x (workgroup id % 8) takes the x-th eighth of the item list (consecutive items share an L2)
    uint32_t nitems;    // items of the shape being launched (set by launch_scan)
    // Device-chained rounds: the item counts of the four shapes are only known on the device (PlanArgs::counters); the launch
    // is then a fixed grid of resident workgroups that walk the items of their shape.  dev_counts = that counter array.
    const uint32_t* dev_counts;
    // ... sized by what the same round needed last time (0: no idea, one resident grid): the grid is a hint, never an input to
    // correctness -- workgroups stride over the true count -- and a right-sized grid lets the dispatcher interleave the
    // workgroups of several search contexts where resident grids would run one context's launch to its end first.
    uint32_t hint_qg[4];
    int hint_valid;     // hint_qg is what the same round of the previous search needed (a 0 there: probably no item of the shape again)
    // the lists once more in LANE ORDER (launch_lanes_from_f32), or null: 64-vector blocks (lists padded like the fragment copies:
    // block_off / 2), block b = d/4 pieces of 1 KiB, piece s = lane l's elements 4s .. 4s+3 of vector 64 b + l.  A wave streams a
    // block with one fully coalesced 16-byte-a-lane load per piece: scan_lanes_kernel needs no LDS staging and no barrier.
    const float* lanes;
};

// items grouped by qg (1, then 2, 4, 8); n_qg = item count of each group
// the shapes are independent: s2 / s1 / s4 (optional) let the qg 2 / 1 / 4 launches run beside the qg 8 one
void launch_scan(const ScanArgs& a, const size_t n_qg[4], hipStream_t s, hipStream_t s2 = nullptr, hipStream_t s1 = nullptr,
                 hipStream_t s4 = nullptr);
// fp32 lists (CSR rows, row stride dpad) -> lane order; nblocks64 = block_off[nlist] / 2
void launch_lanes_from_f32(const float* codes, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, uint64_t nblocks64, int dpad,
                           float* out, hipStream_t s);
// counters of PlanArgs that the chained launches read
constexpr int CNT_ACTIVE = 0, CNT_SEGMENTS = 1, CNT_PAIRS = 2, CNT_GROUPS = 3, CNT_QG1 = 4, CNT_QG2 = 5, CNT_QG4 = 8, CNT_QG8 = 9;
unsigned resident_grid(unsigned workgroups_per_cu);  // CUs of the current device x workgroups_per_cu

// gather + interleave the query rows of every group of (up to) 8 pairs: group g holds pairs
// [group_p0[g], group_p0[g] + group_cnt[g]); missing slots are zero
void launch_pack_queries(const float* queries, const uint32_t* pair_query, const uint32_t* group_p0, const uint32_t* group_cnt,
                         size_t ngroups, int d, float* qtile, hipStream_t s, const uint32_t* dev_ngroups = nullptr, uint32_t hint = 0);

// ---------------------------------------------------------------------------- byte-code scan on the i8 matrix cores
// When lists and queries hold integers 0..255 (and d * max^2 <= 2^24, so that every fp32 partial sum of the reference is an
// exact integer whatever the order) the distance tiles are integer contractions: v_mfma_i32_32x32x32_i8 on bytes re-centred
// to signed (u - 128), L2 = |xs|^2 + |ys|^2 - 2 xs.ys (translation invariant), IP = xs.ys + 128 sum(x) + 128 sum(y) - 16384 d.
//
// Storage of the lists for that kernel ("fragment order"): every list is cut into blocks of 32 vectors (lists padded to an
// even number of blocks); a block is ks x 64 x 16 bytes, ks = ceil(d / 32): 16-byte piece (s, lane) holds bytes
// [h * 16 ks + 16 s, + 16) of vector (lane & 31), h = lane >> 5 -- exactly the B operand of K-step s, so a wave fetches an
// operand with one fully coalesced 1-KiB load and no LDS staging.  Padding vectors / dimensions are signed zeros.
// code_cy: one int32 per stored slot (block * 32 + vector): |ys|^2 (L2) or 128 sum(y) (IP).
constexpr uint32_t MFMA_BLOCK = 32;        // vectors per block = N of the MFMA
constexpr uint32_t MFMA_QBLOCK = 32;       // queries per item = M of the MFMA
uint32_t mfma_chunk();                     // vectors per work item (a multiple of 64; AUNCEL_AMD_MFMA_CHUNK, default 256)
uint32_t mfma_chunk_thr();                 // ... of a threshold round (AUNCEL_AMD_MFMA_CHUNK_THR, default 512)
inline __host__ __device__ uint32_t mfma_ksteps(int d) { return (uint32_t)(d + 31) / 32; }
inline __host__ __device__ uint64_t mfma_list_blocks(uint64_t size) { return ((size + 63) / 64) * 2; }

struct MfmaScanArgs {
    const uint8_t* codes_frag;    // lists in fragment order
    const int32_t* code_cy;       // per stored slot
    const int8_t* queries8;       // signed query bytes, row stride ks * 32
    const int32_t* query_cx;      // per query row: |xs|^2 (L2) or 128 sum(x) - 16384 d (IP)
    const ScanItem* items;        // vec_base = first 32-block of the chunk (global block number), nvec = vectors of the chunk,
                                  // vec_off = position of the chunk in its list, pair_begin / npair (<= 32) = its queries
    const uint32_t* pair_query;
    const uint64_t* pair_out;
    float* dist;
    const float* thr;             // threshold mode (see ScanArgs)
    unsigned long long* mask;
    int d;
    int metric;
    int xcd_chunks;
    uint32_t nitems;
    const uint32_t* dev_nitems;   // chained rounds: the item count lives on the device; the grid is a hint (see ScanArgs)
    uint32_t hint_nitems;         // items the same round had last time (0: unknown -> a resident grid)
    int debug;                    // timing experiments only (results are wrong): 1 no mask stores, 2 no distance stores, 4 no epilogue,
                                  // 8 no contraction (threshold rounds)
    int exact_mask;               // threshold mode: the mask bits are counted as results (range search), not re-tested by a selection
    int pipelined;                // bit 0: dense rounds, bit 1: threshold rounds through scan_mfma_thr_kernel (two blocks in flight
                                  // per wave; threshold rounds: threshold folded into the accumulator, the mask a superset of
                                  // the exact one -- where exact_mask allows it); bit 2: threshold rounds with up to 64
                                  // queries per item through scan_mfma_pair_kernel (mfma_thr_qblock)
};
void launch_scan_mfma(const MfmaScanArgs& a, hipStream_t s);
uint32_t mfma_thr_qblock(int d, int pipelined, bool exact_mask);  // queries per item the planner gives a threshold round (32 | 64)
// fp32 lists (CSR rows, row stride dpad floats, integers 0..255) -> fragment order + code_cy; block_off[l] = first block of list l
void launch_frag_from_f32(const float* codes, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, uint64_t nblocks, int d,
                          int dpad, int metric, uint8_t* out, int32_t* cy, hipStream_t s);
// fp32 query rows (integers 0..255) -> signed byte rows (row stride ks * 32, zero padded) + query_cx
void launch_sbytes_from_f32(const float* x, size_t n, int d, int dpad, int metric, int8_t* out, int32_t* cx, hipStream_t s);
// ---------------------------------------------------------------------------- fp32 filter + exact rescoring (ivf_filter.hip)
// pieces of 8 dimensions per vector in the fragment-ordered fp32 copy: d / 8 rounded up to the step counts the kernel is built
// for (4, 8, 12, 16: the query operand stays in registers) or as it is beyond 128 dimensions
inline __host__ __device__ uint32_t filter_steps(int d) {
    const uint32_t j = (uint32_t)(d + 7) / 8;
    return j <= 4 ? 4u : j <= 8 ? 8u : j <= 12 ? 12u : j <= 16 ? 16u : (j + 1u) & ~1u;  // (beyond 128 dimensions: an even count)
}
struct FilterScanArgs {
    const float* codes_frag;      // lists in fragment order (launch_frag32_from_f32)
    const float* yn;              // per stored slot: |y|^2 (L2) / |y| (IP)
    const float* xf;              // packed queries, row stride 8 filter_steps(d) (launch_filter_queries)
    const float* xn;              // per query row: |x|^2 (L2) / |x| (IP)
    const float* codes;           // the lists as stored (CSR rows, stride dpad): the exact distance is computed from these
    const float* queries;         // the query rows as passed (stride dpad)
    const ScanItem* items;        // as for scan_mfma_kernel; qgroup = global index of the chunk's first vector
    const uint32_t* pair_query;
    const uint64_t* pair_out;
    float* dist;
    const float* thr;
    unsigned long long* mask;
    uint4* surv;                  // survivors of the filter: (distance row position, query row, vector, -)
    uint32_t* surv_count;
    uint32_t surv_cap;
    int d, dpad;
    int metric;
    int xcd_chunks;
    uint32_t nitems;
    const uint32_t* dev_nitems;
    uint32_t hint_nitems;
    int half;                     // 1: codes_frag / xf hold scaled fp16 values in the fp16 fragment order (launch_frag16_from_f32,
                                  // launch_filter_queries16) and `params` the scales and the error constant that go with them
    const float* params;          // half: FilterParams on the device (written by launch_filter_queries16)
};
// what the fp16 form of the filter needs besides its operands (device memory, one per search): the dot product of the scaled
// halves times `ps` is x.y up to C16 (|x|^2 + |y|^2) / 2; C = the constant of the keep test (ivf_filter.hip)
struct FilterParams {
    float sx, ps, C, pad;
};
struct KeepArgs;
// filter + rescoring, two launches; keep (a selected search, ivf_selector.hip): the keep bits are brought into the round's mask
// words between the two, and the rescoring leaves out the survivors whose bit went
// (keep_each: the same with a selector per query, keep_rows_each_kernel; at most one of the two is given)
struct KeepEachArgs;
void launch_scan_filter(const FilterScanArgs& a, hipStream_t s, const KeepArgs* keep = nullptr, const KeepEachArgs* keep_each = nullptr);
// pieces of 16 dimensions per vector in the fp16 fragment order: the step counts the one-wave kernel is built for (4, 6, 8) or an
// even count beyond 128 dimensions
inline __host__ __device__ uint32_t filter_steps16(int d) {
    const uint32_t j = (uint32_t)(d + 15) / 16;
    return j <= 4 ? 4u : j <= 6 ? 6u : j <= 8 ? 8u : (j + 1u) & ~1u;
}
// range of a row-major matrix for the fp16 form: info[0] = max |v| (bits of a non-negative float; +inf if a NaN or an infinity was
// seen), info[1] != 0: some element is not an integer of magnitude <= 2048 (fp16 holds those exactly), info[2] = 0x7f800000 - bits
// of the smallest row maximum among rows that are not all zero; info (4 words) zeroed by the caller
void launch_amax(const float* x, size_t rows, int stride, uint32_t* info, hipStream_t s);
// the scale that goes with such a range (0: none usable) -- ivf_filter.hip
float filter_half_scale(const uint32_t info[4], int d);
// FilterParams from the ranges of two matrices (sx, ps, C as above; pad = the second matrix's scale)
void launch_half_params(const uint32_t* qinfo, const uint32_t* yinfo, int d, FilterParams* params, hipStream_t s);
// fp32 lists -> fp16 fragment order, scaled by the power of two that brings info[0] into [2^14, 2^15); yn as launch_frag32_from_f32
void launch_frag16_from_f32(const float* codes, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, uint64_t nblocks, int d,
                            int dpad, int metric, const uint32_t* info, float* out, float* yn, hipStream_t s);
// query rows -> scaled fp16 rows (stride 16 filter_steps16(d) halves) + xn + the search's FilterParams
void launch_filter_queries16(const float* x, size_t n, int d, int dpad, int metric, const uint32_t* qinfo, const uint32_t* yinfo, float* xf,
                             float* xn, FilterParams* params, hipStream_t s);
// beyond 128 dimensions (the query operand no longer fits a wave's registers) an item of the filter is up to this many queries, computed by a whole workgroup (scan_filter_wide_kernel); AUNCEL_AMD_FILTER_NARROW=1 keeps the one-wave form
constexpr uint32_t FILTER_WIDE_QUERIES = 128;
constexpr uint32_t FILTER_WIDE_VECTORS = 128;  // ... x a chunk of this many vectors (one 32-vector block per wave)
uint32_t filter_item_queries(int d);
uint32_t filter_item_vectors(int d);
void launch_frag32_from_f32(const float* codes, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, uint64_t nblocks, int d,
                            int dpad, int metric, float* out, float* yn, hipStream_t s);
void launch_filter_queries(const float* x, size_t n, int d, int dpad, int metric, float* xf, float* xn, hipStream_t s);

inline __host__ __device__ int scan_qg_class(uint32_t qg) { return qg == 1 ? 0 : qg == 2 ? 1 : qg == 4 ? 2 : 3; }
// The queries of a list go into blocks of `qblock` (64: 8-wave tiles, the byte-code scan, which is short of HBM and
// issue slots rather than of VALU; 32: 4-wave tiles, the fp32 scans); the last block takes the narrowest shape that holds it.
constexpr uint32_t SCAN_QBLOCK = 8 * SCAN_RQ;  // the largest block
inline __host__ __device__ uint32_t scan_shape_of(uint32_t r) { return r <= SCAN_RQ ? 1u : r <= 2 * SCAN_RQ ? 2u : r <= 4 * SCAN_RQ ? 4u : 8u; }
inline __host__ __device__ uint32_t scan_tile_vecs(uint32_t qg) { return (qg >= 4 || qg == 1 ? 1u : 4u / qg) * SCAN_WAVE_VECS; }  // (ScanShape)

// ---------------------------------------------------------------------------- ordered selection
// One wave per query replays the reference's sequential heap (Heap.h) over the distance rows in
// probe order, evaluates the Auncel stop rule after every probe, and collects training samples.
struct TunerDev {
    int enabled;
    int profile;
    int overhead;   // error_pro::overhead_profile: the rule runs on every probe, its verdict is ignored, the loop ends at nlist / 8
    uint32_t max_topk, query_topk, ntraces;
    float multipler, std_m;
    const float* interdis;     // packed upper-triangular centroid table
    const float* arcos;        // 500-entry LUT
    const uint32_t* trace_off; // ntraces + 1
    const float *trace_x, *trace_y, *trace_std;
    const float* require_acc;  // by absolute query id
    const float* gt_D;         // by absolute query id, k wide (may be null)
    unsigned long long* my_nprobe;  // by absolute query id
    float* t_recalls;               // by absolute query id
};

struct TrainDev {
    int enabled;
    uint32_t ntraces;
    const float* interdis;
    const float* arcos;
    const float* gt_D;    // by absolute query id, k wide
    float* const* raw;    // ntraces device pointers
};

struct ReplayArgs {
    int metric;
    int k;
    uint32_t nlist;
    uint32_t nq;               // queries in this launch (chained rounds: an upper bound, the count is *nq_dev)
    const uint32_t* nq_dev;
    uint32_t nq_hint;          // expected number of queries (picks the kernel variant); 0: nq
    const uint32_t* qsel;      // [nq] query slot of each launch position (null: identity)
    uint32_t total_nprobe;     // length of the reference's probe loop (0: not bounded here)
    uint32_t round_probes;     // row stride of seg_* arrays
    uint64_t id_offset;        // absolute query id of query 0 of this launch
    const float* dist;
    const unsigned long long* mask;  // threshold mode: bit i of mask[j] set <=> dist[64 j + i] was stored (rows 64-aligned)
    float* thr;                // [nq] by query slot: heap top when the launch ends (may be null)
    const uint64_t* seg_off;   // [nq][round_probes] offset of the distance row       (by launch position)
    const int32_t* seg_list;   // [nq][round_probes] list number, <0 = missing centroid (by launch position)
    const uint32_t* seg_count; // [nq] probes supplied this round                      (by launch position)
    const uint32_t* seg_begin; // [nq] first entry of the query in seg_off / seg_list; null: li * round_probes
    int seg_by_slot;           // seg_count / seg_begin are indexed by query slot instead of launch position
    const uint64_t* list_off;  // nlist + 1 (vectors)
    const int64_t* ids;        // per stored vector
    int store_pairs;
    int identity_ids;          // ids are the positions themselves (coarse quantiser rows)
    unsigned long long max_codes;
    int finalize_all;          // fixed-nprobe mode: every query ends after this round
    const uint32_t* limit;     // [slot] time-bounded search: this query's probe loop ends at limit[slot] (null: total_nprobe)
    // per-query state carried across rounds
    float* heap_val;           // [nq][k]
    int64_t* heap_ref;         // [nq][k]  (list << 32 | position), -1 = empty
    uint32_t* stage;           // probes consumed so far
    unsigned long long* nscan; // codes visited so far
    uint32_t* done;            // 1 once the query has its final result
    float* pre_val;            // stop-rule state
    uint32_t* stoped;
    float* dtb;                // [nq][nlist/8+20] distance-to-boundary vector
    const float* coarse_dis;   // [nq][coarse_stride] full coarse ranking (tune / train)
    const int64_t* coarse_keys;
    uint32_t coarse_stride;
    uint32_t trace_cap;        // longest trace (LDS cache size), tune mode
    // outputs
    float* D;                  // [nq][k]
    int64_t* I;
    unsigned long long* stats; // {nlist, ndis, nheap, ties} x 8: one row per XCD (added with L2-local atomics: STATS_ROWS below)
    uint32_t* error;           // != 0: the reference would have thrown (code)
    int raw_heap_out;          // scanner API: leave the heap un-reordered in D/I
    long long pair_list = -1;  // scanner API over a list part (store_pairs): the list number new labels carry (< 0: the segment's own)
    unsigned long long* dbg;   // optional [nq][8]: wave cycles, heap updates, candidates, stages evaluated, cycles in the
                               // candidate stream, cycles in the stop rule, masked chunks fetched, probes consumed
    TunerDev tuner;
    TrainDev train;
    // Sorted-array selection (replay_kernel MODE 2; null log: the heap kernels).  heap_val / heap_ref then hold the k best in
    // best-first order (values, global positions) between rounds.
    uint2* log;                // [slot][log_cap] admissions in order: (value bits, global position = list_off[list] + position)
    uint32_t log_cap;
    uint32_t* log_cnt;         // [slot]
    uint32_t* amb;             // [slot] order key of a value whose id became ambiguous (0xffffffff: none)
    uint32_t* tie_flag;        // [slot] set when the query's result has to come from tie_fix_kernel
    uint32_t round;            // number of this round within the search
    uint32_t* log_snap;        // [2][nq_total] log_cnt as this round left it, by round parity (tie_fix_kernel of this round reads it
                               //               while the next round's selection already appends)
    uint32_t nq_total;
    uint32_t* fin_round;       // [slot] the round in which the query got its final state (0xffffffff: not yet)
    uint2* qstat;              // [slot] (lists scanned, heap updates) of this query so far (null: not kept)
    uint32_t* unfinished;      // null or 8 counters (one per XCD): += 1 for every query of this launch that goes on to another round (with the
                               // queries the planning deferred, PlanArgs counters[11], what is left after the round: the host
                               // needs no further planning pass to learn that a search has ended)
    // threshold rounds, optional: what compact_rows_kernel made of the masks (by launch position, like seg_off)
    const uint32_t* cl_cnt;    // marked candidates of the row (CL_WALK: find them in the masks)
    const uint2* cl_ent;       // [CL_CAP] per row: (position in the list, distance bits) in position order while cl_cnt <= CL_CAP; a longer
                               // list is in the arena, and entry 0 says where: (first entry, -)
    const uint2* cl_arena;
};

bool replay_sorted_applies(const ReplayArgs& a);
void launch_replay(const ReplayArgs& a, hipStream_t s);

// A threshold round leaves a mask bit in one candidate of two thousand: a query's selection walking its rows -- mask words, then
// the marked chunks -- pays a trip to memory per row, one row after the other (132 rows: 0.35 ms with the chip nearly empty).
// compact_rows_kernel does that walk for every row of the round at once (a wave per eight rows) and leaves each row's marked
// candidates as a short list at an address the selection knows in advance: it requests 64 rows' lists with its probe table.
// Rows with more candidates than a list holds (the first rows of a hard query: dozens) get a run of the arena: one eighth of it per
// XCD, places handed out by an add that the XCD's L2 serves (ivf_dev.h: xcd_local_add); when that is full: CL_WALK.
constexpr uint32_t CL_CAP = 8;
constexpr uint32_t CL_WALK = 0xffffffffu;
struct CompactArgs {
    const uint32_t* nseg_dev;  // rows of the round (device count), or null: nseg
    uint32_t nseg;
    uint32_t nseg_hint;        // sizes the grid
    uint32_t nlist;
    const int32_t* seg_list;
    const uint64_t* seg_off;
    const uint64_t* list_off;
    const float* dist;
    const unsigned long long* mask;
    uint32_t* cl_cnt;
    uint2* cl_ent;
    uint2* arena;
    uint32_t arena_per_xcd;    // entries
    uint32_t* cursor;          // [8 x 32] next free entry of every XCD's part (zeroed by the round's planning)
};
void launch_compact_rows(const CompactArgs& a, hipStream_t s);

// see tie_fix_kernel (ivf_select.hip)
struct TieFixArgs {
    int metric;
    int k;
    uint32_t nq, nlist;
    const uint2* log;
    uint32_t log_cap;
    uint32_t round;              // the selection round this launch follows
    int final_pass;              // 1: one launch at the end of the search instead of one per round: every flagged query, whole log
    const uint32_t* log_cnt;     // [nq] (final pass)
    const uint32_t* log_snap;    // [2][nq]
    const uint32_t* fin_round;   // [nq]
    float* fix_val;              // [nq][k] the reference's heap (node order) as far as the log has been replayed
    int64_t* fix_ref;            // [nq][k] global positions, -1 = empty
    uint32_t* fix_pos;           // [nq] log entries replayed so far
    uint32_t* tie_flag;
    const uint64_t* list_off;
    const int64_t* ids;
    int store_pairs, identity_ids;
    float* D;
    int64_t* I;
};
void launch_tie_fix(const TieFixArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------- range search
// IndexIVF::range_search_preassigned: the scan runs in threshold mode with the radius as every query's threshold,
// so the masks mark exactly the entries scan_codes_range would add.  One wave per query counts its entries, then
// (offsets known) writes (distance, label) in the reference's order: probes in order, list entries in order.
struct RangeArgs {
    uint32_t nq;                 // active queries of this round
    uint32_t nlist;
    const uint32_t* qsel;        // [nq] query slot of each launch position
    const uint32_t* seg_count;   // by slot: probes this round
    const uint32_t* seg_begin;   // by slot: first entry in seg_list / seg_off
    const int32_t* seg_list;
    const uint64_t* seg_off;
    const uint64_t* list_off;
    const int64_t* ids;
    const float* dist;
    const unsigned long long* mask;
    uint32_t* counts;                     // by slot: entries found (count pass)
    const unsigned long long* out_off;    // by slot: first output position (fill pass)
    int64_t* out_labels;
    float* out_dist;
    uint32_t* stage;
    uint32_t* done;
    unsigned long long* stats;   // {nlist, ndis, -}
    uint32_t* error;
};
void launch_range_count(const RangeArgs& a, hipStream_t s);
void launch_range_fill(const RangeArgs& a, hipStream_t s);

// error_pro::set_online for nq queries: dtb[q][nlist/8+20] from the full coarse ranking (before round 0)
void launch_set_online(int metric, uint32_t nlist, uint32_t nq, const float* coarse_dis, const int64_t* coarse_keys,
                       uint32_t coarse_stride, const float* interdis, const float* arcos, float* dtb, uint32_t* error, hipStream_t s,
                       const uint32_t* qsel = nullptr, const uint32_t* nq_dev = nullptr);  // (optional: a subset of the queries, count on the device)
void launch_partition_qsel(const uint32_t* qsel, const uint32_t* nq_dev, uint32_t nq, const int32_t* slot_of, uint32_t* q_free, uint32_t* q_wait,
                           uint32_t* counts, hipStream_t s);

// ---------------------------------------------------------------------------- device-side round planning
struct PlanArgs {
    uint32_t nq;               // query slots of this search (state arrays are indexed by slot)
    uint32_t nlist;
    uint32_t total_nprobe;     // length of the probe loop (= nlist in tune / train mode)
    uint32_t key_stride;
    uint32_t slot_base;        // row of slot 0 in the query matrix the scan reads (pair_query = slot_base + slot)
    uint32_t first_round, round_len;
    uint32_t min_inc;          // tune mode: probes a later round adds at least (round 0 runs first_round)
    int tune;
    int d;
    float multipler;
    double grow;
    unsigned long long id_offset;
    unsigned long long dist_budget;  // floats
    uint32_t seg_cap;
    const int64_t* keys;             // [nq][key_stride] coarse ranking
    const uint64_t* list_off;
    const uint32_t* stage;
    const uint32_t* done;
    const unsigned long long* my_nprobe;  // by absolute id, may be null
    // time-bounded search (IndexIVF.cpp:504-506,545-549): budgets in ms by absolute id, ms elapsed when this round is
    // planned, and the per-slot end of the probe loop the plan derives from them (read by the replay)
    const float* budget_ms;
    float elapsed_ms;
    uint32_t* limit;
    // outputs
    uint32_t* cnt;                   // [nq] probes this round (0: finished or deferred)
    unsigned long long* need;        // [nq] floats of distance rows (rows padded to multiples of `row_align`)
    uint32_t* pad;                   // [nq] padding inside need
    uint32_t row_align;              // 1 or 64
    uint32_t qblock;                 // queries per full block of a list: 64 (8-wave tiles) or 32 (4-wave tiles)
    uint32_t mfma_chunk;             // != 0: items for scan_mfma_kernel (vectors per item); counted as tiles of shape 8
    uint32_t mfma_qblock;            // queries per item in that form (MFMA_QBLOCK: one tile)
    int item_order;                  // ... items of a list: 0 chunk major (a chunk's query blocks are neighbours), 1 query block major
    const uint64_t* block_off;       // mfma: first 32-vector block of every list in the fragment-order storage
    const uint64_t* lane_block_off;  // fp32 tiles over the lane-ordered copy (ScanArgs::lanes): the same array, else null
    uint32_t* seg_begin;             // [nq]
    unsigned long long* dist_base;   // [nq]
    uint32_t* qsel;                  // active slots, compacted
    int32_t* seg_list;
    uint64_t* seg_off;
    uint32_t* lcount;                // [nlist] pairs per list (written by plan_lists_kernel)
    uint32_t* lstart;
    uint32_t* gbase;
    uint32_t* ibase;                 // [4][nlist]
    uint32_t* xcount;                // [8 x nlist] pairs per (XCD that counted them, list); after plan_lists_kernel: the XCDs' offsets inside a list
    uint32_t* seg_slot;              // [seg_cap] per pair: XCD << 28 | its place among that XCD's pairs of the list
    uint32_t* pair_query;
    uint64_t* pair_out;
    uint32_t* group_p0;
    uint32_t* group_cnt;
    ScanItem* items;
    uint32_t item_cap;
    uint32_t* error;                 // device error word (ERR_ITEM_OVERFLOW: the round needs more tiles than item_cap)
    unsigned long long* acc64;       // [0] += (query, vector) slots computed, [1] += pairs wanted (tile bookkeeping)
    uint32_t* history;               // null or 16 uint32: receives the counters as the previous round's planning left them
    int first_plan;                  // first planning pass of a search: the accumulators below and round_unfinished start from zero
    uint32_t* round_unfinished;      // null or [PLAN_MAX_ROUNDS][8]: per round and XCD, queries its selection left unfinished (ReplayArgs::unfinished)
    uint32_t* cl_cursor;             // null or [8 x 32]: CompactArgs::cursor, zeroed with the counters
    uint32_t* counters;              // [0] active queries [1] segments [2] pairs [3] groups [4] tiles qg1 [5] tiles qg2
                                     // [6] scratch (compaction cursor, zeroed by host) [7] MiB of distances [8] tiles qg4 [9] tiles qg8
                                     // [10] queries that may still be unfinished after this round, [11] of those: deferred by the
                                     //      budget cut
    double* bytes;                   // [0] += algorithmic bytes of the round's distances
    // [0] += bytes the round cannot avoid moving through HBM: every probed list once (row_bytes per stored vector) and the
    // rows it writes (4 bytes per distance of a dense round, one mask bit per distance in threshold mode)
    double* min_bytes;
    double* min_bytes_thr;           // the same for the threshold rounds alone (null: not kept)
    uint32_t row_bytes;
    int dense_round;
    // null or the sorted coarse distances [nq][key_stride]: a round never ends inside a run of exactly equal distances (the order
    // inside a run may still change -- launch_tie_patch -- and a round's rows can be reordered, not exchanged with the next round's)
    const float* run_dis;
    // a search under an id selector that skips the lists it keeps nothing in: the per-list kept counts of the call's selector (kept),
    // or of every selector of the call's table with the selector number of every query slot (kepts / kept_sel_of); all null: every
    // probe is planned.  A (query, list) pair whose count is 0 is planned as an absent probe: seg_list -1, no row, no pair, no item --
    // the selection counts the probe and evaluates the stop rule after it, as it does for an empty list.
    const uint32_t* kept;
    const uint32_t* const* kepts;
    const uint32_t* kept_sel_of;
};

// self-check of the per-XCD counters (ivf_plan.hip: xcd_check_kernel): counters [8][nkeys] zeroed by the caller
void launch_xcd_check(uint32_t* counters, uint32_t nkeys, uint32_t* slot, uint32_t* xcc_of, uint32_t n, hipStream_t s);

constexpr uint32_t PLAN_MAX_ROUNDS = 64;
// Counters that every wave of a selection adds to (statistics, queries left unfinished) exist once per XCD and are added to with
// workgroup-scope atomics, which that XCD's L2 serves: thousands of adds on ONE word from all eight XCDs are served one after the
// other at the memory side, ~12 ns each -- 30000 of them were 0.21 of a 0.48 ms selection launch (cfg 1, 10000 queries).  Rows
// 0..7: the XCDs; row 8: kernels that add with ordinary (agent-scope) atomics.  The host sums the rows.
constexpr uint32_t STATS_ROWS = 9;
void launch_plan(const PlanArgs& a, hipStream_t s);

constexpr uint32_t ERR_ARCOS_DOMAIN = 1;
constexpr uint32_t ERR_COSINE_PRECOND = 2;
constexpr uint32_t ERR_INVALID_KEY = 3;
constexpr uint32_t ERR_ITEM_OVERFLOW = 4;
constexpr uint32_t ERR_LOG_OVERFLOW = 5;  // a query admitted more candidates than its admission log holds

// ---------------------------------------------------------------------------- coarse helpers
// full ascending/descending sort of each row of `dis` (nlist entries) keeping the first nprobe
// prefix != 0: only the first `prefix` entries are needed in order; the rest may come out as (neutral, -1)
bool sort_rows_ranks_a_prefix(uint32_t nlist, uint32_t nprobe, uint32_t prefix);
void launch_sort_rows(const float* dis, uint32_t nq, uint32_t nlist, uint32_t nprobe, int metric, float* out_dis,
                      int64_t* out_keys, hipStream_t s, uint32_t prefix = 0, bool tail_is_neutral = false);

// Rows whose first `nout` entries hold (or end inside) a run of exactly equal distances are re-ranked by the reference's
// own heap (utils.cpp:417-490, Heap.h:88-142,295-322), whose order inside such a run depends on its history; *nrows
// counts them.  false = heap + row exceed one workgroup's LDS, nothing launched.
bool launch_heap_tie_order(const float* dis, uint32_t nq, uint32_t nlist, uint32_t nprobe, uint32_t nout, int metric, float* out_dis,
                           int64_t* out_keys, unsigned long long* nrows, hipStream_t s, const uint32_t* dev_nq = nullptr);

size_t heap_tie_order_lds(uint32_t nlist, uint32_t nprobe);  // LDS bytes of one row's workgroup

// Rankings that may need the heap's order, set aside while the search runs (AUNCEL_AMD_COARSE_TIES=redo): every query whose
// first run of equal distances starts in [lo, window) gets a slot (at most cap; *count keeps counting beyond) holding copies of
// its distance row (nlist floats) and of the first ncopy entries of its ranking (slot rows of nlist entries);
// slot_of[q] = its slot or -1.  launch_heap_tie_order(dev_nq = count) then re-ranks the slots on a side stream.
void launch_spec_collect(const uint32_t* first, uint32_t nq, uint32_t lo, uint32_t window, uint32_t cap, uint32_t nlist, uint32_t ncopy,
                         const float* full, const float* cdis, const int64_t* ckeys, uint32_t* count, int32_t* slot_of, float* s_full,
                         float* s_dis, int64_t* s_keys, hipStream_t s, uint32_t* slot_query = nullptr);
// The heap's order of the slots' rankings applied to the search that set them aside, between the scan and the selection of its
// first round (nothing before the selection reads the order inside a run of equal distances: the planner takes whole runs into
// the round, PlanArgs::run_dis).  Per slot: the ranking's keys are overwritten with the heap's (same distances in the same places);
// where that changes the order of rows the round has scanned, the rows and their table entries are put in the new order (through
// `scratch`).  slot_of[q] = -2 - slot where that is not possible (more than 64 rows, a run across the end of the round, scratch full): the
// caller searches those queries again.  *patched counts the rankings that changed.
struct TiePatchArgs {
    const uint32_t* count;       // slots handed out (may exceed cap)
    uint32_t cap, nlist, ncopy, key_stride;
    const uint32_t* slot_query;  // [cap]
    int32_t* slot_of;            // [nq]
    const int64_t* s_keys;       // [cap][nlist] the heap's order
    int64_t* ckeys;              // [nq][key_stride] the search's ranking
    const uint32_t* seg_count;   // [nq] rows of the query in the round
    const uint32_t* seg_begin;   // [nq]
    int32_t* seg_list;
    uint64_t* seg_off;
    const uint64_t* list_off;
    float* dist;
    uint32_t row_align;
    float* scratch;
    unsigned long long scratch_floats;
    unsigned long long* cursor;  // zeroed by the caller
    uint32_t* patched;
};
void launch_tie_patch(const TiePatchArgs& a, hipStream_t s);
// launch_first_tie + launch_spec_collect in one launch (sorted rankings of row stride nlist): first_out[q] as launch_first_tie
// leaves it, slots handed out in the order the waves arrive
void launch_tie_collect(const float* sorted_dis, uint32_t nq, uint32_t nreal, uint32_t window, uint32_t cap, uint32_t nlist, uint32_t ncopy,
                        const float* full, const int64_t* ckeys, uint32_t* first_out, uint32_t* count, int32_t* slot_of, float* s_full, float* s_dis,
                        int64_t* s_keys, uint32_t* slot_query, hipStream_t s);
// rows of a second search from those slots: ranking row j <- slot slots[j] (ncopy leading entries, rows of nlist entries)
void launch_spec_gather(const int32_t* slots, uint32_t m, uint32_t nlist, uint32_t ncopy, const float* s_dis, const int64_t* s_keys,
                        float* cdis, int64_t* ckeys, hipStream_t s);
// out row j <- x row idx[j] (rows of dpad floats)
void launch_gather_rows(const float* x, const uint32_t* idx, uint32_t m, uint32_t dpad, float* out, hipStream_t s);

// position of the first pair of equal neighbours among the first nreal entries of every sorted ranking (row stride `stride`
// floats), 0xffffffff if there is none
void launch_first_tie(const float* sorted_dis, uint32_t nq, uint32_t stride, uint32_t nreal, uint32_t* out, hipStream_t s);

// GEMM-formulated coarse distances on the fp32 matrix cores (row stride d, d % 4 == 0)
void launch_row_norms(const float* x, size_t n, int d, float* out, hipStream_t s);
// approximate distances from fp16 operands (the rows are scaled and rounded while they are staged; the error constant that goes
// with them is params->C: |approx - exact| <= C (|x|^2 + |y|^2), C < 0: no usable scale, the result means nothing)
void launch_coarse_gemm16(int metric, const float* X, const float* Y, const float* xn, const float* yn, int nq, int ny, int d, float* out,
                          const FilterParams* params, hipStream_t s);
void launch_coarse_gemm(int metric, const float* X, const float* Y, const float* xn, const float* yn, int nq, int ny, int d, float* out,
                        hipStream_t s);

// exact top-nprobe (nprobe << nlist <= 4096) from approximate distances + exact recomputation of the candidates (see
// coarse_pick_kernel); queries whose result could depend on the reference's heap history are counted in *nflag / listed in
// flagged[] and left to the caller
void launch_coarse_pick(int metric, const float* approx, const float* x, const float* centroids, const float* xn, float cmax, uint32_t n,
                        uint32_t nlist, uint32_t nprobe, int dpad, float* out_dis, int64_t* out_keys, uint32_t* nflag, uint32_t* flagged,
                        hipStream_t s, const FilterParams* params = nullptr, uint32_t* why = nullptr);  // params: the approximate distances came from launch_coarse_gemm16
void launch_scatter_rows(const void* in, const uint32_t* idx, uint32_t m, uint32_t words, void* out, hipStream_t s);

// packed upper triangle (IVF_pro.cpp:21-39 layout) of a full nlist x nlist distance matrix
void launch_pack_upper(const float* full, uint32_t nlist, float* out, hipStream_t s);

// k-means centroid update (ivf_kmeans.hip): points grouped by centroid with a stable sort, then fp32 sums in point order.
// counts: k + 1 entries, points per centroid and, in counts[k], a flag raised by any assignment outside [0, k)
size_t kmeans_sort_temp_bytes(size_t n);
void launch_kmeans_group(const int64_t* assign, size_t n, uint32_t k, uint32_t* keys_in, uint32_t* keys_out, uint32_t* idx_in,
                         uint32_t* idx_out, uint32_t* counts, void* temp, size_t temp_bytes, hipStream_t s);
void launch_kmeans_sums(const float* x, size_t stride, int d, const uint32_t* idx_sorted, const uint32_t* seg_off, uint32_t k, float* centroids,
                        hipStream_t s);

// Up to MAX small copies in ONE launch (one workgroup row per segment; sizes in 4-byte words).  A search starts and ends with a
// dozen copies of a few bytes to a few tens of KB (per-call inputs, error word, counters, my_nprobe, t_recalls ...): as
// hipMemcpyAsync each of them is a blit kernel of its own on the stream (18 % of the four-in-flight span in round 3's trace);
// through page-locked staging they are one kernel before the first round and one behind the last.
struct CopySegs {
    static constexpr int MAX = 12;
    const void* src[MAX];
    void* dst[MAX];
    uint32_t words[MAX];
    uint32_t n;
};
void launch_copy_segs(const CopySegs& c, hipStream_t s);

// fill helpers
struct InitStateArgs {
    size_t n, k;
    float neutral;  // FLT_MAX (L2) / -FLT_MAX (IP)
    float* heap_val;
    int64_t* heap_ref;
    float* thr;
    uint32_t* stage;
    unsigned long long* nscan;
    uint32_t* done;
    float* pre_val;
    uint32_t* stoped;
    unsigned long long* stats;  // 4 counters
    uint32_t* error;
    uint32_t *log_cnt, *amb, *tie_flag;  // sorted-array selection (may be null)
    uint32_t *log_snap, *fin_round, *fix_pos;
    uint2* qstat;
    float* fix_val;
    int64_t* fix_ref;
};
void launch_init_state(const InitStateArgs& a, hipStream_t s);
// A call of at most four queries: the per-query state (init_state_kernel), the boundary distances of the stop rule
// (set_online_kernel), the start of each ranking's first run of equal coarse distances (first_tie_kernel) and the signed-byte view of
// the queries (sbytes_from_f32_kernel) in ONE launch -- four launches of a few microseconds of work each are four dispatch
// latencies on the critical path of a 0.25 ms call.
struct SmallStateArgs {
    InitStateArgs init;
    int metric;
    uint32_t nlist, nq;
    const float* coarse_dis;
    const int64_t* coarse_keys;
    uint32_t coarse_stride;
    const float* interdis;
    const float* arcos;
    float* dtb;
    const float* ft_sorted_dis;  // first tie: null = not wanted
    uint32_t ft_stride, ft_nreal;
    uint32_t* ft_out;
    const float* bx;             // byte view: null = not wanted
    int d, dpad;
    int8_t* bout;
    int32_t* bcx;
};
void launch_small_state(const SmallStateArgs& a, hipStream_t s);
void launch_range_collect(const float* dist, uint32_t n, float radius, int metric, uint32_t* count, uint32_t* out_pos, float* out_dis, hipStream_t s);
void launch_fill_f32(float* p, size_t n, float v, hipStream_t s);
void launch_fill_i64(int64_t* p, size_t n, int64_t v, hipStream_t s);

// ---------------------------------------------------------------------------- in-place updates (ivf_update.hip)
// The derived copies again for the blocks listed in `blocks` only (32-vector blocks; the lane copy's 64-vector blocks), with the
// same device code as the whole-copy launches above: an update re-encodes what it changed and copies the rest.
void launch_frag_from_f32_list(const float* codes, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, const uint64_t* blocks,
                               uint64_t nlisted, int d, int dpad, int metric, uint8_t* out, int32_t* cy, hipStream_t s);
void launch_frag32_from_f32_list(const float* codes, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, const uint64_t* blocks,
                                 uint64_t nlisted, int d, int dpad, int metric, float* out, float* yn, hipStream_t s);
void launch_frag16_from_f32_list(const float* codes, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, const uint64_t* blocks,
                                 uint64_t nlisted, int d, int dpad, int metric, const uint32_t* info, float* out, float* yn, hipStream_t s);
void launch_lanes_from_f32_list(const float* codes, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, const uint64_t* blocks64,
                                uint64_t nlisted, int dpad, float* out, hipStream_t s);
// rows (stride dpad) and ids of the new layout: entry p of list l comes from entry p of the old layout where p < its old size, else
// it is zeroed (the scatter below writes it)
void launch_relayout_rows(const float* old_codes, const int64_t* old_ids, const uint64_t* old_off, const uint64_t* new_off, uint32_t nlist,
                          uint64_t nt_new, int dpad, float* codes, int64_t* ids, hipStream_t s);
// the written entries from one staged block: rows[i] (a row of the new layout), ids[i], vals[i * dpad .. + dpad)
void launch_scatter_rows(const uint64_t* rows, const int64_t* wids, const float* vals, uint64_t nw, int dpad, float* codes, int64_t* ids,
                         hipStream_t s);
// a block copy in its new layout: block b of list l is block b of the old layout where the list had one (the changed blocks are
// re-encoded afterwards); `shift` 0 for 32-vector blocks, 1 for 64-vector blocks (block_off / 2); main: block_bytes a block,
// side (or null): side_bytes a block (cy, yn)
void launch_relayout_blocks(const void* old_main, void* new_main, uint64_t block_bytes, const void* old_side, void* new_side, uint64_t side_bytes,
                            const uint64_t* old_boff, const uint64_t* new_boff, uint32_t nlist, uint64_t nblk_new, int shift, hipStream_t s);

// ---------------------------------------------------------------------------- subset of a resident index (ivf_subset.hip)
// Which entries a subset keeps (include/auncel_amd.h: amd_ivf_subset; the kinds: selector_args.h).  Every array is device memory.
struct SubsetSel {
    int type;
    int64_t a1, a2;          // ID_RANGE: a1 <= id < a2; ID_MOD: id % a1 == a2
    const uint64_t* runs;    // SLICE: entries [runs[2 l], runs[2 l + 1]) of list l
    const uint64_t* bits;    // ID_BITS: nsel words
    const int64_t* batch;    // ID_BATCH: nsel ids, ascending, each once
    uint64_t nsel;
};
// The keep-mask of the parent's entries: word w covers 64 consecutive entries of ONE list (list l owns words block_off[l] / 2 ..
// block_off[l + 1] / 2: the 64-vector blocks of the padded copies), bit i of it entry 64 (w - first word) + i; count[w] = its set bits.
void launch_subset_member(const int64_t* ids, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, uint64_t nwords,
                          const SubsetSel& sel, uint64_t* mask, uint32_t* count, hipStream_t s);
// rank_base[w] = kept entries of w's list before word w; then the kept lists' offsets and block table (nlist + 1 each)
void launch_subset_offsets(const uint32_t* count, const uint64_t* block_off, uint32_t nlist, uint32_t* rank_base, uint64_t* list_total,
                           uint64_t* new_off, uint64_t* new_block_off, hipStream_t s);
// kept rows (stride dpad) and ids to their places, in the parent's order; range = {some value is not an integer of magnitude <= 4095,
// order key of the smallest value, of the largest, -} over the kept rows, started by the caller at {0, key(0), key(0), 0}
// (subset_range_key / subset_range_value)
void launch_subset_compact(const float* old_codes, const int64_t* old_ids, const uint64_t* old_off, const uint64_t* old_block_off, uint32_t nlist,
                           uint64_t nwords, const uint64_t* mask, const uint32_t* rank_base, const uint64_t* new_off, int dpad, float* codes,
                           int64_t* ids, uint32_t* range, hipStream_t s);
// ---------------------------------------------------------------------------- resident indexes joined (ivf_concat.hip)
// One part of a join (include/auncel_amd.h: amd_ivf_concat): the rows (stride dpad) and ids of an index that is resident on the same
// device, and what is added to every id taken from it
struct ConcatPart {
    const float* codes;
    const int64_t* ids;
    int64_t id_add;
};
// Rows and ids of the joined layout: entry p of list l comes from the first part j with cum[j * nlist + l] > p -- cum: the entries
// parts 0 .. j give list l together -- and is that part's row src_start[j * nlist + l] + (p - cum[(j - 1) * nlist + l]), its id plus
// the part's id_add.  Every array is device memory; range as launch_subset_compact's, over the rows taken.
void launch_concat_rows(const ConcatPart* parts, uint32_t nparts, const uint64_t* src_start, const uint64_t* cum, const uint64_t* new_off,
                        uint32_t nlist, uint64_t nt, int dpad, float* codes, int64_t* ids, uint32_t* range, hipStream_t s);
// ---------------------------------------------------------------------------- stored vectors back (ivf_reconstruct.hip)
// table[id - lo] = max(table[id - lo], list << 32 | offset) for every stored entry whose id lies in [lo, lo + n) (nt entries, list_off:
// nlist + 1); the caller starts the table at -1 in every slot and counts at {0, 0}: counts[0] += entries outside the window,
// counts[1] += slots that took a position.  lo + n must be an int64 (reconstruct_args.h: recon_window_error).
void launch_id_positions(const int64_t* ids, const uint64_t* list_off, uint32_t nlist, uint64_t nt, int64_t lo, uint64_t n, int64_t* table,
                         unsigned long long* counts, hipStream_t s);
// m position labels (list << 32 | offset, or -1) into m compact rows of d floats, read from the rows as stored (stride dpad)
constexpr int RECON_NONE_FILL = 0, RECON_NONE_SKIP = 1, RECON_NONE_ERROR = 2;  // what a label of -1 does
struct GatherRowsArgs {
    uint64_t m;
    const int64_t* labels;   // row i's label, unless ...
    const int64_t* keys;     // ... table != null: table[keys[i]], keys[i] in [0, table_n)
    const int64_t* table;
    uint64_t table_n;
    const float* codes;      // the resident rows, ids and offsets
    const int64_t* ids;
    const uint64_t* list_off;
    uint64_t nlist;
    int d, dpad;
    int none_mode;           // RECON_NONE_FILL: 0xFF bytes and id -1; _SKIP: nothing written, found 0; _ERROR: the flag
    int wide_out;            // rows is 16-byte aligned and d % 4 == 0: 16-byte stores
    float* rows;             // m x d out
    int64_t* ids_out;        // m stored ids out, or null
    uint8_t* found;          // m bytes out (1: a row was written), or null
    unsigned long long* bad; // started at ~0 by the caller: the smallest i whose label or key names nothing (nothing is read for it)
};
void launch_gather_rows(const GatherRowsArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------- query rows from device memory (ivf_ingest.hip)
// n rows of d elements (dtype 0: fp32, 1: fp16; row stride ldx >= d elements, columns contiguous) at the device pointer x -> the
// engine's query layout in `out` (fp32, row stride dpad, zero padded), and in the same pass the range of the n x d elements
// (query_range.h) into parts[INGEST_MAX_PARTS]; parts[0 .. INGEST_MAX_PARTS) are the workgroups' partial ranges.  Two launches.
constexpr uint32_t INGEST_MAX_PARTS = 512;
void launch_ingest_rows(const void* x, int dtype, size_t n, int d, int dpad, size_t ldx, float* out, QueryRange* parts, hipStream_t s);

// ---------------------------------------------------------------------------- search under an id selector (ivf_selector.hip)
// kept[l] = the set bits of list l's words (a wave per list)
void launch_selector_list_kept(const uint32_t* count, const uint64_t* block_off, uint32_t nlist, uint32_t* kept, hipStream_t s);
// amd_ivf_selector_combine: keep[w] = op(a[w], b[w]) & the bits of w that stand for entries of its list (selector_args.h:
// selector_combine_word, selector_valid_word, from list_off alone), count[w] its set bits, kept[l] those of list l's words.  A wave
// per list; b is null for SELECTOR_NOT; keep may not alias a or b.
void launch_selector_combine(int op, const uint64_t* a, const uint64_t* b, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist,
                             uint64_t* keep, uint32_t* count, uint32_t* kept, hipStream_t s);
// The keep words of a selector into the mask words of a round's rows: row r (seg_list / seg_off, as the planner left them) of list l
// owns the words seg_off[r] / 64 ... of the mask, one per 64 candidates, and word j of it lines up with keep word block_off[l] / 2 + j.
// write = 1 (a dense round: the scan left no mask) the keep words become the row's mask, else (a threshold round) they are ANDed
// into what the scan marked.
struct KeepArgs {
    const uint32_t* nseg_dev;  // rows of the round (device count), or null: nseg
    uint32_t nseg;
    uint32_t nseg_hint;        // sizes the grid
    uint32_t nlist;
    const int32_t* seg_list;
    const uint64_t* seg_off;
    const uint64_t* list_off;
    const uint64_t* block_off;
    const unsigned long long* keep;
    unsigned long long* mask;
    int write;
};
void launch_keep_rows(const KeepArgs& a, hipStream_t s);
// ... with a selector per QUERY (amd_ivf_search_*_selected_each): the keep words of a row are those of its query's selector,
// keeps[sel_of[slot]].  A round's rows of one query are consecutive (seg_begin / seg_count, by query slot, as the planner left them);
// launch position p < the round's active queries stands for slot qsel[p] -- the table the selection kernels go through to the
// query's row of D / I -- and sel_of is indexed by that slot, which is the caller's query number.
struct KeepEachArgs {
    const uint32_t* nq_dev;    // active queries of the round (device count), or null: nq
    uint32_t nq;
    uint32_t nseg_hint;        // rows expected: sizes the grid
    uint32_t probes;           // P: waves dealt to a query, the round's probe count (a query with more rows takes several trips)
    uint32_t nlist;
    uint32_t nsel;
    const uint32_t* qsel;      // [active] query slot of each launch position
    const uint32_t* seg_count; // by slot: rows this round
    const uint32_t* seg_begin; // by slot: first row
    const int32_t* seg_list;
    const uint64_t* seg_off;
    const uint64_t* list_off;
    const uint64_t* block_off;
    const unsigned long long* const* keeps;  // [nsel] keep-word base of every selector of the call (device table)
    const uint32_t* sel_of;    // by slot
    unsigned long long* mask;
    int write;
};
void launch_keep_rows_each(const KeepEachArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------- exact search over the whole index (ivf_exact.hip)
// The list pass of amd_ivf_search_exact: every query against every 32-vector block of the byte fragments (d <= 128; launch_scan_all_wide_i8: up to 1024), candidates at or
// within the query's threshold appended to the query's buffer.  seed_D / seed_I: the n x k result of a search of the same lists
// (row q's last entry is the threshold; id < 0 there: the query has none and emits nothing).
struct ExactScanArgs {
    const uint8_t* codes_frag;    // lists in fragment order
    const int32_t* code_cy;       // per stored slot
    const uint2* blk;             // per block: (global position of its first slot, slots that hold an entry) -- launch_exact_blocks;
                                  // under a selector (its keep words passed): (..., mask of the slots that hold a member)
    uint64_t nblk;                // blocks of the copy (even)
    uint32_t slab;                // consecutive blocks per workgroup (even)
    const int8_t* queries8;       // signed query bytes, row stride ks * 32
    const int32_t* query_cx;
    const float* seed_D;
    const int64_t* seed_I;
    uint32_t n, k;
    int d, metric;
    uint32_t* cnt;                // [n] candidates of the query so far (zeroed by the caller); keeps counting beyond cap
    uint2* cand;                  // [n][cap] (global position, distance bits)
    uint32_t cap;
};
// The same pass over float lists (d <= 128), on the filter's fp16 copy: codes_frag / yn are the index's (launch_frag16_from_f32), xf /
// xn / params the call's (launch_filter_queries16).  A candidate is emitted as (global position, -): launch_exact_rescore writes the
// reference's distance into the second word.
struct ExactScanF16Args {
    const float* codes_frag;      // fp16 fragments: filter_steps16(d) pieces of 1 KiB per block
    const float* yn;              // per stored slot: |y|^2 (L2) / |y| (IP)
    const uint2* blk;             // as above
    uint64_t nblk;
    uint32_t slab;
    const float* xf;              // scaled fp16 query rows, row stride 8 filter_steps16(d) floats
    const float* xn;
    const FilterParams* params;
    const float* seed_D;
    const int64_t* seed_I;
    uint32_t n, k;
    int d, metric;
    uint32_t* cnt;
    uint2* cand;
    uint32_t cap;
};
struct ExactRescoreArgs {
    uint32_t n, cap;
    int dpad, metric;
    const uint32_t* cnt;
    uint2* cand;
    const float* queries;         // the query rows as passed (stride dpad)
    const float* codes;           // the lists as stored (CSR rows, stride dpad)
};
struct ExactSelectArgs {
    uint32_t n, k, cap;
    int metric;
    int rescored;                 // 1: the fp16 pass -- candidates beyond the threshold (seed_D) sort last and are not counted
    const float* seed_D;
    const uint32_t* cnt;
    const uint2* cand;
    const int64_t* seed_I;
    const int64_t* ids;           // per stored vector
    float* D;                     // [n][k], written for the queries flagged 0
    int64_t* I;
    uint32_t* flag;               // [n] 0 answered, 1 equal distances met, 2 no threshold / more candidates than slots
    unsigned long long* totals;   // [0..2] += queries by flag, [3] += candidates emitted, [4] += candidates at or within the threshold,
                                  // [5] = max of one query's emitted count (six words, zeroed by the caller)
};
// keep (the selector's words) or null; with it, the table of a call under a selector: out[b].y is the mask of block b's slots that hold a member
void launch_exact_blocks(const uint64_t* list_off, const uint64_t* block_off, const unsigned long long* keep, uint32_t nlist, uint64_t nblk,
                         uint2* out, hipStream_t s);
void launch_identity_keys(int64_t* keys, size_t rows, uint32_t nlist, hipStream_t s);  // keys[i][l] = l
uint32_t exact_slab_blocks(uint64_t nblk, uint32_t n);
// keep: a.blk is launch_exact_blocks' table under a selector (the members' mask), else the plain one (the entries' count)
void launch_scan_all(const ExactScanArgs& a, bool keep, hipStream_t s);
void launch_scan_all_f16(const ExactScanF16Args& a, bool keep, hipStream_t s);
// the same pass for 128 < d <= 1024 (option "exact_wide"): a workgroup tile of 128 queries x 4 blocks, the query operand through LDS;
// a.slab is a multiple of 4 (exact_args.h: exact_wide_slab)
void launch_scan_all_wide_f16(const ExactScanF16Args& a, bool keep, hipStream_t s);
// the byte pass for 128 < d <= 1024 (option "exact_wide_bytes"): the same tile on the byte fragments, launch_scan_all's arguments and
// candidates (global position, the exact integer distance); a.slab is a multiple of 4 (exact_args.h: exact_wide_slab)
void launch_scan_all_wide_i8(const ExactScanArgs& a, bool keep, hipStream_t s);
void launch_exact_rescore(const ExactRescoreArgs& a, hipStream_t s);
void launch_exact_select(const ExactSelectArgs& a, hipStream_t s);
// Exact range search (amd_ivf_range_search_exact): what stands where the selection stands in the k-NN call.  collect: a query's
// min(cnt, cap) candidates are tested against the radius with the reference's strict compare, sorted by global position -- the
// reference's order: lists in list-number order, entries in position order -- and the valid run written back to the head of the
// query's candidate slots.  fill: (id, distance) of the runs into one contiguous result, query q's at off[q].
struct ExactRangeArgs {
    uint32_t n, cap;
    int metric;
    float radius;                 // the caller's, never the clamped threshold of the byte pass
    const uint32_t* cnt;          // candidates emitted per query (beyond cap only the counter moved)
    uint2* cand;                  // [n][cap] (global position, distance bits): in, and out for the valid run
    uint32_t* valid;              // [n] entries of the valid run (0 for a flagged query)
    uint32_t* flag;               // [n] 0 answered, 2 more candidates than slots
    unsigned long long* totals;   // as ExactSelectArgs::totals ([1] stays 0: a range result knows no tie)
};
struct ExactRangeFillArgs {
    uint32_t n, cap;
    const uint2* cand;
    const uint32_t* valid;
    const uint32_t* flag;         // a flagged query writes nothing
    const uint64_t* off;          // [n] where query q's run starts in labels / dist
    const int64_t* ids;           // per stored vector
    int64_t* labels;
    float* dist;
};
void launch_exact_range_collect(const ExactRangeArgs& a, hipStream_t s);
void launch_exact_range_fill(const ExactRangeFillArgs& a, hipStream_t s);

inline uint32_t subset_range_key(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
inline float subset_range_value(uint32_t key) {
    const uint32_t u = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
    float x;
    memcpy(&x, &u, 4);
    return x;
}

}  // namespace amdivf
