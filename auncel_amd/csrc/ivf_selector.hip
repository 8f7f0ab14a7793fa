// Search under an id selector (amd_ivf_selector_create, amd_ivf_search_selected): the selector is one keep bit per stored entry, in
// the membership pass's own layout (ivf_subset.hip: a word per 64 entries of ONE list, list l's words from block_off[l] / 2), and a
// search reads the parent's lists as they are.  What brings the bits into a round is keep_rows_kernel: the rounds already carry a
// mask word per 64 candidates of a row, a row is the candidates of one list in list order, so word j of a row lines up with keep word
// j of its list -- one pass over the round's mask words, 8 bytes in and 8 out per 64 candidates, behind the round's scan.  The
// selection behind it is the masked walk it always was: no candidate that is not a member is ever seen.
// Selectors of one index share that layout, so they combine word by word (amd_ivf_selector_combine: selector_combine_kernel).
#include <hip/hip_runtime.h>

#include "ivf_dev.h"

namespace amdivf {

namespace {

// a wave per list: the set bits of its words
__global__ __launch_bounds__(256) void selector_list_kept_kernel(const uint32_t* __restrict__ count, const uint64_t* __restrict__ boff, uint32_t nlist,
                                                                 uint32_t* __restrict__ kept) {
    const uint32_t l = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (l >= nlist) return;
    const uint64_t w0 = boff[l] >> 1, w1 = boff[l + 1] >> 1;
    uint32_t sum = 0;
    for (uint64_t w = w0 + lane; w < w1; w += 64) sum += count[w];
    sum = wave_sum_u32(sum);
    if (lane == 0) kept[l] = sum;
}

// amd_ivf_selector_combine.  A wave per list, its lanes stride over the list's words, 8 bytes in per operand and 8 out; what a word
// may hold comes from the list's length, never from the operands -- ~a sets the tail of the last used word and every padding word,
// and a dense round would take those bits for candidates.  The counts ride along: no second pass, no shared counter.
__global__ __launch_bounds__(256) void selector_combine_kernel(int op, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                               const uint64_t* __restrict__ off, const uint64_t* __restrict__ boff, uint32_t nlist,
                                                               uint64_t* __restrict__ keep, uint32_t* __restrict__ count,
                                                               uint32_t* __restrict__ kept) {
    const uint32_t l = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (l >= nlist) return;
    const uint64_t w0 = boff[l] >> 1, w1 = boff[l + 1] >> 1, n = off[l + 1] - off[l];
    uint32_t sum = 0;
    for (uint64_t w = w0 + lane; w < w1; w += 64) {
        const uint64_t r = selector_combine_word(op, a[w], b ? b[w] : 0ull) & selector_valid_word(n, w - w0);
        const uint32_t c = (uint32_t)__popcll(r);
        keep[w] = r;
        count[w] = c;
        sum += c;
    }
    sum = wave_sum_u32(sum);
    if (lane == 0) kept[l] = sum;
}

// A wave per row, a lane per word, 64 words a trip (a row of the bench index is ~40 words: one trip); the rows of a round are dealt
// to the resident waves in turn.  WRITE: a dense round (the scan stored every distance and no mask); else the scan's marks are
// narrowed to the members.  Every word of a row is written, none behind it: what the selection's walk reads.
template <bool WRITE> __global__ __launch_bounds__(256) void keep_rows_kernel(KeepArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t nseg = a.nseg_dev ? *a.nseg_dev : a.nseg;
    const uint32_t stride = gridDim.x * 4u;
    for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < nseg; r += stride) {
        const int key = a.seg_list[r];
        if (key < 0 || (uint32_t)key >= a.nlist) continue;  // (an absent probe: the row is empty)
        const uint32_t n = (uint32_t)(a.list_off[key + 1] - a.list_off[key]);
        const uint32_t words = (n + 63u) >> 6;
        const unsigned long long* kw = a.keep + (a.block_off[key] >> 1);
        unsigned long long* mw = a.mask + (a.seg_off[r] >> 6);
        for (uint32_t j = (uint32_t)lane; j < words; j += 64u) {
            const unsigned long long k = kw[j];
            mw[j] = WRITE ? k : (__builtin_nontemporal_load(mw + j) & k);
        }
    }
}

// keep_rows_kernel with a selector per query (amd_ivf_search_*_selected_each).  The keep-word base of a row comes from the row's
// query, and a round's rows of one query are consecutive, so no wave searches for its query: wave w stands for launch position
// w / P and the query's row j = w % P (P = the round's probe count; a query that was given more rows -- a run of equal coarse
// distances taken whole -- walks them P apart), idle when the query has fewer.  Position -> query: qsel, the table the selection
// kernels go through to reach a query's row of D / I.  qsel[p] is the query's SLOT, which is its number in the caller's arrays --
// a budget cut defers queries to a later pass and later rounds compact the unfinished ones, so position p of a round is not query p
// -- and seg_count / seg_begin / sel_of are all indexed by that slot.  Two wave-uniform loads per row (selector number, base), then
// the 8 bytes in and 8 out per lane and word of keep_rows_kernel.  No LDS, no atomics, no barrier.
template <bool WRITE> __global__ __launch_bounds__(256) void keep_rows_each_kernel(KeepEachArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t nq = a.nq_dev ? *a.nq_dev : a.nq;
    const uint32_t P = a.probes;
    const unsigned long long total = (unsigned long long)nq * P, stride = (unsigned long long)gridDim.x * 4u;
    for (unsigned long long w = (unsigned long long)blockIdx.x * 4u + wave; w < total; w += stride) {
        const uint32_t slot = a.qsel[w / P];
        const uint32_t cnt = a.seg_count[slot], begin = a.seg_begin[slot];
        uint32_t j = (uint32_t)(w % P);
        if (j >= cnt) continue;
        const uint32_t sel = a.sel_of[slot];
        if (sel >= a.nsel) continue;  // (refused on the host: never reached)
        const unsigned long long* keep = a.keeps[sel];
        for (; j < cnt; j += P) {
            const uint32_t r = begin + j;
            const int key = a.seg_list[r];
            if (key < 0 || (uint32_t)key >= a.nlist) continue;  // (an absent probe: the row is empty)
            const uint32_t n = (uint32_t)(a.list_off[key + 1] - a.list_off[key]);
            const uint32_t words = (n + 63u) >> 6;
            const unsigned long long* kw = keep + (a.block_off[key] >> 1);
            unsigned long long* mw = a.mask + (a.seg_off[r] >> 6);
            for (uint32_t i = (uint32_t)lane; i < words; i += 64u) {
                const unsigned long long k = kw[i];
                mw[i] = WRITE ? k : (__builtin_nontemporal_load(mw + i) & k);
            }
        }
    }
}

}  // namespace

void launch_selector_list_kept(const uint32_t* count, const uint64_t* block_off, uint32_t nlist, uint32_t* kept, hipStream_t s) {
    LAUNCH(selector_list_kept_kernel, dim3((nlist + 3) / 4), dim3(256), 0, s, count, block_off, nlist, kept);
}

void launch_selector_combine(int op, const uint64_t* a, const uint64_t* b, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist,
                             uint64_t* keep, uint32_t* count, uint32_t* kept, hipStream_t s) {
    if (nlist == 0) return;
    LAUNCH(selector_combine_kernel, dim3((nlist + 3) / 4), dim3(256), 0, s, op, a, b, list_off, block_off, nlist, keep, count, kept);
}

void launch_keep_rows(const KeepArgs& a, hipStream_t s) {
    const uint32_t want = a.nseg_dev ? a.nseg_hint : a.nseg;
    if (want == 0) return;
    const uint32_t grid = std::min<uint32_t>((want + 3u) / 4u, 8192u);
    if (a.write) LAUNCH(keep_rows_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else LAUNCH(keep_rows_kernel<false>, dim3(grid), dim3(256), 0, s, a);
}

// (the grid from the same hints: a wave per expected row, which is what nq x P comes to when every query takes P rows)
void launch_keep_rows_each(const KeepEachArgs& a, hipStream_t s) {
    if (a.probes == 0 || a.nsel == 0) throw std::runtime_error("keep_rows_each: no probes or no selectors");
    const unsigned long long want = a.nq_dev ? a.nseg_hint : (unsigned long long)a.nq * a.probes;
    if (want == 0) return;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>((want + 3u) / 4u, 8192u);
    if (a.write) LAUNCH(keep_rows_each_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else LAUNCH(keep_rows_each_kernel<false>, dim3(grid), dim3(256), 0, s, a);
}

}  // namespace amdivf
