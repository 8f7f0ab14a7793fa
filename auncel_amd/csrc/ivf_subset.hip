// A subset of a device-resident index, cut on the device (amd_ivf_subset): the rows are in HBM already, in the engine's own layout, and
// a subset is a stable compaction of them.  Three passes, each bound by memory traffic: a keep-mask of the parent's entries (a bit
// per entry, a word per 64 entries of one list), the kept lists' offsets from the words' counts, and the copy of the kept rows and
// ids to places that are a pure function of the mask -- the same bytes on every run, whatever order the waves run in.
#include <hip/hip_runtime.h>

#include "ivf_dev.h"

namespace amdivf {

namespace {

// largest l < nlist with boff[l] / 2 <= w (the list of mask word w; empty lists share their successor's offset)
__device__ __forceinline__ uint32_t list_of_word(const uint64_t* __restrict__ boff, uint32_t nlist, uint64_t w) {
    uint32_t lo = 0, hi = nlist;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((boff[mid] >> 1) <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool is_member(const SubsetSel& sel, int64_t id, uint64_t pos, uint32_t l) {
    switch (sel.type) {
        case SUBSET_ID_RANGE: return sel.a1 <= id && id < sel.a2;
        case SUBSET_ID_MOD: return id % sel.a1 == sel.a2;
        case SUBSET_SLICE: return sel.runs[2 * (uint64_t)l] <= pos && pos < sel.runs[2 * (uint64_t)l + 1];
        case SUBSET_ID_BITS: return id >= 0 && ((uint64_t)id >> 6) < sel.nsel && ((sel.bits[(uint64_t)id >> 6] >> (id & 63)) & 1);
        default: {  // SUBSET_ID_BATCH
            uint64_t lo = 0, hi = sel.nsel;
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (sel.batch[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            return lo < sel.nsel && sel.batch[lo] == id;
        }
    }
}

// a wave per mask word, a lane per entry: the wave's 64 verdicts are one ballot, stored by one lane
__global__ __launch_bounds__(256) void subset_member_kernel(const int64_t* __restrict__ ids, const uint64_t* __restrict__ off,
                                                            const uint64_t* __restrict__ boff, uint32_t nlist, uint64_t nwords, SubsetSel sel,
                                                            uint64_t* __restrict__ mask, uint32_t* __restrict__ count) {
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= nwords) return;
    const uint32_t l = list_of_word(boff, nlist, w);
    const uint64_t pos = (w - (boff[l] >> 1)) * 64 + lane, size = off[l + 1] - off[l];
    bool keep = false;
    if (pos < size) keep = is_member(sel, ids[off[l] + pos], pos, l);  // (the lanes past the list's end stay out of the word)
    const uint64_t b = __ballot(keep);
    if (lane == 0) {
        mask[w] = b;
        count[w] = (uint32_t)__popcll(b);
    }
}

// a wave per list: the exclusive prefix of its words' counts, and their sum
__global__ __launch_bounds__(256) void subset_rank_kernel(const uint32_t* __restrict__ count, const uint64_t* __restrict__ boff, uint32_t nlist,
                                                          uint32_t* __restrict__ rank_base, uint64_t* __restrict__ list_total) {
    const uint32_t l = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (l >= nlist) return;
    const uint64_t w0 = boff[l] >> 1, w1 = boff[l + 1] >> 1;
    uint32_t run = 0;
    for (uint64_t w = w0; w < w1; w += 64) {
        const uint64_t i = w + lane;
        const uint32_t c = i < w1 ? count[i] : 0u;
        uint32_t x = c;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, o);
            if (lane >= o) x += y;
        }
        if (i < w1) rank_base[i] = run + x - c;
        run += (uint32_t)__shfl((int)x, 63);
    }
    if (lane == 0) list_total[l] = run;
}

// one workgroup: the lists' totals into offsets and the block table of the padded copies
__global__ __launch_bounds__(256) void subset_offsets_kernel(const uint64_t* __restrict__ list_total, uint32_t nlist, uint64_t* __restrict__ new_off,
                                                             uint64_t* __restrict__ new_boff) {
    __shared__ uint64_t s_n[256], s_b[256];
    const uint32_t t = threadIdx.x, per = (nlist + 255) / 256;
    const uint32_t l0 = t * per < nlist ? t * per : nlist, l1 = l0 + per < nlist ? l0 + per : nlist;
    uint64_t n = 0, b = 0;
    for (uint32_t l = l0; l < l1; l++) {
        n += list_total[l];
        b += mfma_list_blocks(list_total[l]);
    }
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
        new_off[nlist] = rn;
        new_boff[nlist] = rb;
    }
    __syncthreads();
    n = s_n[t];
    b = s_b[t];
    for (uint32_t l = l0; l < l1; l++) {
        new_off[l] = n;
        new_boff[l] = b;
        n += list_total[l];
        b += mfma_list_blocks(list_total[l]);
    }
}

// a wave per mask word: the kept entries of the word go to consecutive rows of the new layout, 16-byte loads and stores, four in
// flight per lane; the range of the values (IntRange) rides on the loads
__global__ __launch_bounds__(256) void subset_compact_kernel(const float* __restrict__ old_codes, const int64_t* __restrict__ old_ids,
                                                             const uint64_t* __restrict__ old_off, const uint64_t* __restrict__ old_boff,
                                                             uint32_t nlist, uint64_t nwords, const uint64_t* __restrict__ mask,
                                                             const uint32_t* __restrict__ rank_base, const uint64_t* __restrict__ new_off, int dpad,
                                                             float* __restrict__ codes, int64_t* __restrict__ ids, uint32_t* range) {
    __shared__ uint64_t s_src[4][64];
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (w >= nwords) return;
    const uint64_t m = mask[w];
    if (m == 0) return;
    const uint32_t l = list_of_word(old_boff, nlist, w);
    const uint64_t src0 = old_off[l] + (w - (old_boff[l] >> 1)) * 64, dst0 = new_off[l] + rank_base[w];
    const uint32_t nrows = (uint32_t)__popcll(m);
    if ((m >> lane) & 1) {
        const uint32_t r = (uint32_t)__popcll(m & ((1ull << lane) - 1));  // (kept entries below this one)
        s_src[wave][r] = src0 + lane;
        ids[dst0 + r] = old_ids[src0 + lane];
    }
    wave_sync();
    const uint32_t nsteps = (uint32_t)dpad >> 2, total = nrows * nsteps;
    const float4* src4 = reinterpret_cast<const float4*>(old_codes);
    float4* dst4 = reinterpret_cast<float4*>(codes) + dst0 * nsteps;
    RangeWatch watch;
    for (uint32_t i0 = lane; i0 < total; i0 += 4 * 64) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t i = i0 + u * 64;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < total) {
                const uint32_t r = i / nsteps;
                v[u] = src4[s_src[wave][r] * nsteps + (i - r * nsteps)];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t i = i0 + u * 64;
            if (i < total) dst4[i] = v[u];
            watch.look(v[u]);
        }
    }
    watch.commit(range, lane);
}

}  // namespace

void launch_subset_member(const int64_t* ids, const uint64_t* list_off, const uint64_t* block_off, uint32_t nlist, uint64_t nwords,
                          const SubsetSel& sel, uint64_t* mask, uint32_t* count, hipStream_t s) {
    if (nwords == 0) return;
    LAUNCH(subset_member_kernel, dim3((unsigned)((nwords + 3) / 4)), dim3(256), 0, s, ids, list_off, block_off, nlist, nwords, sel, mask, count);
}

void launch_subset_offsets(const uint32_t* count, const uint64_t* block_off, uint32_t nlist, uint32_t* rank_base, uint64_t* list_total,
                           uint64_t* new_off, uint64_t* new_block_off, hipStream_t s) {
    LAUNCH(subset_rank_kernel, dim3((nlist + 3) / 4), dim3(256), 0, s, count, block_off, nlist, rank_base, list_total);
    LAUNCH(subset_offsets_kernel, dim3(1), dim3(256), 0, s, list_total, nlist, new_off, new_block_off);
}

void launch_subset_compact(const float* old_codes, const int64_t* old_ids, const uint64_t* old_off, const uint64_t* old_block_off, uint32_t nlist,
                           uint64_t nwords, const uint64_t* mask, const uint32_t* rank_base, const uint64_t* new_off, int dpad, float* codes,
                           int64_t* ids, uint32_t* range, hipStream_t s) {
    if (nwords == 0) return;
    LAUNCH(subset_compact_kernel, dim3((unsigned)((nwords + 3) / 4)), dim3(256), 0, s, old_codes, old_ids, old_off, old_block_off, nlist, nwords,
           mask, rank_base, new_off, dpad, codes, ids, range);
}

}  // namespace amdivf
