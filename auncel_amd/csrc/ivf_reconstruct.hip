// Stored vectors back from a device-resident index (amd_ivf_make_direct_map, amd_ivf_reconstruct*, amd_ivf_search_and_reconstruct):
// the rows are in HBM already, so handing some of them back is a gather, and finding them by id is one pass over the resident ids.
// Two kernels, both pure data movement: id_positions_kernel writes the position of every stored id of a window into a
// table -- the reference's direct_map when the window is [0, ntotal) --, gather_rows_kernel turns position labels into compact rows
// and ids.  Nothing here depends on the order the waves run in: the table takes the LARGEST position of an id (a 64-bit atomic
// maximum), which is what the reference's list-by-list, offset-by-offset loops leave behind (IndexIVF.cpp:311-323, 881-899).
#include <hip/hip_runtime.h>

#include "ivf_dev.h"
#include "reconstruct_args.h"

namespace amdivf {

namespace {

// largest l < nlist with off[l] <= g (the list of entry g < off[nlist]; empty lists share their successor's offset)
__device__ __forceinline__ uint32_t list_of_entry(const uint64_t* __restrict__ off, uint32_t nlist, uint64_t g) {
    uint32_t lo = 0, hi = nlist;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A lane per stored entry.  counts[0] += entries whose id lies outside [lo, lo + n); counts[1] += slots of the table that took their
// first position (exactly one of the maxima on a slot finds it empty, whichever arrives first): a ballot each, one add per wave.
__global__ __launch_bounds__(256) void id_positions_kernel(const int64_t* __restrict__ ids, const uint64_t* __restrict__ off, uint32_t nlist,
                                                           uint64_t nt, int64_t lo, uint64_t n, long long* __restrict__ table,
                                                           unsigned long long* __restrict__ counts) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool outside = false, first = false;
    if (g < nt) {
        uint64_t slot;
        if (recon_in_window(ids[g], lo, n, &slot)) {
            const uint32_t l = list_of_entry(off, nlist, g);
            const long long pos = (long long)recon_label(l, g - off[l]);
            first = __hip_atomic_fetch_max(&table[slot], pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (long long)RECON_NONE;
        } else {
            outside = true;
        }
    }
    const uint64_t bo = __ballot(outside), bf = __ballot(first);
    if ((threadIdx.x & 63) == 0) {
        if (bo) atomicAdd(&counts[0], (unsigned long long)__popcll(bo));
        if (bf) atomicAdd(&counts[1], (unsigned long long)__popcll(bf));
    }
}

// A lane per (output row, group of four columns): the row's source is 16-byte aligned and padded to dpad, so it is always read by
// one 16-byte load; the compact output takes a 16-byte store where d % 4 == 0 and the buffer is aligned (wide_out), else the up
// to four floats below d one by one -- the scalar tail, and every column when rows do not start on 16 bytes.
// Row i's label: labels[i], or table[keys[i]] (by id).  none_mode says what a label of -1 does: RECON_NONE_FILL a row of 0xFF bytes
// and id -1, RECON_NONE_SKIP nothing (found[i] = 0), RECON_NONE_ERROR the flag.  Any other label that names no stored entry, and
// a key outside the table, reads nothing, writes nothing and raises the flag: *bad = the smallest such i.
__global__ __launch_bounds__(256) void gather_rows_kernel(GatherRowsArgs a) {
    const uint32_t nsteps = (uint32_t)a.dpad >> 2;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = t / nsteps;
    if (i >= a.m) return;
    const uint32_t c4 = (uint32_t)(t - i * nsteps);
    int64_t label;
    if (a.table) {
        const int64_t key = a.keys[i];
        if (key < 0 || (uint64_t)key >= a.table_n) {
            if (c4 == 0) atomicMin(a.bad, (unsigned long long)i);
            return;
        }
        label = a.table[key];
    } else {
        label = a.labels[i];
    }
    uint64_t row = 0;
    const bool none = label == RECON_NONE;
    if (none) {
        if (a.none_mode == RECON_NONE_ERROR && c4 == 0) atomicMin(a.bad, (unsigned long long)i);
        if (a.none_mode == RECON_NONE_SKIP && c4 == 0 && a.found) a.found[i] = 0;
        if (a.none_mode != RECON_NONE_FILL) return;
    } else if (!recon_label_row(label, a.list_off, a.nlist, &row)) {
        if (c4 == 0) atomicMin(a.bad, (unsigned long long)i);
        return;
    }
    if (c4 == 0) {
        if (a.ids_out) a.ids_out[i] = none ? -1 : a.ids[row];
        if (a.found) a.found[i] = 1;
    }
    float4 v;
    if (none) {
        const float ff = __uint_as_float(0xffffffffu);
        v = make_float4(ff, ff, ff, ff);
    } else {
        v = reinterpret_cast<const float4*>(a.codes)[row * nsteps + c4];
    }
    const uint32_t c = c4 * 4;
    float* dst = a.rows + i * (uint64_t)a.d + c;
    if (a.wide_out) {
        *reinterpret_cast<float4*>(dst) = v;  // (d == dpad here: every group lies inside the row)
    } else {
        if (c + 0 < (uint32_t)a.d) dst[0] = v.x;
        if (c + 1 < (uint32_t)a.d) dst[1] = v.y;
        if (c + 2 < (uint32_t)a.d) dst[2] = v.z;
        if (c + 3 < (uint32_t)a.d) dst[3] = v.w;
    }
}

}  // namespace

void launch_id_positions(const int64_t* ids, const uint64_t* list_off, uint32_t nlist, uint64_t nt, int64_t lo, uint64_t n, int64_t* table,
                         unsigned long long* counts, hipStream_t s) {
    if (nt == 0 || n == 0) return;
    LAUNCH(id_positions_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, ids, list_off, nlist, nt, lo, n,
           reinterpret_cast<long long*>(table), counts);
}

void launch_gather_rows(const GatherRowsArgs& a, hipStream_t s) {
    if (a.m == 0) return;
    const uint64_t threads = a.m * (uint64_t)(a.dpad >> 2), blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffull) throw std::runtime_error("gather_rows: too many rows for one launch");
    LAUNCH(gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
}

}  // namespace amdivf
