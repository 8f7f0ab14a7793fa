// The host side of an id selector (include/auncel_amd.h: amd_ivf_subset, amd_ivf_selector_create): which kinds there are, which
// arguments they take, and what the host prepares for the membership pass (ivf_subset.hip) -- the per-list runs of a SLICE and the
// sorted ids of an ID_BATCH.  Plain C++, nothing of the device in it: both callers share it, and it builds on its own
// (tests/cpp/selector_args_main.cpp runs it under the address and undefined-behaviour sanitizers).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace amdivf {

constexpr int SUBSET_ID_RANGE = 0, SUBSET_ID_MOD = 1, SUBSET_SLICE = 2, SUBSET_ID_BITS = 5, SUBSET_ID_BATCH = 6;

// empty: the arguments are valid; else the message of the refusal (`what`: the caller's name, the first word of the message)
inline std::string selector_args_error(const char* what, int type, int64_t a1, int64_t a2, const void* sel, size_t nsel, uint64_t ntotal) {
    const std::string w(what);
    const bool by_sel = type == SUBSET_ID_BITS || type == SUBSET_ID_BATCH;
    if (type != SUBSET_ID_RANGE && type != SUBSET_ID_MOD && type != SUBSET_SLICE && !by_sel)
        return w + ": unknown subset type (by-list subsets are made on the host)";
    if (type == SUBSET_ID_MOD && a1 <= 0) return w + ": ID_MOD wants a1 > 0";
    if (type == SUBSET_SLICE && (a1 < 0 || a1 > a2 || (uint64_t)a2 > ntotal)) return w + ": SLICE wants 0 <= a1 <= a2 <= ntotal";
    if (by_sel && !sel && nsel) return w + ": null selector";
    return std::string();
}

// IndexIVF::copy_subset_to, type 2: the run [runs[2 l], runs[2 l + 1]) of every list from the running count (list_off: nlist + 1)
inline std::vector<uint64_t> selector_slice_runs(const uint64_t* list_off, size_t nlist, int64_t a1, int64_t a2) {
    std::vector<uint64_t> runs(2 * nlist, 0);
    const uint64_t nt = list_off[nlist];
    if (nt == 0) return runs;
    uint64_t cut1 = 0, cut2 = 0;
    for (size_t l = 0; l < nlist; l++) {
        const uint64_t next = list_off[l + 1], n1 = next * (uint64_t)a1 / nt, n2 = next * (uint64_t)a2 / nt;
        runs[2 * l] = n1 - cut1;
        runs[2 * l + 1] = n2 - cut2;
        cut1 = n1;
        cut2 = n2;
    }
    return runs;
}

// ID_BATCH: the ids ascending, each once (the device looks them up by bisection)
inline std::vector<int64_t> selector_batch(const int64_t* ids, size_t n) {
    std::vector<int64_t> batch;
    if (n) batch.assign(ids, ids + n);
    std::sort(batch.begin(), batch.end());
    batch.erase(std::unique(batch.begin(), batch.end()), batch.end());
    return batch;
}

}  // namespace amdivf
