// The host side of an id selector (include/auncel_amd.h: amd_ivf_subset, amd_ivf_selector_create): which kinds there are, which
// arguments they take, and what the host prepares for the membership pass (ivf_subset.hip) -- the per-list runs of a SLICE and the
// sorted ids of an ID_BATCH.  Plain C++, nothing of the device in it: both callers share it, and it builds on its own
// (tests/cpp/selector_args_main.cpp runs it under the address and undefined-behaviour sanitizers).  So are the operand checks of
// amd_ivf_selector_combine and the one rule that says which bits of a keep word stand for entries (selector_valid_word: the combine
// kernel and tests/cpp/selector_combine_main.cpp read the same definition), and the checks of a search under a selector per query
// (amd_ivf_search_*_selected_each: selector_each_*_error, tests/cpp/selector_each_main.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define SELECTOR_HD __host__ __device__
#else
#define SELECTOR_HD
#endif

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

// ---- amd_ivf_selector_combine
constexpr int SELECTOR_AND = 0, SELECTOR_OR = 1, SELECTOR_ANDNOT = 2, SELECTOR_NOT = 3;

// what the checks read of an operand: the index it was made on and that index's layout_gen at the time
struct SelectorOperand {
    const void* index;
    uint64_t gen;
};

// empty: the operands can be combined; else the message of the refusal.  a / b: null where the caller passed none; index_gen: the
// layout_gen of a's index as it is now (read only behind the null checks); tickets: searches submitted on it and not yet waited for
inline std::string selector_combine_error(int op, const SelectorOperand* a, const SelectorOperand* b, bool have_out, uint64_t index_gen, bool tickets) {
    const std::string w("selector combine: ");
    if (!a || !have_out) return w + "null argument";
    if (op != SELECTOR_AND && op != SELECTOR_OR && op != SELECTOR_ANDNOT && op != SELECTOR_NOT) return w + "unknown op";
    if (op == SELECTOR_NOT && b) return w + "NOT takes one operand (b must be null)";
    if (op != SELECTOR_NOT && !b) return w + "a binary op wants two operands (null b)";
    if (b && b->index != a->index) return w + "the operands were made on different indexes";
    if (a->gen != index_gen || (b && b->gen != index_gen))
        return w + "an operand is stale: the index's lists were given or changed after it was made; make a new one";
    if (tickets) return w + "tickets are still out: wait for them before making a selector";
    return std::string();
}

// ---- amd_ivf_search_*_selected_each: a table of selectors and one index into it per query
// What the caller passed at all: read before anything behind a pointer is.  empty: go on to selector_each_error.
inline std::string selector_each_null_error(const char* what, bool have_h, bool have_sels, bool have_sel_of, bool have_x, bool have_D, bool have_I,
                                            size_t nsel, size_t n) {
    const std::string w = std::string(what) + ": ";
    if (!have_h || !have_sels || !have_sel_of || !have_D || !have_I) return w + "null argument";
    if (!have_x && n > 0) return w + "null queries";
    if (nsel == 0 && n > 0) return w + "no selectors (nsel == 0) for " + std::to_string(n) + " queries";
    return std::string();
}
// The table and the indexes.  ops[j]: what the checks read of sels[j] (index == nullptr: the entry is null); index / index_gen: the
// searching handle's index and its layout_gen as it is now.  Every entry of the table is checked, used by a query or not.
inline std::string selector_each_error(const char* what, const SelectorOperand* ops, size_t nsel, const uint32_t* sel_of, size_t n, const void* index,
                                       uint64_t index_gen) {
    const std::string w = std::string(what) + ": ";
    for (size_t j = 0; j < nsel; j++) {
        const std::string at = "selector " + std::to_string(j) + " of the table ";
        if (!ops[j].index) return w + at + "is null";
        if (ops[j].index != index) return w + at + "was made on another index";
        if (ops[j].gen != index_gen)
            return w + at + "is stale: the index's lists were given or changed after it was made (amd_ivf_set_lists, amd_ivf_add, "
                            "amd_ivf_update_lists, amd_ivf_remove_ids); make a new one";
    }
    for (size_t i = 0; i < n; i++)
        if ((size_t)sel_of[i] >= nsel)
            return w + "sel_of[" + std::to_string(i) + "] = " + std::to_string(sel_of[i]) + " is not below nsel = " + std::to_string(nsel);
    return std::string();
}
// resident queries [start, start + n) of n_resident: a range that wraps is refused as such, not as whatever start + n comes to
inline std::string selector_each_range_error(const char* what, size_t start, size_t n, size_t n_resident) {
    const std::string w = std::string(what) + ": ";
    if (start + n < start) return w + "the resident query range wraps";
    if (start + n > n_resident) return w + "resident query range out of bounds";
    return std::string();
}

// The bits of keep word j of a list of n entries that stand for entries: all 64 while the word lies inside the list, the low n - 64 j
// in the word the list ends in, none in a word behind it (a list's block count is rounded up to even, and may be padded further).
// Every reader of keep words relies on the other bits being zero: a dense round's mask is the keep words themselves.
SELECTOR_HD inline uint64_t selector_valid_word(uint64_t n, uint64_t j) {
    const uint64_t first = j << 6;
    if (j >= ((uint64_t)1 << 58) || first >= n) return 0;
    const uint64_t left = n - first;
    return left >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << left) - 1);
}

SELECTOR_HD inline uint64_t selector_combine_word(int op, uint64_t a, uint64_t b) {
    return op == SELECTOR_AND ? (a & b) : op == SELECTOR_OR ? (a | b) : op == SELECTOR_ANDNOT ? (a & ~b) : ~a;
}

}  // namespace amdivf
