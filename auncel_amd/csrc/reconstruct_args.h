// The host side of handing stored vectors back (include/auncel_amd.h: amd_ivf_make_direct_map, amd_ivf_reconstruct, _reconstruct_n,
// _reconstruct_from_offsets, amd_ivf_search_and_reconstruct): what the entry points refuse before anything touches a device -- null
// pointers with work to do, an id window that leaves the int64 range, a label that names no stored entry -- and the one rule that
// says what a position label means.  Plain C++, nothing of the device in it: the kernels of ivf_reconstruct.hip and the host read
// the same definitions, and it builds on its own (tests/cpp/reconstruct_args_main.cpp, which is what the address and
// undefined-behaviour sanitizers are pointed at).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define RECON_HD __host__ __device__
#else
#define RECON_HD
#endif

namespace amdivf {

// A position label, as a store_pairs search returns it and as the direct map holds it: list << 32 | offset (IndexIVF.cpp:321, 928-929).
// -1 is "no entry": the padding of a search result, an id without an entry in the map.
constexpr int64_t RECON_NONE = -1;
RECON_HD inline int64_t recon_label(uint64_t list, uint64_t offset) { return (int64_t)(list << 32 | offset); }
RECON_HD inline uint64_t recon_label_list(int64_t label) { return (uint64_t)label >> 32; }
RECON_HD inline uint64_t recon_label_offset(int64_t label) { return (uint64_t)label & 0xffffffffull; }

// The row of the resident layout that a label names (list_off: nlist + 1 running counts), or false: the label is none of -1 and a
// stored entry's position -- a list at or past nlist (every negative label but -1 decodes to one), an offset at or past its list's
// size.  Nothing is read through a label this rule refuses.
RECON_HD inline bool recon_label_row(int64_t label, const uint64_t* list_off, uint64_t nlist, uint64_t* row) {
    const uint64_t l = recon_label_list(label), o = recon_label_offset(label);
    if (l >= nlist) return false;
    if (o >= list_off[l + 1] - list_off[l]) return false;
    *row = list_off[l] + o;
    return true;
}

// whether id lies in [lo, lo + n), and where: one unsigned subtraction, right for every int64 id and lo as long as lo + n itself is
// an int64 (recon_window_error)
RECON_HD inline bool recon_in_window(int64_t id, int64_t lo, uint64_t n, uint64_t* slot) {
    *slot = (uint64_t)id - (uint64_t)lo;
    return *slot < n;
}

// ---- argument checks: empty when the arguments are valid, else the message of the refusal
// the id window [i0, i0 + ni) of amd_ivf_reconstruct_n: ni >= 0 and i0 + ni inside the int64 range (compared, never computed)
inline std::string recon_window_error(int64_t i0, int64_t ni) {
    if (ni < 0) return "reconstruct_n: ni must not be negative";
    if (i0 > 0 && ni > INT64_MAX - i0) return "reconstruct_n: i0 + ni overflows";
    return std::string();
}
inline std::string recon_n_args_error(bool have_handle, int64_t i0, int64_t ni, const void* recons) {
    if (!have_handle) return "reconstruct_n: null handle";
    const std::string w = recon_window_error(i0, ni);
    if (!w.empty()) return w;
    if (ni > 0 && !recons) return "reconstruct_n: null argument";
    return std::string();
}
// amd_ivf_reconstruct (what = "reconstruct", keys = ids) and amd_ivf_reconstruct_from_offsets (what = "reconstruct_from_offsets",
// keys = labels)
inline std::string recon_keys_args_error(const char* what, bool have_handle, size_t n, const void* keys, const void* recons) {
    const std::string w = std::string(what) + ": ";
    if (!have_handle) return w + "null handle";
    if (n > 0 && (!keys || !recons)) return w + "null argument";
    return std::string();
}
// amd_ivf_search_and_reconstruct / _resident: [start, start + n) is the resident range (0 for the form that takes rows), checked
// here only for wrapping round
inline std::string recon_search_args_error(bool have_handle, bool have_queries, size_t start, size_t n, size_t k, const void* D, const void* I,
                                           const void* recons) {
    const std::string w("search_and_reconstruct: ");
    if (!have_handle) return w + "null handle";
    if (k == 0) return w + "k must be positive";
    if (start + n < start) return w + "resident query range out of bounds";
    if (n && (!have_queries || !D || !I || !recons)) return w + "null argument";
    return std::string();
}

// the first of n ids outside [0, ntotal), or n: none (amd_ivf_reconstruct's "invalid key")
inline size_t recon_first_bad_id(const int64_t* ids, size_t n, uint64_t ntotal) {
    for (size_t i = 0; i < n; i++)
        if (ids[i] < 0 || (uint64_t)ids[i] >= ntotal) return i;
    return n;
}
// the first of n labels that is neither -1 nor a stored entry's position, or n: none
inline size_t recon_first_bad_label(const int64_t* labels, size_t n, const uint64_t* list_off, uint64_t nlist) {
    uint64_t row;
    for (size_t i = 0; i < n; i++)
        if (labels[i] != RECON_NONE && !recon_label_row(labels[i], list_off, nlist, &row)) return i;
    return n;
}

}  // namespace amdivf
