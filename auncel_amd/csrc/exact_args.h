// The host side of the exact search over the whole index (include/auncel_amd.h: amd_ivf_search_exact): what the entry points refuse
// before anything touches a device, and the one rule that says when a query's result can be read off its sorted candidates (DESIGN.md
// 13), the keep rule of the fp16 list pass over float lists, and what the forms under an id selector add: their checks, the seed's
// nprobe and the mask of a block's live slots; of the exact range search (amd_ivf_range_search_exact) its checks, the threshold
// the byte pass is given for a radius, the strict test and the candidates' key.  Plain C++, nothing of the device in it: the
// kernels of ivf_exact.hip and the host read the same definitions, and it builds on its own (tests/cpp/exact_args_main.cpp,
// exact_float_main.cpp, exact_selected_main.cpp, exact_range_main.cpp and exact_wide_bytes_main.cpp, which are what the address and undefined-behaviour
// sanitizers are pointed at).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define EXACT_HD __host__ __device__
#else
#define EXACT_HD
#endif

namespace amdivf {

// empty: the arguments are valid; else the message of the refusal.  have_queries: the query rows were passed (the resident form has
// them on the device: true); [start, start + n) is the resident range (start = 0 for the form that takes rows), checked here only
// for wrapping round -- whether it lies inside the resident queries is the handle's to say
inline std::string exact_args_error(bool have_handle, bool have_queries, size_t start, size_t n, size_t k, const void* D, const void* I) {
    const std::string w("exact search: ");
    if (!have_handle) return w + "null handle";
    if (k == 0) return w + "k must be positive";
    if (start + n < start) return w + "resident query range out of bounds";
    if (n && (!have_queries || !D || !I)) return w + "null argument";
    return std::string();
}

// ... of the forms that search under a selector (amd_ivf_search_exact_selected / _resident_selected): the same, and the selector must
// be there.  Whether it is of this index and of the lists as they are now is the handle's to say (selector_words).
inline std::string exact_selected_args_error(bool have_handle, bool have_selector, bool have_queries, size_t start, size_t n, size_t k,
                                             const void* D, const void* I) {
    if (have_handle && !have_selector) return std::string("exact search: null selector");
    return exact_args_error(have_handle, have_queries, start, n, k, D, I);
}

// The seed's nprobe under a selector that keeps `kept` of `ntotal` entries: `seed` lists hold seed x ntotal / nlist entries on
// average and so seed x kept / nlist members; ceil(seed x ntotal / kept) lists hold as many members as `seed` lists hold entries.
// kept = 0 (nothing to find) and a product beyond 64 bits: the largest value, which no nlist reaches.  The seed only sets a
// threshold: any value gives the same result.
inline uint64_t exact_selected_seed(uint64_t seed, uint64_t ntotal, uint64_t kept) {
    if (kept == 0 || (ntotal && seed > UINT64_MAX / ntotal)) return UINT64_MAX;
    const uint64_t p = seed * ntotal;
    return p / kept + (p % kept != 0);
}

// The entries of a 32-slot block that a selected list pass may emit, bit m for slot m: the slot holds an entry (m < left, left = the
// entries of the list from the block's first slot on) AND the selector keeps it (keep_half: the block's half of its keep word, bit m
// for slot m).  The AND with the `left` mask does not lean on the keep words being zero past a list's end.
EXACT_HD inline uint32_t exact_block_valid_mask(uint64_t left, uint32_t keep_half) {
    const uint32_t live = left >= 32 ? 0xffffffffu : (((uint32_t)1 << left) - 1u);
    return live & keep_half;
}
// the half of keep word `blk >> 1` that belongs to block `blk`
EXACT_HD inline uint32_t exact_block_keep_half(uint64_t word, uint64_t blk) { return (uint32_t)(word >> (32 * (blk & 1))); }

// A candidate's sort key: the order key of its distance (smaller = better, whatever the metric) above its global position.
EXACT_HD inline uint64_t exact_key(uint32_t dist_key, uint32_t position) { return ((uint64_t)dist_key << 32) | position; }

// The tie rule.  sorted: a query's candidates -- every stored entry at or within its threshold -- as exact_key values in ascending
// order, `count` of them (>= k: the threshold is the k-th distance of a search of the same lists).  The window that decides the
// result is the best min(count, k + 1): with fewer than k + 1 candidates the (k + 1)-th best entry lies beyond the threshold and so
// differs from the k-th.  True when two neighbours of the window have the same distance: then, and only then, the reference's result
// depends on the order its heap met the entries in.  The pairs looked at are (i, i + 1) for i = first, first + step, ...: the host
// passes (0, 1), a wave its lane and 64.
EXACT_HD inline bool exact_window_tied(const uint64_t* sorted, size_t count, size_t k, size_t first = 0, size_t step = 1) {
    const size_t window = count < k + 1 ? count : k + 1;
    bool tied = false;
    for (size_t i = first; i + 1 < window; i += step) tied |= (sorted[i] >> 32) == (sorted[i + 1] >> 32);
    return tied;
}

// The keep rule of the fp16 list pass over float lists (scan_all_f16_kernel; the bound is ivf_filter.hip's, the argument for the
// non-strict comparison DESIGN.md 13).  p = the fp16 matrix-core dot product brought back to the operands' scale, xn / yn = |x|^2,
// |y|^2 (L2) or |x|, |y| (IP) accumulated in double and rounded once, tau = the query's threshold, a reference distance.  Every stored
// entry whose reference distance r satisfies r <= tau (L2) / r >= tau (IP) is kept, the all-zero pair included; what else is kept is
// weeded out by the rescoring.
// The constant: (2 d + 32) 2^-24 for the fp32 roundings on either side, + 2^-10 + 2^-12 for the operands' rounding to fp16 unless every
// element of both matrices is an integer of magnitude <= 2048 (fp16 holds those as they are).
EXACT_HD inline float exact_float_constant(int d, bool operands_exact) {
    const float C = (float)(2 * d + 32) * 5.9604644775390625e-08f;
    return operands_exact ? C : C + 0.0009765625f + 0.000244140625f;
}
// per query: what the entry's side of the test is compared with, and (IP) the factor of |y|
EXACT_HD inline float exact_float_bound(bool l2, float C, float xn, float tau) { return l2 ? (1.f - C) * xn - tau : tau; }
EXACT_HD inline float exact_float_slack(bool l2, float C, float xn) { return l2 ? 0.f : C * xn; }
// per pair: L2 keeps iff 2 p - (1 - C) yn >= (1 - C) xn - tau, IP iff p + C |x| |y| >= tau
EXACT_HD inline bool exact_float_keep(bool l2, float C, float p, float yn, float bound, float slack) {
    const float t = l2 ? __builtin_fmaf(2.f, p, -((1.f - C) * yn)) : __builtin_fmaf(slack, yn, p);
    return t >= bound;
}

// Which list pass serves a call (exact_slice): 0 none -- the general way whole --, 1 the byte pass, 2 the fp16 pass + rescoring,
// 3 the workgroup-tiled ("wide") fp16 pass + rescoring (4, the wide byte pass: exact_pass_kind_bytes below).  shape: what every pass needs besides d (centroids for the seed, blocks,
// ntotal < 2^32, k < cap, k <= members; the exact range search, which has no seed and no k: blocks and ntotal < 2^32); bytes: the call runs on the lists' byte codes; float_ok: the filter's copies may be used
// (filter_available: option "filter" != 0, float lists or byte codes not in use); the two options as booleans.  Up to 128
// dimensions this is the rule that was there before the wide pass, whatever opt_wide says.  Beyond, only the wide pass exists:
// byte-coded lists have no pass there by this rule, and 1024 is where the fp16 copy's row rule changes regime (ivf_filter.hip: half_scale_of).
// What the caller still has to establish for 2 and 3: ensure_frag16 and a usable fp16 scale of the query rows.
constexpr int EXACT_NARROW_MAX_D = 128, EXACT_WIDE_MAX_D = 1024;
inline int exact_pass_kind(int d, bool shape, bool bytes, bool float_ok, bool opt_float, bool opt_wide) {
    if (!shape || d < 1) return 0;
    if (d <= EXACT_NARROW_MAX_D) return bytes ? 1 : (float_ok && opt_float ? 2 : 0);
    if (d <= EXACT_WIDE_MAX_D) return !bytes && float_ok && opt_float && opt_wide ? 3 : 0;
    return 0;
}
// ... with the byte pass beyond 128 dimensions (scan_all_wide_i8_kernel): 4 exactly when the shape holds, the call
// runs on the lists' byte codes, 128 < d <= 1024 and option "exact_wide_bytes" is set; in every other case exact_pass_kind's answer.
// Where it says 4 that answer was 0 (byte-coded lists have no fp16 pass), so no answer of 1, 2 or 3 changes, and the option is
// independent of the two above.  A byte pass like 1: byte_queries, no fp16 operands, no rescoring.
inline int exact_pass_kind_bytes(int d, bool shape, bool bytes, bool float_ok, bool opt_float, bool opt_wide, bool opt_wide_bytes) {
    if (shape && bytes && d > EXACT_NARROW_MAX_D && d <= EXACT_WIDE_MAX_D && opt_wide_bytes) return 4;
    return exact_pass_kind(d, shape, bytes, float_ok, opt_float, opt_wide);
}
// the passes whose candidates carry the byte scans' exact integer distance
inline bool exact_kind_is_bytes(int kind) { return kind == 1 || kind == 4; }

// ---- exact range search (amd_ivf_range_search_exact)
// empty: the arguments are valid; else the message of the refusal.  As exact_args_error, with the lims where k-NN has (D, I): they are
// written for every n, n = 0 included (lims[0] = 0).
inline std::string exact_range_args_error(bool have_handle, bool have_queries, size_t start, size_t n, const void* lims) {
    const std::string w("exact range search: ");
    if (!have_handle) return w + "null handle";
    if (!lims) return w + "null lims";
    if (start + n < start) return w + "resident query range out of bounds";
    if (n && !have_queries) return w + "null argument";
    return std::string();
}
inline std::string exact_range_selected_args_error(bool have_handle, bool have_selector, bool have_queries, size_t start, size_t n, const void* lims) {
    if (have_handle && !have_selector) return std::string("exact range search: null selector");
    return exact_range_args_error(have_handle, have_queries, start, n, lims);
}

// The threshold the BYTE list passes are given for a radius.  scan_all_kernel (and scan_all_wide_i8_kernel) emits nothing for a query whose threshold is NaN or beyond
// 2^30 in magnitude, and works in 32-bit integers around it; a radius may be any float.  The byte rule bounds every distance the pass
// can meet by d m^2 <= 2^24 in magnitude (L2: 0 <= dis; IP: |dis| <= d m^2), so a radius beyond +-2^28 decides like +-2^28: on the
// full side every entry passes `dis <= 2^28` / `dis >= -2^28`, on the empty side none passes `dis <= -2^28` / `dis >= 2^28`.  Inside
// the range the radius is returned as it is.  *none: the radius is NaN -- the reference's compare is false for every entry, there is
// nothing to pass over the lists for.  The strict test behind the pass always uses the caller's radius, never this value.
constexpr float EXACT_RANGE_CLAMP = 268435456.f;  // 2^28
constexpr float EXACT_SCAN_GUARD = 1073741824.f;  // 2^30: scan_all_kernel's own limit
inline float exact_range_threshold(float radius, bool* none) {
    *none = radius != radius;
    if (*none) return 0.f;
    return radius > EXACT_RANGE_CLAMP ? EXACT_RANGE_CLAMP : radius < -EXACT_RANGE_CLAMP ? -EXACT_RANGE_CLAMP : radius;
}
// the reference's range test (C::cmp(radius, dis): CMax for L2, CMin for the inner product), strict on either side
EXACT_HD inline bool exact_range_within(bool l2, float radius, float dis) { return l2 ? radius > dis : radius < dis; }
// A range candidate's sort key: its global position (unique per stored entry: the order is determined) above its distance's bits;
// invalid candidates take EXACT_RANGE_INVALID, which no valid key equals (a position is below 2^32 - 1: ntotal < 2^32 - 1).
constexpr uint64_t EXACT_RANGE_INVALID = ~(uint64_t)0;
EXACT_HD inline uint64_t exact_range_key(uint32_t position, uint32_t dist_bits) { return ((uint64_t)position << 32) | dist_bits; }

// The wide passes' tile (scan_all_wide_f16_kernel, scan_all_wide_i8_kernel): four waves walk a slab in chunks of four consecutive blocks, wave w block w; the
// query operand goes through LDS in stages of `sp` pieces.
constexpr uint32_t EXACT_WIDE_QUERIES = 128, EXACT_WIDE_CHUNK = 4;
// stages that cover J pieces
EXACT_HD inline int exact_wide_stages(int J, int sp) { return (J + sp - 1) / sp; }
// the slab of the narrow passes rounded up to whole chunks
inline uint32_t exact_wide_slab(uint32_t slab) { return (slab + (EXACT_WIDE_CHUNK - 1)) & ~(EXACT_WIDE_CHUNK - 1); }
// blocks of the chunk that starts at block c of a slab that ends before block B1 (c < B1): 4, or 2 in a stream's last chunk
EXACT_HD inline uint32_t exact_wide_chunk_blocks(uint64_t c, uint64_t B1) {
    return B1 - c < EXACT_WIDE_CHUNK ? (uint32_t)(B1 - c) : EXACT_WIDE_CHUNK;
}
// the block wave w computes in that chunk: its own, or -- where the chunk has none for it -- the chunk's first, result dropped
EXACT_HD inline uint64_t exact_wide_wave_block(uint64_t c, uint64_t B1, uint32_t w) { return w < exact_wide_chunk_blocks(c, B1) ? c + w : c; }

}  // namespace amdivf
