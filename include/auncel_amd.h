/* auncel_amd.h -- C ABI of the MI355X (gfx950) IVF-Flat search engine.
 *
 * This is the drop-in boundary for Auncel's IVF-Flat search hot path: plain pointers and
 * sizes, no C++/torch types.  Every entry point names the reference interface it replaces
 * (paths relative to the reference repo's Auncel/ directory).  The host-side C++ mirror of
 * the reference classes (auncel_amd/csrc/host/, namespace faiss) calls only these functions;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions (same as the reference's c_api, c_api/error_c.h:20-33, macros_impl.h:22-58):
 *   - every function returns 0 on success, -1 unknown error, -2 engine exception (what the
 *     reference raises as FaissException: invalid key, arcos domain, cosine-theorem
 *     precondition, tune without tuner...), -4 std::exception / HIP runtime failure;
 *     amd_ivf_last_error() returns the message of the last failure on the calling thread.
 *   - matrices are compact row-major; ids are int64 ("long" idx_t, Index.h:67); outputs are
 *     fully overwritten, sorted best first, padded with id -1 and +/-FLT_MAX (Heap.h:317-320).
 *   - x / D / I / keys / coarse_dis arguments are HOST pointers unless the function name ends
 *     in _dev, in which case they are device pointers on the handle's GPU.
 *   - there is NO CPU fallback: without a usable HIP device every call fails with -4.
 */
#ifndef AUNCEL_AMD_H
#define AUNCEL_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMD_IVF_METRIC_INNER_PRODUCT 0 /* MetricType, Index.h:49-52 */
#define AMD_IVF_METRIC_L2 1

typedef struct amd_ivf amd_ivf_t;

const char* amd_ivf_last_error(void);
int amd_ivf_device_count(int* count);

/* ---- index lifetime and contents ------------------------------------------------------ */

/* Self-check of an assumption the engine's device-side bookkeeping rests on: counters that exist once per XCD (statistics,
 * queries left unfinished by a round, pairs per list) are added to with workgroup-scope atomics, which the issuing XCD's L2
 * executes -- exact as long as no other XCD touches the row, and an XCD has a number below 8.  Runs the adds under contention
 * (2^20 returning adds on 8 x 1024 addresses).  out[0] adds made, out[1] sum of the counters (must equal out[0]), out[2] (XCD,
 * address) pairs whose returned values are not exactly 0 .. count - 1 (must be 0), out[3] bit mask of the XCD numbers seen.
 * amd_ivf_create runs it once per device and refuses to create an index where it fails.  (No reference counterpart: diagnostics.) */
int amd_ivf_self_check(int device, uint64_t out[4]);

/* IndexIVFFlat(quantizer, d, nlist, metric)  [IndexIVFFlat.cpp:28-33, IndexIVF.cpp:146-170] */
int amd_ivf_create(int d, size_t nlist, int metric, int device, amd_ivf_t** out);
int amd_ivf_destroy(amd_ivf_t* h);

/* A second search context over the same device-resident index: its own HIP stream, workspaces and resident
 * queries; lists, centroids, centroid table and traces stay with (and are owned by) `h`.  The reference's
 * search() / search_preassigned() are const and re-entrant over the index data (IndexIVF.h:189-207, and
 * IndexShards(threaded=true) calls them from one thread per shard, IndexShards.cpp:261-311); a context is what a
 * thread of the caller uses to keep its own batch in flight on the GPU while another thread's batch is in a
 * latency-bound phase.  Valid on a clone: set_queries, search, search_preassigned, search_resident,
 * search_adaptive(_x), stats, scan_arith, last_timing, ntotal, list_size, destroy; everything else must go through
 * `h` and returns -2 here.  Build the index first: clones do not see later add() / set_*() calls until `h` has
 * searched once, and `h` must outlive its clones. */
int amd_ivf_clone(amd_ivf_t* h, amd_ivf_t** out);

/* quantizer->add(nlist, centroids): IndexFlat::xb, row-major nlist x d  [IndexFlat.cpp:30-33] */
int amd_ivf_set_centroids(amd_ivf_t* h, const float* centroids);

/* ArrayInvertedLists contents: per list l, sizes[l] vectors codes[l] (sizes[l] x d fp32) and
 * ids[l]; copied to HBM CSR-packed  [InvertedLists.h:182-202, InvertedLists.cpp:138-196] */
int amd_ivf_set_lists(amd_ivf_t* h, const size_t* sizes, const float* const* codes, const int64_t* const* ids);

/* IndexIVFFlat::add_core: assign each vector to its nearest centroid (exact kernel) and append
 * it to that list in input order; xids == NULL -> ids ntotal..ntotal+n-1; precomputed_idx may
 * be NULL, entries < 0 are skipped  [IndexIVFFlat.cpp:41-80] */
int amd_ivf_add(amd_ivf_t* h, size_t n, const float* x, const int64_t* xids, const int64_t* precomputed_idx);

int amd_ivf_ntotal(const amd_ivf_t* h, size_t* ntotal);
int amd_ivf_list_size(const amd_ivf_t* h, size_t list_no, size_t* size);
/* InvertedLists::get_codes / get_ids: copy one list back to the host */
int amd_ivf_get_list(const amd_ivf_t* h, size_t list_no, float* codes, int64_t* ids);

/* ---- changes of the lists in place ------------------------------------------------------
 * amd_ivf_add, amd_ivf_update_lists and amd_ivf_remove_ids keep a journal of the entries they write; the next refresh of the device
 * lists (the next search; these two entry points at once) builds the new layout in HBM from the old one and the written entries
 * instead of sending every list again (option "incremental").  Either way the device then holds exactly what amd_ivf_set_lists of
 * the same lists would have made.  With tickets out (amd_ivf_submit_*), these entry points, and an amd_ivf_add that would move the
 * device layout, return -2 and leave the index as it was.  Owner only.
 *
 * entries changed since the last refresh: sizes = the nlist new list sizes; nw written entries at where[i] = list << 32 | offset
 * (offset < sizes[list]), with ids[i] and the row codes[i*d .. i*d+d).  Every entry at or past its list's old size must be
 * written; the others keep their value. */
int amd_ivf_update_lists(amd_ivf_t* h, const size_t* sizes, size_t nw, const uint64_t* where, const int64_t* ids, const float* codes);
/* IndexIVF::remove_ids with an IDSelectorBatch: the list's last entry takes a removed entry's place  [IndexIVF.cpp:955-987] */
int amd_ivf_remove_ids(amd_ivf_t* h, size_t n, const int64_t* ids, size_t* nremoved);
/* the last refresh of the device lists: {0 none / 1 incremental / 2 full, host-to-device bytes, entries written, 32-vector blocks
 * re-encoded (per copy)} */
int amd_ivf_last_update(amd_ivf_t* h, uint64_t out[4]);
/* 64-bit digests of the device layout over its logical extent, padding included: offsets + block tables, rows, ids, byte
 * fragments + cy, fp16 copy + yn + its range, fp32 copy + yn, lane copy, flags (0 for a copy that does not exist).  Refreshes the
 * device lists first.  A test aid: it reads every buffer back. */
int amd_ivf_layout_digest(amd_ivf_t* h, uint64_t out[8]);

/* ---- a subset index, cut on the device -------------------------------------------------
 * IndexIVF::copy_subset_to  [IndexIVF.cpp, subset types 0, 1, 2] and selectors of ids, applied to the index that is resident in
 * HBM: *out is an index of its own on h's device -- same d, nlist, metric -- whose list l holds the members of h's list l, in h's
 * order, with their ids.  No list row crosses PCIe: a keep-mask, the kept lists' offsets and a stable compaction of rows and ids are
 * made by three passes over the device lists, and the device then holds exactly what amd_ivf_set_lists of the
 * filtered lists would have made (byte eligibility is taken over the kept values: a subset can qualify where its parent does not).
 * Centroids, the centroid table of amd_ivf_set_interdis, the tuner and the options are copied from h; the subset borrows nothing,
 * so h may be destroyed first.  A pending amd_ivf_add of h is applied first; h itself is not changed.
 * The subset is read-only: every search entry point, amd_ivf_clone, tickets, range search, the scanner calls, amd_ivf_get_list,
 * sizes, options and amd_ivf_subset of it work; amd_ivf_add, amd_ivf_set_lists, amd_ivf_update_lists, amd_ivf_remove_ids and
 * amd_ivf_set_centroids return -2.  Returns -2 before the device is touched for: a null h / out, h a clone, tickets out on h, an
 * unknown type, a1 <= 0 (ID_MOD), a1 > a2 or a2 > ntotal (SLICE), sel == NULL with nsel > 0.  An empty result is a valid index
 * of ntotal 0.  (Types 3 and 4, the by-list subsets of the class mirror, stay on the host.) */
#define AMD_IVF_SUBSET_ID_RANGE 0 /* a1 <= id < a2                           copy_subset_to type 0 */
#define AMD_IVF_SUBSET_ID_MOD 1   /* id % a1 == a2 (C++ %, as the reference) copy_subset_to type 1 */
#define AMD_IVF_SUBSET_SLICE 2    /* entries [n1, n2) of the running count,  copy_subset_to type 2 */
#define AMD_IVF_SUBSET_ID_BITS 5  /* sel = uint64 words, nsel of them: id is a member iff 0 <= id < 64 nsel and bit id is set */
#define AMD_IVF_SUBSET_ID_BATCH 6 /* sel = nsel int64 ids in any order, repeats allowed (IDSelectorBatch) */
int amd_ivf_subset(amd_ivf_t* h, int subset_type, int64_t a1, int64_t a2, const void* sel, size_t nsel, amd_ivf_t** out);
/* {entries looked at, entries kept, host-to-device bytes, device-to-host bytes} of the call that made `sub` */
int amd_ivf_last_subset(amd_ivf_t* sub, uint64_t out[4]);

/* ---- resident indexes joined on the device ---------------------------------------------
 * The inverse of amd_ivf_subset, and what ivflib::merge_into and SlidingIndexWindow::step  [IVFlib.cpp:77-88, 190-243] do to host
 * lists, applied to indexes that are resident in HBM: *out is an index of its own on the parts' device -- same d, nlist, metric --
 * whose list l holds, for j = 0 .. nparts - 1 in order, entries [begin_j[l], end_j[l]) of part j's list l in that part's order, their
 * ids plus id_add_j.  A merge is every part taken whole; a step of a sliding window is two parts: the window without the prefix
 * its oldest slice gave every list, then the new slice.  No list row crosses PCIe: every size is on the host, so the host makes the
 * joined offsets and per part a table of source starts and of cumulative lengths -- O(nparts * nlist) numbers, one upload -- and one
 * pass copies rows and ids device to device.  The device then holds exactly what amd_ivf_set_lists of the joined lists
 * would have made: amd_ivf_layout_digest is equal in all eight words once the same derived copies were built, byte eligibility
 * included -- it is decided over the values actually taken, so a window that drops its only non-byte row comes back byte-coded.
 * A pending amd_ivf_add of a part is applied first; no part is changed; the same handle may appear in several parts.  Centroids (with
 * norms and the fp16 range), the centroid table of amd_ivf_set_interdis, the tuner and the options are copied from part 0, as
 * amd_ivf_subset copies them from its parent; the result borrows nothing, so every part may be destroyed afterwards.
 * The result is in a subset's state: no host rows, read-only.  Everything a subset allows works on it -- every search form, clones,
 * tickets, selectors, the exact calls, range search, the scanner calls, amd_ivf_get_list, the reconstruct calls, amd_ivf_subset and
 * amd_ivf_concat of it -- and the mutating entry points return -2.
 * Returns -2 before the device is touched for: a null parts / out; nparts 0 or above 64; a part whose h is null or a clone or has
 * tickets out; parts that differ in device, d, nlist or metric; centroids that part 0 has and another part lacks or holds with other
 * bits; begin[l] > end[l] or end[l] beyond the list's size; a joined list of 2^32 entries or more.  An empty result is a valid index
 * of ntotal 0. */
typedef struct {
    amd_ivf_t* h;          /* an owner handle, or an index made by amd_ivf_subset / amd_ivf_concat; not a clone */
    const uint64_t* begin; /* nlist entries, or NULL: 0 for every list */
    const uint64_t* end;   /* nlist entries, or NULL: the list's size */
    int64_t id_add;        /* added to every id taken from this part (IndexIVF::merge_from's add_id) */
} amd_ivf_part_t;
int amd_ivf_concat(const amd_ivf_part_t* parts, size_t nparts, amd_ivf_t** out);
/* {entries taken, parts, host-to-device bytes, device-to-host bytes} of the call that made `joined` */
int amd_ivf_last_concat(amd_ivf_t* joined, uint64_t out[4]);

/* ---- search under an id selector, without a subset index -------------------------------
 * The same selectors as amd_ivf_subset (kind, a1, a2, sel, nsel: the five AMD_IVF_SUBSET_* kinds, the same membership rules, made
 * by the same pass over the resident ids), kept as ONE BIT PER STORED ENTRY instead of a second index: a selector moves no row and
 * costs an eighth of a byte per entry plus its counts; several selectors of one index are alive at once and all of them search the
 * same resident lists.  A pending amd_ivf_add of h is applied first; h itself is not changed.
 * A selector belongs to the index it was made on and to the lists as they were: it is used from that handle and from its clones;
 * amd_ivf_set_lists, amd_ivf_add, amd_ivf_update_lists and amd_ivf_remove_ids make it stale, and a search with a stale selector
 * returns -2 (it never reads old bits).  It is destroyed on its own, and before its index: amd_ivf_destroy of an index with live
 * selectors returns -2 and says how many there are; amd_ivf_selector_destroy of a selector that tickets still search under
 * (amd_ivf_submit_search_resident_selected) returns -2 and leaves it alive until they have been waited for.
 * amd_ivf_selector_create returns -2 before the device is touched for: a null h / out, h a clone, tickets out on h, an unknown
 * kind, a1 <= 0 (ID_MOD), a1 > a2 or a2 > ntotal (SLICE), sel == NULL with nsel > 0. */
typedef struct amd_ivf_selector amd_ivf_selector_t;
int amd_ivf_selector_create(amd_ivf_t* h, int kind, int64_t a1, int64_t a2, const void* sel, size_t nsel, amd_ivf_selector_t** out);
int amd_ivf_selector_destroy(amd_ivf_selector_t* s);
/* {entries looked at, entries kept, host-to-device bytes, device bytes held} */
int amd_ivf_selector_info(amd_ivf_selector_t* s, uint64_t out[4]);
/* Selectors combined on the device: *out keeps the stored entries that op says, from the keep bits of a and b as they lie in HBM --
 * one pass over a bit per entry, nothing crosses PCIe (info: {entries looked at, kept, 0, device bytes held}).  *out is a selector
 * like any other: it belongs to a's index and to the same lists, counts among the index's live selectors, works with every
 * _selected entry point and as an operand of a later combine, and is destroyed on its own -- a and b may be destroyed before it.
 * NOT keeps every STORED entry that a does not keep: the bits past a list's end stay zero whatever the op.
 * Returns -2 before the device is touched for: a null a / out, an unknown op, b == NULL for a binary op or b != NULL for NOT,
 * operands made on different indexes, a stale operand, tickets out on the index. */
#define AMD_IVF_SELECTOR_AND 0    /* a & b  */
#define AMD_IVF_SELECTOR_OR 1     /* a | b  */
#define AMD_IVF_SELECTOR_ANDNOT 2 /* a & ~b */
#define AMD_IVF_SELECTOR_NOT 3    /* ~a, b must be NULL */
int amd_ivf_selector_combine(int op, const amd_ivf_selector_t* a, const amd_ivf_selector_t* b, amd_ivf_selector_t** out);
/* amd_ivf_search / _search_preassigned / _search_resident over the members only: (D, I) are, bit for bit, what the same call
 * returns on amd_ivf_subset(h, the same selector) -- the reference's search_preassigned over the lists with the non-members removed,
 * in order; a query that finds fewer than k members ends with the reference's padding.  The coarse ranking is h's own.  In
 * amd_ivf_stats, nheap_updates is the subset's (the admissions are the same sequence); ndis counts the entries of the probed lists
 * AS h HOLDS THEM, members or not: every one of them is scanned.
 * Fixed nprobe or a radius (below), every list (amd_ivf_search_exact_selected, further down), the adaptive rule and its training
 * branch (amd_ivf_search_adaptive_selected & co, below), ids.  Not offered under a selector: the scanner calls, store_pairs /
 * max_codes, and tickets of any search but amd_ivf_search_resident_selected -- there is no entry point that takes a selector for any
 * of them, so none can return an unfiltered answer.  One selector per QUERY: the _each calls below.  -2 for a null h / s, a selector
 * of another index, a stale selector. */
int amd_ivf_search_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t n, const float* x, size_t k, size_t nprobe, int coarse_mode,
                            float* D, int64_t* I);
int amd_ivf_search_preassigned_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t n, const float* x, size_t k, size_t nprobe,
                                        const int64_t* keys, const float* coarse_dis, float* D, int64_t* I);
int amd_ivf_search_resident_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t start, size_t n, size_t k, size_t nprobe,
                                     int coarse_mode, float* D, int64_t* I);
/* The three calls above with a selector per QUERY: sels is a table of nsel selectors of h's index, sel_of[i] < nsel names the one
 * query i of the call is searched under (_resident: query start + i).  Row i of (D, I) is, bit for bit, row i of what the call above
 * of the same kind returns for the same queries under sels[sel_of[i]]; nsel == 1 gives the bits of that call.  The same selector may
 * stand in sels more than once, and a selector need not be used by any query; a query without a selector is one under a selector that
 * keeps everything.  One coarse ranking, one plan and one scan per round serve the whole batch: a list is fetched once for all the
 * queries that probe it, whichever selectors they carry (keep_rows_each_kernel).  In amd_ivf_stats nq, nlist and ndis
 * are the single-selector call's over the whole batch (ndis over h's lists), nheap_updates the sum of every query's admissions under
 * its own selector.  Synchronous; the selectors' ticket counts are not involved.
 * -2 before anything reaches the device, D and I untouched: a null h, sels, sel_of, D or I; a null x with n > 0; nsel == 0 with
 * n > 0; a null entry of sels, one of another index or a stale one (the message says which position); sel_of[i] >= nsel (the
 * message says which i); a resident range that wraps or ends behind the resident queries.  n == 0 returns 0 without a launch. */
int amd_ivf_search_selected_each(amd_ivf_t* h, const amd_ivf_selector_t* const* sels, size_t nsel, const uint32_t* sel_of, size_t n,
                                 const float* x, size_t k, size_t nprobe, int coarse_mode, float* D, int64_t* I);
int amd_ivf_search_preassigned_selected_each(amd_ivf_t* h, const amd_ivf_selector_t* const* sels, size_t nsel, const uint32_t* sel_of,
                                             size_t n, const float* x, size_t k, size_t nprobe, const int64_t* keys,
                                             const float* coarse_dis, float* D, int64_t* I);
int amd_ivf_search_resident_selected_each(amd_ivf_t* h, const amd_ivf_selector_t* const* sels, size_t nsel, const uint32_t* sel_of,
                                          size_t start, size_t n, size_t k, size_t nprobe, int coarse_mode, float* D, int64_t* I);
/* The adaptive (error-bounded) search and its training branch over the members only: amd_ivf_search_adaptive, _search_adaptive_x and
 * amd_ivf_train_samples (declared further down; every argument behind the selector is theirs) under one selector, and the resident
 * adaptive search under a selector per QUERY (sels / nsel / sel_of as in the _each calls above; sel_of[i] belongs to query
 * start + i).  D, I, my_nprobe and t_recalls -- for the training call D, I and raw -- are, bit for bit, what the unselected call of
 * the same name returns on amd_ivf_subset(h, the same selector), when h's centroid table and tuner were set before the cut; row i of
 * the _each call is what the single-selector call returns for query start + i under sels[sel_of[i]].  All arrays are indexed as the
 * unselected calls index them: by absolute query id, my_nprobe zero on entry.  The stop rule is evaluated after every probe on the
 * heap of the members; a probed list that holds no member counts as a probe, as an empty list of the subset does.  gt_D, when
 * given, is the caller's FILTERED ground truth (amd_ivf_search_exact_selected returns it): profile bit 0 measures t_recalls against
 * it, and the training call makes a tenant's raw traces from it.  The traces the rule reads are whatever the handle holds (set_tuner):
 * training them per tenant is the caller's business.
 * Option "selected_skip_empty" (default 1; read by these four calls only): a (query, list) pair whose list keeps nothing under the
 * query's selector is planned as an absent probe -- no distance row, no scan -- from the per-list kept counts the selector holds on
 * the device; 0 scans and masks such a list like any other.  The outputs are the same either way; amd_ivf_last_timing's scan bytes
 * are not.
 * Coarse tie order: these calls never patch a pass in flight (the patch moves distance rows, the masks are addressed by the rows'
 * places); under option "coarse_ties" = 2 the queries concerned are searched again, under their own selectors.
 * Not offered under a selector: the _pre forms, tickets (amd_ivf_submit_adaptive), the timed search, profile bit 1
 * (overhead_profile: -2), search contexts made by amd_ivf_clone (-2, as for every call not on their list), and the class mirror
 * under csrc/host.
 * -2 before anything reaches the device, outputs untouched: a null h, selector or table, sel_of, require_acc, my_nprobe, t_recalls, D
 * or I (the training call: gt_D, raw, D, I); a null x with n > 0; a stale selector or one of another index; nsel == 0 with n > 0, a
 * null / foreign / stale entry of sels, sel_of[i] >= nsel; profile bit 1; a resident range that wraps or ends behind the resident
 * queries. */
int amd_ivf_search_adaptive_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t start, size_t n, size_t query_topk, float multipler,
                                     float std_m, const float* require_acc, const float* gt_D, int profile, int coarse_mode,
                                     uint64_t* my_nprobe, float* t_recalls, float* D, int64_t* I);
int amd_ivf_search_adaptive_x_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t n, const float* x, size_t id_offset, size_t query_topk,
                                       float multipler, float std_m, const float* require_acc, const float* gt_D, int profile,
                                       int coarse_mode, uint64_t* my_nprobe, float* t_recalls, float* D, int64_t* I);
int amd_ivf_search_adaptive_selected_each(amd_ivf_t* h, const amd_ivf_selector_t* const* sels, size_t nsel, const uint32_t* sel_of, size_t start,
                                          size_t n, size_t query_topk, float multipler, float std_m, const float* require_acc,
                                          const float* gt_D, int profile, int coarse_mode, uint64_t* my_nprobe, float* t_recalls, float* D,
                                          int64_t* I);
int amd_ivf_train_samples_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t start, size_t n, size_t max_topk, const float* gt_D,
                                   size_t train_num, int coarse_mode, float* const* raw, float* D, int64_t* I);
/* amd_ivf_range_search / _range_search_preassigned over the members only; the results are fetched with amd_ivf_range_results.  lims,
 * labels and distances are, bit for bit and in the same order, what the same call returns on amd_ivf_subset(h, the same selector).
 * ndis as above: the probed lists' entries as h holds them.  -2 as above, before anything is read. */
int amd_ivf_range_search_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t n, const float* x, float radius, size_t nprobe,
                                  int coarse_mode, size_t* lims);
int amd_ivf_range_search_preassigned_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t n, const float* x, float radius,
                                              size_t nprobe, const int64_t* keys, size_t* lims);
/* amd_ivf_search_resident_selected in flight: a ticket for amd_ivf_wait, as amd_ivf_submit_search_resident (below).  The selector is
 * checked at submit (-2 as above, and no ticket is issued); it cannot go stale under a ticket, since every call that changes the
 * lists is refused while tickets are out, and it cannot be destroyed under one (amd_ivf_selector_destroy, above).  Owner only. */
int amd_ivf_submit_search_resident_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t start, size_t n, size_t k, size_t nprobe,
                                            int coarse_mode, float* D, int64_t* I, uint64_t* ticket);

/* ---- search ---------------------------------------------------------------------------- */

/* quantizer->search(n, x, nprobe, coarse_dis, keys)  [IndexFlat.cpp:42-56].
 * mode 0: exact per-pair kernel, same fp32 summation order as the reference's default (SSE)
 *         build of fvec_L2sqr / fvec_inner_product, i.e. knn_L2sqr_sse [utils.cpp:454-490];
 * mode 1: |x|^2+|y|^2-2x.y on the fp32 MFMA path, i.e. knn_L2sqr_blas [utils.cpp:538-608]
 *         (the reference takes it for n >= 20; its rounding belongs to the vendor BLAS);
 * mode -1: pick as the reference does (n < 20 && d % 4 == 0 -> 0, else 1)  [utils.cpp:644-655] */
int amd_ivf_coarse(amd_ivf_t* h, size_t n, const float* x, size_t nprobe, float* coarse_dis, int64_t* keys, int mode);

/* IndexIVF::search_preassigned (plain branch)  [IndexIVF.cpp:382-736; vanilla faiss/IndexIVF.cpp:250-428] */
int amd_ivf_search_preassigned(amd_ivf_t* h, size_t n, const float* x, size_t k, size_t nprobe, const int64_t* keys,
                               const float* coarse_dis, float* D, int64_t* I, int store_pairs, size_t max_codes);

/* IndexIVF::search(n, x, k, D, I): coarse + scan without leaving the device  [IndexIVF.cpp:335-353] */
int amd_ivf_search(amd_ivf_t* h, size_t n, const float* x, size_t k, size_t nprobe, int coarse_mode, float* D,
                   int64_t* I);

/* ---- exact k-NN over the whole index -----------------------------------------------------
 * (D, I) are, bit for bit, what amd_ivf_search_preassigned(h, n, x, k, nprobe = nlist, keys, ..., store_pairs = 0, max_codes = 0)
 * returns when every row of keys is 0, 1, ..., nlist - 1: the reference's search_preassigned over every list in list-number order
 * [IndexIVF.cpp:382-736], padding included (k > ntotal, an empty index).  A pending amd_ivf_add / _update_lists / _remove_ids is
 * applied first.  _resident: over resident queries [start, start + n) (amd_ivf_set_queries).  Both work on amd_ivf_clone contexts.
 * How: the reference's heap admits an entry only if it strictly beats the top, so a query whose best
 * min(k + 1, ntotal) distances are pairwise different ends with exactly the k best entries, sorted, whatever the scan order was.
 * Lists of d <= 128 are therefore searched in four stages (byte-valued lists -- the rule of every byte scan, amd_ivf_scan_arith 2 --
 * in exact integer arithmetic; float lists as described below): a seed
 * search with a fixed nprobe (option "exact_seed_nprobe") gives each query a threshold, its k-th distance; ONE pass over all lists
 * (scan_all_kernel: a list block is fetched once per 256 queries) emits each query's entries at or within its threshold; a
 * selection orders them and writes the result of every query in which no equal distances met in that window; the other queries --
 * and those without a full seed result or with more candidates than slots -- are searched the general way, as one sliced
 * amd_ivf_search_preassigned with identity keys made on the device.
 * Float lists (and byte-valued ones whose byte codes are switched off or whose queries leave the byte rule): the pass runs on the
 * fp16 copy of the lists that the filter keeps (option "filter" = 2), v_mfma_f32_32x32x16_f16 against the fp16 query rows
 * (scan_all_f16_kernel).  Such a dot product differs from the reference's distance by at most the filter's bound, so the pass emits
 * every entry that MAY lie at or within the threshold -- the comparison is not strict: an entry exactly at the threshold is never
 * lost -- each emitted entry's distance is recomputed from the fp32 rows in the reference's rounding sequence, and the selection
 * drops what lies strictly beyond the threshold before it looks for equal distances.  Option "exact_float" = 1 switches it on;
 * without it such calls go the general way whole, as they always did.
 * Beyond 128 dimensions, up to 1024, the same pass exists as a workgroup tile (scan_all_wide_f16_kernel: 128 queries x 4 list blocks,
 * the query operand through LDS); it serves a call when option "exact_wide" = 1 is set beside "exact_float" = 1 and every other
 * condition of the fp16 pass holds, and amd_ivf_last_exact_detail then reports pass 3.
 * Byte-valued lists beyond 128 dimensions, up to 1024, whose byte codes are in use have the byte pass on the same tile
 * (scan_all_wide_i8_kernel: v_mfma_i32_32x32x32_i8 on the byte fragments the byte scans keep, exact integers, no rescoring); it
 * serves a call when option "exact_wide_bytes" = 1 is set -- independent of "exact_float" and "exact_wide" -- and
 * amd_ivf_last_exact_detail then reports pass 4.  Still the general way whole: d > 1024, and such lists without
 * "exact_wide_bytes" (their general way is the int8 matrix-core scan already; with amd_ivf_set_byte_codes(h, 0), or queries
 * outside the byte rule, the call is decided as one over float lists is: the wide fp16 pass if its options ask for it).
 * A call goes the general way whole when it does not qualify: d > 128 (d > 1024, no "exact_wide" for the fp16 pass, no "exact_wide_bytes" for the byte pass), k > ntotal, k >= the candidate slots, no centroids; for the
 * fp16 pass also option "exact_float" 0, option "filter" below 2, and lists or queries of the call without a usable fp16 scale (a non-finite element,
 * magnitudes outside 2^+-24, a row that is not all zero whose largest element is below 2^-12 of the matrix's).
 * Returns -2 before the device is touched for: a null h, k = 0, null x / D / I with n > 0, a resident range that wraps round; -2 for
 * a resident range outside the resident queries.
 * amd_ivf_stats after the call: nq += n, nlist += n x nlist, ndis += n x ntotal -- every query meets every entry; nheap_updates
 * changes only by what the general-way part of the call did: the list pass does not replay the reference's heap, so it has no
 * admission count and does not invent one (the seed search leaves no trace in any of the four).
 * amd_ivf_last_exact: out[0] queries of the last exact call answered by the list pass, out[1] queries searched the general way
 * because equal distances met, out[2] queries searched the general way for any other reason (candidate overflow, no full seed
 * result, the whole call not qualifying), out[3] candidates the list pass emitted (the fp16 pass: before rescoring), summed over
 * the call.
 * amd_ivf_last_exact_detail: out[0] the list pass the last exact call ran (0 none, 1 bytes, 2 fp16 + rescoring, 3 wide fp16 + rescoring, 4 wide bytes), out[1] candidates
 * emitted, out[2] candidates at or within the threshold (the fp16 pass: after rescoring, among the stored ones; the byte pass emits
 * nothing else: out[1]; so does the wide byte pass), out[3] the largest emitted count of any one query -- what the candidate slots have to hold.
 * AUNCEL_AMD_EXACT_CAP=<n> (a test knob, read once per process): candidate slots per query, 2..4096 (default 1024).
 * Not offered: d > 128 in the pass unless option "exact_wide" (float lists up to d = 1024) or "exact_wide_bytes" (byte-coded lists up to d = 1024) asks for it, d > 1024, tickets, store_pairs / max_codes, the adaptive rule -- there is no exact entry point that takes
 * any of them.  (Selectors: below.) */
int amd_ivf_search_exact(amd_ivf_t* h, size_t n, const float* x, size_t k, float* D, int64_t* I);
int amd_ivf_search_exact_resident(amd_ivf_t* h, size_t start, size_t n, size_t k, float* D, int64_t* I);
int amd_ivf_last_exact(amd_ivf_t* h, uint64_t out[4]);
int amd_ivf_last_exact_detail(amd_ivf_t* h, uint64_t out[4]);
/* amd_ivf_search_exact / _resident over the members of a selector only: the filtered ground truth.  (D, I) are, bit for bit, what
 * amd_ivf_search_exact returns on amd_ivf_subset(h, the same selector); what amd_ivf_search_preassigned_selected returns with
 * nprobe = nlist and every row of keys 0, 1, ..., nlist - 1; the reference's search_preassigned over every list in list-number order
 * with the non-members removed -- padding included: a query with fewer than k members ends with id -1 and +-FLT_MAX.  Both work on
 * amd_ivf_clone contexts; a pending journal is applied first (a selector made before it is then stale, as everywhere).
 * How: the four stages above over "the lists with the non-members removed".  The seed searches under the selector, so
 * its k-th distance is that of k members; its nprobe is ceil("exact_seed_nprobe" x ntotal / kept), as many lists as hold the
 * members that "exact_seed_nprobe" lists hold entries.  The list pass reads a per-block mask of the slots that hold a member where it
 * read the count of slots that hold an entry: a non-member emits nothing, takes no candidate slot, and over float lists is never
 * rescored.  Equal distances count among members only.  The general way is amd_ivf_search_preassigned_selected's.
 * The call goes the general way whole when the unfiltered call would, with k > kept in place of k > ntotal, and when the scaled seed
 * reaches nlist (the seed would be the whole search); a selector without members is answered on the host with the padding.
 * Returns -2 before the device is touched for everything amd_ivf_search_exact refuses, a null s, a selector of another index and a
 * stale selector.
 * amd_ivf_stats: nq += n, nlist += n x nlist, ndis += n x ntotal of h -- the entries as h holds them, members or not, as under every
 * selector; nheap_updates by the general-way part only; the seed leaves no trace.  amd_ivf_last_exact / _detail report the call as
 * they report an unfiltered one; candidates are members only.
 * Not offered, because no entry point takes them: tickets, the adaptive rule, store_pairs / max_codes, a selector per query. */
int amd_ivf_search_exact_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t n, const float* x, size_t k, float* D, int64_t* I);
int amd_ivf_search_exact_resident_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t start, size_t n, size_t k, float* D, int64_t* I);

/* ---- exact range search over the whole index ---------------------------------------------
 * The range ground truth: lims, and the labels and distances amd_ivf_range_results then returns from the same handle, are, bit for
 * bit, what amd_ivf_range_search_preassigned(h, n, x, radius, nprobe = nlist, keys, lims) returns when every row of keys is
 * 0, 1, ..., nlist - 1: the reference's range_search_preassigned over every list -- per query the lists in list-number order and
 * the entries in position order, an entry kept iff radius > dis (L2) / radius < dis (inner product) on the reference's distance.
 * _resident: over resident queries [start, start + n).  _selected: over the selector's members only -- what
 * amd_ivf_range_search_preassigned_selected returns with those keys, and what the unselected call returns on
 * amd_ivf_subset(h, the same selector).  All forms work on amd_ivf_clone contexts; a pending journal is applied first.
 * How: the list pass of amd_ivf_search_exact, chosen by the same rule (bytes; fp16 + rescoring with "exact_float";
 * wide fp16 with "exact_wide"; wide bytes with "exact_wide_bytes") with the radius as every query's threshold.  No seed search: the radius is the threshold.  No tie
 * rule and no second pass for tied queries: the reference keeps an entry whatever it met before.  The pass emits a superset
 * (dis <= / >= threshold); exact_range_collect_kernel applies the strict test to the caller's radius, sorts a query's candidates by
 * global position -- unique, so the order is determined, and the reference's -- and exact_range_fill_kernel writes ids and
 * distances.  The byte passes are handed the radius clamped to +-2^28 (beyond every distance the byte rule allows); the test is
 * always on the radius as passed, +-inf included.  A query with more candidates than slots (AUNCEL_AMD_EXACT_CAP, above) is
 * searched the general way -- amd_ivf_range_search_preassigned(_selected) with identity keys made on the device -- and its run
 * spliced into its place; a call that qualifies for no pass (the conditions above, less the ones on k and the centroids) goes that
 * way whole.
 * Answered without a launch: n = 0 (lims[0] = 0), an empty index, a selector without members, a NaN radius (the reference's compare
 * is false for every entry): all lims 0, an empty result.
 * Returns -2 before the device is touched for: a null h, null lims, null x with n > 0, a null s, a resident range that wraps round,
 * a selector of another index, a stale selector; -2 for a resident range outside the resident queries.
 * amd_ivf_stats: nq += n, nlist += n x nlist, ndis += n x ntotal of h (members or not); nheap_updates does not move.
 * amd_ivf_last_range_exact: out[0] the list pass the last exact range call ran (0 none, 1 bytes, 2 fp16 + rescoring, 3 wide fp16 +
 * rescoring, 4 wide bytes), out[1] queries answered from the pass, out[2] queries searched the general way (candidate overflow, or the whole call
 * not qualifying), out[3] the largest emitted candidate count of any one query.  A call answered without a launch reports zeros.
 * Not offered: tickets, a radius or a selector per query, byte-coded lists beyond 128 dimensions in the pass unless option "exact_wide_bytes" asks for it, d > 1024. */
int amd_ivf_range_search_exact(amd_ivf_t* h, size_t n, const float* x, float radius, size_t* lims);
int amd_ivf_range_search_exact_resident(amd_ivf_t* h, size_t start, size_t n, float radius, size_t* lims);
int amd_ivf_range_search_exact_selected(amd_ivf_t* h, const amd_ivf_selector_t* s, size_t n, const float* x, float radius, size_t* lims);
int amd_ivf_last_range_exact(amd_ivf_t* h, uint64_t out[4]);

/* ---- stored vectors back ---------------------------------------------------------------------
 * IndexIVF::make_direct_map / reconstruct / reconstruct_n / search_and_reconstruct and IndexIVFFlat::reconstruct_from_offset
 * [IndexIVF.cpp:305-328, 869-945, IndexIVFFlat.cpp:226-230, c_api/IndexIVF_c.h:103-150] over the lists that are resident in HBM: a
 * vector is handed back by a gather over the rows amd_ivf_get_list reads -- the stored bits, whatever arithmetic the scans use, byte-
 * coded indexes included -- and found by id through a table of positions that one pass over the resident ids makes.
 * What crosses PCIe: the ids / labels sent in, a few counters, and the rows (and ids) of the answer, by one copy at the end.  Every
 * call applies a pending journal first and works on an index made by amd_ivf_subset, which keeps no host rows.
 * A position label is list << 32 | offset, what a store_pairs = 1 search returns; -1 is "no entry".  Ids may repeat: wherever a
 * vector is found by id, it is the entry at the LARGEST position (the last one the reference's list-by-list, offset-by-offset
 * loops write), whatever order the device works in.
 *
 * amd_ivf_make_direct_map(h, 1): the reference's direct_map, on the device -- table[id] = position, ntotal slots, one pass over the
 * ids, nothing but the counters comes back.  -2 with the reference's message ("direct map supported only for seuquential ids",
 * spelled as there), and no map, if any stored id lies outside [0, ntotal).  enable = 0 frees the table.  The map is a function of
 * the lists: after amd_ivf_set_lists, _add, _update_lists or _remove_ids the next call that needs it makes it again, and if the new
 * lists break the precondition that call returns -2 and the map is off.  Owner only; refused with tickets out.
 * amd_ivf_direct_map_info: {1 if a map is alive, ids mapped, ids of [0, ntotal) without an entry, passes over the ids made so far} of
 * the map as it was last made.
 * amd_ivf_reconstruct: IndexIVF::reconstruct for n ids at once, recons n x d.  -2 "direct map is not initialized" without a map; -2
 * "invalid key", with the id and its position in ids, for an id outside [0, ntotal) and for one without an entry in the map (the
 * reference reads direct_map's -1 as a position there).  Whatever is refused, recons is untouched.  Owner only.
 * amd_ivf_reconstruct_n: IndexIVF::reconstruct_n over the id window [i0, i0 + ni): slot id - i0 of recons (ni x d) gets the row of the
 * last stored entry with that id; a slot whose id is not stored is left as it was, as the reference leaves it, and found[slot] (may
 * be NULL) says which is which.  Needs no map and assumes nothing about the ids: the window may lie anywhere (the reference's
 * i0 >= 0 && i0 + ni <= ntotal is the class mirror's to enforce); its table costs 8 ni bytes of HBM.  ni = 0 returns 0 without a
 * launch; -2 before the device is touched for ni < 0 and for i0 + ni beyond the int64 range.  Works on amd_ivf_clone contexts.
 * amd_ivf_reconstruct_from_offsets: reconstruct_from_offset for n labels at once; ids (may be NULL) gets the stored ids.  A label of
 * -1 gives a row of 0xFF bytes -- the reference's memset(reconstructed, -1, ...) -- and id -1.  -2, naming the position, for a label
 * whose list is >= nlist or whose offset is at or past its list's size (every negative label but -1 is one); the outputs are then
 * untouched.  Works on amd_ivf_clone contexts.
 * amd_ivf_search_and_reconstruct / _resident: (D, I) are, bit for bit, what amd_ivf_search / amd_ivf_search_resident return for the
 * same arguments; recons (n x k x d) row (i, j) is the stored row of the ENTRY that was admitted -- its position, not "some entry
 * with id I[i, j]" -- and a row of 0xFF bytes where I is the padding's -1.  The search runs with pair labels that never leave the
 * device; one gather turns them into ids and rows.  amd_ivf_stats, amd_ivf_last_timing and the tie diagnostics move as for the plain
 * search (the wall time includes the gather).  (D, I) come back by a copy at the end; recons is written by the gather itself when
 * it is page-locked and option "direct_out" is not 0, else it is gathered in HBM and comes back by one copy.  Works on
 * amd_ivf_clone contexts and on subsets.
 * Returns -2 before the device is touched for: a null h; null ids / labels / x or a null output with n > 0; k = 0; a resident range
 * that wraps round.
 * Not offered, because no entry point takes them, so none can return a wrong row: a selector form (cut a subset and reconstruct from
 * it), the exact calls (they have no store_pairs), the adaptive rule, tickets. */
int amd_ivf_make_direct_map(amd_ivf_t* h, int enable);
int amd_ivf_direct_map_info(amd_ivf_t* h, uint64_t out[4]);
int amd_ivf_reconstruct(amd_ivf_t* h, size_t n, const int64_t* ids, float* recons);
int amd_ivf_reconstruct_n(amd_ivf_t* h, int64_t i0, int64_t ni, float* recons, uint8_t* found);
int amd_ivf_reconstruct_from_offsets(amd_ivf_t* h, size_t n, const int64_t* labels, float* recons, int64_t* ids);
int amd_ivf_search_and_reconstruct(amd_ivf_t* h, size_t n, const float* x, size_t k, size_t nprobe, int coarse_mode, float* D, int64_t* I,
                                   float* recons);
int amd_ivf_search_and_reconstruct_resident(amd_ivf_t* h, size_t start, size_t n, size_t k, size_t nprobe, int coarse_mode, float* D,
                                            int64_t* I, float* recons);

/* InvertedListScanner: set_query + set_list + scan_codes on a caller-owned raw binary heap
 * (simi/idxi, k entries, heapified by the caller as in tests/test_lowlevel_ivf.cpp:150-175);
 * returns the number of heap updates in *nup  [IndexIVFFlat.cpp:101-137] */
int amd_ivf_scan_codes(amd_ivf_t* h, const float* query, size_t list_no, int store_pairs, size_t k, float* simi,
                       int64_t* idxi, size_t* nup);
/* ... scan_codes over ANY run of codes of the list: the reference's scanner scans the n codes at whatever pointer it is handed
 * (IndexIVFFlat.cpp:117-137; tests/test_lowlevel_ivf.cpp:426-564 hands different parts of a list to different threads).  Here the
 * codes live in HBM, so the run is named: vectors [offset, offset + n) of list `list_no`.  Labels of the entries this call admits:
 * store_pairs = 0: the stored ids of those vectors; store_pairs = 1: list_no << 32 | j with j counted FROM `offset`, exactly what the
 * reference computes for a `codes` pointer that starts there (IndexIVFFlat.cpp:131).  Labels already in the heap pass through. */
int amd_ivf_scan_codes_at(amd_ivf_t* h, const float* query, size_t list_no, size_t offset, size_t n, int store_pairs, size_t k,
                          float* simi, int64_t* idxi, size_t* nup);
/* InvertedListScanner::scan_codes_range over the same kind of run  [IndexIVF.h:349-354, IndexIVFFlat.cpp:139-155]: the entries with
 * C::cmp(radius, dis) -- dis < radius (L2) / dis > radius (IP) -- in position order, as RangeQueryResult::add receives them.  *count
 * entries; amd_ivf_scan_codes_range_results copies their positions j (counted from `offset`) and distances out of the handle. */
int amd_ivf_scan_codes_range(amd_ivf_t* h, const float* query, size_t list_no, size_t offset, size_t n, float radius, size_t* count);
int amd_ivf_scan_codes_range_results(amd_ivf_t* h, uint32_t* positions, float* distances);
/* InvertedListScanner::distance_to_code for vector `offset` of list `list_no`  [IndexIVFFlat.cpp:110-115] */
int amd_ivf_distance_to_code(amd_ivf_t* h, const float* query, size_t list_no, size_t offset, float* dis);

/* IndexIVFStats {nq, nlist, ndis, nheap_updates}  [IndexIVF.h:361-374, IndexIVF.cpp:731-734] */
int amd_ivf_stats(amd_ivf_t* h, size_t stats[4], int reset);

/* amd_ivf_coarse over resident queries [start, start + n) (coarse_dis may be NULL: keys only) */
int amd_ivf_coarse_resident(amd_ivf_t* h, size_t start, size_t n, size_t nprobe, float* coarse_dis, int64_t* keys, int mode);
/* search_preassigned over resident queries [start, start + n): the caller's keys (n x nprobe, host), the engine's lists.
 * What a shard of an IndexShards runs when the coarse ranking was computed once, elsewhere. */
int amd_ivf_search_resident_preassigned(amd_ivf_t* h, size_t start, size_t n, size_t k, size_t nprobe, const int64_t* keys, float* D,
                                        int64_t* I);
/* ---- resident query sets (Error_sys::set_queries keeps the query matrix and later searches
 *      slices of it, profile.cpp:173-227): upload once, search slices with data already in HBM */
int amd_ivf_set_queries(amd_ivf_t* h, size_t n, const float* x);
int amd_ivf_search_resident(amd_ivf_t* h, size_t start, size_t n, size_t k, size_t nprobe, int coarse_mode, float* D,
                            int64_t* I);

/* ---- Auncel error-bound machinery (IVF_pro.{h,cpp}, profile.{h,cpp}) -------------------- */

/* Level1Quantizer::train_q1 table: interdis_cem[(2 nlist-1-i) i/2 + j-1-i], i<j  [IndexIVF.cpp:97-117].
 * With table == NULL it is computed on the device from the current centroids (L2: squared
 * distances; IP: reference normalisation quirk + acos); otherwise it is uploaded as given. */
int amd_ivf_set_interdis(amd_ivf_t* h, const float* table);
int amd_ivf_get_interdis(amd_ivf_t* h, float* table); /* nlist(nlist-1)/2 floats */

/* IndexIVF::init_tune + trained traces: ntraces = log2(nlist/8)+1 maps sum-of-angles -> k-scaling,
 * trace i has trace_len[i] ascending bins (x, y, std)  [IndexIVF.cpp:203-244, IVF_pro.h:47-66].
 * arcos_list: 500-entry acos LUT (error_pro::construct_arcos, IVF_pro.cpp:151-160). */
int amd_ivf_set_tuner(amd_ivf_t* h, size_t max_topk, size_t ntraces, const size_t* trace_len, const float* const* trace_x,
                      const float* const* trace_y, const float* const* trace_std, const float* arcos_list);

/* search_preassigned, tune branch, driven as Error_sys::search does (nprobe = nlist, k = max_topk)
 * on resident queries [start, start+n): per-query adaptive stop  [IndexIVF.cpp:507-638, profile.cpp:211-227].
 * require_acc / gt_D (may be NULL unless profile) / my_nprobe / t_recalls are indexed by absolute query id
 * like the reference's arrays (id_q = i + offset, IndexIVF.cpp:487); my_nprobe entries must be 0 on entry
 * for queries that have not been searched (Error_sys::set_queries zeroes them).
 * profile: bit 0 = error_pro::profile (t_recalls gets the true recall at the stop, IndexIVF.cpp:628-631);
 *          bit 1 = error_pro::overhead_profile (IndexIVF.cpp:529-539,614,634-637; eval/overhead.cpp:284-290): the rule is
 *          evaluated on every probe, its verdict ignored, every query runs to stage nlist / 8 and my_nprobe stays as
 *          passed.  The reference prints the time of the list scans alone next to it; here that is the same search without
 *          the rule, amd_ivf_search_resident(start, n, max_topk, nlist / 8) (the class mirror times both). */
int amd_ivf_search_adaptive(amd_ivf_t* h, size_t start, size_t n, size_t query_topk, float multipler, float std_m,
                            const float* require_acc, const float* gt_D, int profile, int coarse_mode,
                            uint64_t* my_nprobe, float* t_recalls, float* D, int64_t* I);

/* same, for queries passed by (host) pointer: IndexIVF::search(n, x, k, D, I, offset) with tune on
 * [IndexIVF.cpp:355-378]; arrays are indexed by id_offset + i */
int amd_ivf_search_adaptive_x(amd_ivf_t* h, size_t n, const float* x, size_t id_offset, size_t query_topk, float multipler,
                              float std_m, const float* require_acc, const float* gt_D, int profile, int coarse_mode,
                              uint64_t* my_nprobe, float* t_recalls, float* D, int64_t* I);

/* IndexIVF::search_preassigned with tune on, over the coarse ranking the CALLER passes (Auncel/IndexIVF.cpp:382-386: keys and
 * coarse_dis are arguments there; Error_sys::search gets them from its quantizer with nprobe = nlist, profile.cpp:220): rows of
 * nprobe entries per query, best first.  The probe loop has nprobe steps and set_online reads entries 0 .. nlist/8 + 20, so
 * nprobe must exceed nlist/8 + 20 (else -2).  Everything else as amd_ivf_search_adaptive_x.  This is what a subclass overriding
 * search_preassigned uses when the order of the reference's own quantizer (its BLAS, its tie order) has to be kept. */
int amd_ivf_search_adaptive_pre(amd_ivf_t* h, size_t n, const float* x, size_t id_offset, size_t nprobe, const int64_t* keys,
                                const float* coarse_dis, size_t query_topk, float multipler, float std_m, const float* require_acc,
                                const float* gt_D, int profile, uint64_t* my_nprobe, float* t_recalls, float* D, int64_t* I);

/* Time-bounded search: Error_sys::time_search (profile.cpp:229-244) = IndexIVF::search with tune off, nprobe = nlist and
 * error_pro::time_tune on: the plain probe loop (nprobe probes; time_search sets nprobe = nlist) over resident queries [start, start+n), heap of k, left when the
 * query's budget is used up.  budget_ms is indexed by absolute query id (the reference keeps the budgets in
 * t->require_acc[id_q], effect_time.cpp:274-281).  The reference tests after every probe ik whether one more is expected to
 * fit, `el >= 0.95 budget - el / (ik + 1)` (IndexIVF.cpp:545-549); the engine reads the clock between rounds and lets a
 * query take as many further probes as the same estimate says still fit (at most doubling per round).  The clock starts
 * when the call is entered (coarse quantisation included, which the reference's t0 leaves out).  Whatever the timing, the
 * result of query i is exactly search_preassigned's over its first nprobe_used[i] probes (nprobe_used may be NULL). */
int amd_ivf_search_timed(amd_ivf_t* h, size_t start, size_t n, size_t k, size_t nprobe, const float* budget_ms, int coarse_mode,
                         uint64_t* nprobe_used, float* D, int64_t* I);
/* same for queries passed by (host) pointer; budget_ms[id_offset + i] belongs to query i */
int amd_ivf_search_timed_x(amd_ivf_t* h, size_t n, const float* x, size_t id_offset, size_t k, size_t nprobe,
                           const float* budget_ms, int coarse_mode, uint64_t* nprobe_used, float* D, int64_t* I);

/* search_preassigned, training branch, driven as Error_sys::sys_train does: raw (sum_angle, kscaling)
 * samples for stages 1,2,4..nlist/8 of resident queries [start, start+n); raw[i] has
 * train_num*(max_topk/4) (x,y) pairs and must be pre-filled with (-1,-1)  [IndexIVF.cpp:640-673, profile.cpp:88-156].
 * Query start + qi reads row start + qi of gt_D (max_topk floats a row) and writes row start + qi of every raw[i] (max_topk / 4
 * pairs a row, rounded down), so the call is refused with -2, before anything reaches the device and with raw, D and I untouched,
 * when start + n > train_num or when max_topk < 4 (a row of no pairs; the reference writes behind its buffers in both cases).
 * amd_ivf_last_timing reports the call's planning passes (out[7]) and leaves the phase times of the search before it. */
int amd_ivf_train_samples(amd_ivf_t* h, size_t start, size_t n, size_t max_topk, const float* gt_D, size_t train_num,
                          int coarse_mode, float* const* raw, float* D, int64_t* I);

/* the same over n query rows of the caller's: row qi is query id_offset + qi of gt_D and of raw.  -2 as above when
 * id_offset + n > train_num or max_topk < 4. */
int amd_ivf_train_samples_x(amd_ivf_t* h, size_t n, const float* x, size_t id_offset, size_t max_topk, const float* gt_D,
                            size_t train_num, int coarse_mode, float* const* raw, float* D, int64_t* I);

/* the training branch over the caller's coarse ranking (search_preassigned with training on and its keys / coarse_dis
 * arguments, IndexIVF.cpp:382-386,640-673); nprobe > nlist/8 + 20.  -2 as above when id_offset + n > train_num or max_topk < 4. */
int amd_ivf_train_samples_pre(amd_ivf_t* h, size_t n, const float* x, size_t id_offset, size_t nprobe, const int64_t* keys,
                              const float* coarse_dis, size_t max_topk, const float* gt_D, size_t train_num, float* const* raw,
                              float* D, int64_t* I);

/* error_pro::construct_arcos: the 500-entry acos LUT, computed with the host libm exactly as the
 * reference does (LUT[i] = acosf((i-250)/250.f))  [IVF_pro.cpp:151-160] */
int amd_ivf_arcos_table(float out[500]);

/* Trace::SB: sort the raw samples by x descending, drop unset (-1,-1) ones, bucket by `bs` (250 in the
 * reference), mean x / mean y / std y per bucket, ascending on return; out_* need n/bs + 1 entries;
 * *nbuckets receives the count.  Host-side, like the reference  [IVF_pro.cpp:109-149] */
int amd_ivf_trace_sb(const float* raw_xy, size_t n, size_t bs, float* out_x, float* out_y, float* out_std,
                     size_t* nbuckets);

/* ---- sharding (IndexShards over list-id shards, IndexShards.cpp:44-105,261-311) ----------- */

/* k-way merge of nshard sorted result tables (all_D/all_I: nshard x n x k) -- host-side, as in the reference */
int amd_ivf_merge_tables(int metric, size_t n, size_t k, size_t nshard, const float* all_D, const int64_t* all_I,
                         float* D, int64_t* I);

/* ---- k-means -------------------------------------------------------------------------------------
 * Clustering::train (Clustering.cpp:75-226) over an IndexFlat of `metric`, as Level1Quantizer::train_q1 runs it
 * (IndexIVF.cpp:84-92): sub-sampling beyond k * max_points_per_centroid and seeding with the reference's rand_perm /
 * RandomGenerator (utils.cpp:111-137,229-239), niter x { assignment (coarse_mode as in amd_ivf_coarse: 0 exact kernel,
 * 1 |x|^2+|y|^2-2xy on the matrix cores, -1 the reference's switch), objective, km_update_centroids (utils.cpp:1078-1159)
 * in its fp32 summation order, void-cluster splitting }, spherical / int_centroids post-processing.  nredo 1, no input
 * centroids.  centroids: k x d out; obj: niter objective values out (may be NULL).  With coarse_mode 0 the centroids
 * equal the reference's bit for bit wherever its BLAS assignment picks the same centroids (tests/golden/kmeans_*).
 * Before anything reaches the device, returns -2 (as the reference throws) when n < k, when x (all n rows, before
 * sub-sampling) holds a NaN or an Inf ("input contains NaN's or Inf's"), or when max_points_per_centroid is 0; -2 also
 * when an assignment step yields a centroid number outside [0, k), which is then never used as an index.  When the
 * training set (after sub-sampling) has exactly k points, the centroids are the first k rows of x -- the reference's
 * corner case, even where sub-sampling chose other rows -- and obj is not written. */
int amd_ivf_kmeans(int d, size_t n, const float* x, size_t k, int metric, int niter, long seed, size_t max_points_per_centroid,
                   int spherical, int int_centroids, int coarse_mode, int device, float* centroids, float* obj);

/* ---- range search ------------------------------------------------------------------------------
 * IndexIVF::range_search / range_search_preassigned (IndexIVF.cpp:740-857) with IVFFlatScanner::scan_codes_range
 * (IndexIVFFlat.cpp:139-155): all stored vectors of the probed lists with dis < radius (L2) / dis > radius (IP), per
 * query in the reference's order (probes in order, list entries in order), unsorted.  RangeSearchResult is filled in
 * two steps as in the reference (lims first, then do_allocation): the search call writes lims (n + 1 entries), the
 * caller allocates lims[n] labels / distances and fetches them with amd_ivf_range_results from the same handle. */
int amd_ivf_range_search_preassigned(amd_ivf_t* h, size_t n, const float* x, float radius, size_t nprobe, const int64_t* keys,
                                     size_t* lims);
int amd_ivf_range_search(amd_ivf_t* h, size_t n, const float* x, float radius, size_t nprobe, int coarse_mode, size_t* lims);
int amd_ivf_range_results(amd_ivf_t* h, int64_t* labels, float* distances);

/* ---- environment ----------------------------------------------------------------------------------
 * AUNCEL_AMD_BLOCKING_SYNC=1   host threads wait for the device on blocking events (sleep until the interrupt) instead of
 *                              hipStreamSynchronize's spinning: for hosts where the calling threads outnumber their cores
 * GPU_MAX_HW_QUEUES (the HIP runtime's own variable): hardware queues per stream-priority class.  The engine's streams -- a
 *                              high-priority main stream, a background stream and a low-priority side stream per search context --
 *                              are laid out for 8 (ROCm's default is 4, with which the background streams of several searches in
 *                              flight share queues and wait for each other's kernels).  The library never changes the environment:
 *                              a process that wants more than 4 searches in flight (amd_ivf_set_async_depth, or threads of its own on
 *                              amd_ivf_clone contexts) exports GPU_MAX_HW_QUEUES=8 before anything -- torch included -- starts the HIP
 *                              runtime (bench.py and the tests do).  With fewer queues the asynchronous entry points run only as
 *                              many searches at a time as there are queues in a class and say so once on stderr (AUNCEL_AMD_QUIET)
 * Debugging knobs of the round planner's cut (plan_prefix_body defers the queries that do not fit a round to another pass over the
 * lists), each read ONCE per process, by the first search -- setting them later changes nothing (tests/test_gpu_budget_cut.py runs
 * them in child processes):
 * AUNCEL_AMD_DIST_BUDGET_MB=<n> the distance workspace of a round in MiB (2^18 floats each) instead of what the search would take;
 *                              never below the lists' vectors + 1024 x nlist + 1024 floats, so one query's rows always fit
 * AUNCEL_AMD_SEG_CAP_PAIRS=<n>  the (query, list) pairs a round may hold; only ever lowers the engine's own cap (2 Mi pairs), never
 *                              below a query's nprobe; the buffers keep the size they have without it
 * The other AUNCEL_AMD_* variables the sources read are measurement switches (DESIGN.md names the ones it quotes). */

/* ---- measurement hooks (bench.py): time of the kernels of the last search call, from HIP events
 *      recorded on the engine's own stream: {coarse_ms, scan_ms, select_ms, total_ms, scan_launches,
 *      bytes of the distances the scan tiles computed (x d x 4), fraction of the computed (query, vector)
 *      slots that were wanted pairs, planning passes of the call (= rounds planned, the last look of a search that is planned
 *      once more to find nothing left included; counted on the host, so also where the phases are not timed)} */
int amd_ivf_last_timing(amd_ivf_t* h, double out[8]);
/* the same by phase, (ms, launches) pairs: coarse ranking, dense scan (round 0), selection of dense rounds, threshold scan,
 * selection of threshold rounds, tie_fix_kernel (its own stream), round planning; then the bytes the dense and the threshold
 * rounds of the search could not avoid moving (every probed list once per round + rows / mask bits written) -- bench.py's
 * roofline.per_launch */
int amd_ivf_last_timing_detail(amd_ivf_t* h, double out[16]);
/* bytes the scans of the last search could not avoid moving through HBM: every probed list once per round (as stored:
 * d bytes per vector in byte-code mode, 4 d in fp32) plus the rows written (4 bytes per distance of a dense round, one
 * mask bit per distance in threshold mode).  A lower bound of the traffic, counted on the device by the planning kernels. */
int amd_ivf_last_scan_min_bytes(amd_ivf_t* h, double* bytes);
/* Coarse rankings longer than 128 are sorted on the device; inside a run of exactly equal distances the reference's order
 * (knn_L2sqr_sse / knn_inner_product_sse, Auncel/utils.cpp:417-490: a binary heap over centroids 0..nlist-1, heap-sorted
 * at the end, Heap.h:295-322) depends on the heap's history.  Rankings that hold such a run in the part that is read can
 * be re-run through that heap on the device (up to 2.8 ms each at nlist 4096).  Policy:
 *   calls of fewer than 20 queries (the reference's exact regime; what the eval/ harnesses issue) -- fixed-nprobe search, coarse,
 *     training: re-run.  Adaptive search: searched with such runs in centroid-number order first; a query reads only
 *     entries below 2 my_nprobe + 14, so if no run starts below that the result is the reference's, else the call is
 *     repeated with the heap's order -- same results as always re-running, at a hundredth of the cost.  Time-bounded
 *     search: centroid-number order (the clock decides the depth);
 *   larger calls: centroid-number order (the reference ranks sgemm output there);
 *   AUNCEL_AMD_COARSE_TIES=heap: always re-run; =id: never; =redo (adaptive calls of >= 20 queries): the exact-distance result
 *     for every query of the call.  The rankings whose first run starts inside what the first two rounds can read are re-run
 *     through the heap on a side stream WHILE the call's first round is planned and scanned (the planner takes whole runs into a
 *     round, so nothing before the first selection depends on the order inside a run); the heap's order is then written over
 *     those rankings and, where it changes the order of rows already scanned, over the rows (amd_ivf_last_tie_patched: rankings
 *     changed) -- one pass, the reference's order.  What that cannot cover (no slot left, a ranking read past what was re-run,
 *     nlist not a power of two: the level-parallel heap does not apply) is searched again as one small call with the heap's
 *     order (amd_ivf_last_tie_redone: how many queries that was).
 * *rows = rankings re-run so far on this handle. */
int amd_ivf_coarse_tie_rows(amd_ivf_t* h, uint64_t* rows);
int amd_ivf_last_tie_redone(amd_ivf_t* h, uint64_t* queries);
int amd_ivf_last_tie_patched(amd_ivf_t* h, uint64_t* rankings);
/* Launch sizing of the last search.  The device-planned rounds are enqueued without reading anything back, so a scan's grid is
 * sized from what the same round of the previous search of this shape needed (+ 12 %); its workgroups stride over the item
 * count the planner left on the device, so a round that needs more is still complete -- it just runs on fewer workgroups than it
 * would have been given.  out[0] = scan launches of the last search that were sized by such a hint, out[1] = those whose hint
 * was too small. */
int amd_ivf_last_round_hints(amd_ivf_t* h, uint64_t out[2]);
/* Selection diagnostics of the last search on this handle.  The k best of a query are kept as a sorted array (same
 * admissions as the reference's heap, Auncel/Heap.h:88-142); a query in which equal distances met -- the only case in which
 * the heap's history decides an id or an output order -- gets its result from the reference's heap replayed over the query's
 * admission log.  *queries = how many queries of the last search took that second path. */
int amd_ivf_last_tie_fixed(amd_ivf_t* h, uint64_t* queries);
/* fp32 lists: threshold rounds compute x.y on the matrix cores and keep a candidate iff its distance, widened by a rigorous
 * bound on the difference to the reference's value (utils_simd.cpp:391-443 rounding sequence), can beat the query's threshold;
 * the kept ones are recomputed in the reference's rounding sequence, so (D, I) stay bit-identical.  out[0] = rounds of the last
 * search on this handle that ran that way, out[1] = survivor slots the last of them handed out (>= the candidates it kept for the
 * exact recomputation: a wave takes slots 64 at a time and marks the ones it leaves unused). */
int amd_ivf_last_filter(amd_ivf_t* h, uint64_t out[2]);
/* 1 if the last search on this handle wrote (D, I) straight into the caller's buffers: when both are page-locked, device-visible
 * host memory (hipHostMalloc / hipHostRegister; torch's pin_memory) the selection kernels store each query's row there as the
 * query finishes, under the later rounds, and the call ends without a copy; pageable buffers are filled by a copy at the end.
 * AUNCEL_AMD_DIRECT_OUT=0 always copies. */
int amd_ivf_last_direct_out(amd_ivf_t* h);
/* Exact coarse rankings of a large fixed-nprobe call (>= 256 queries, nprobe <= 128 << nlist <= 4096; IndexFlat::search in the
 * arithmetic of knn_L2sqr_sse / knn_inner_product_sse, utils.cpp:417-490): the matrix cores rank every centroid approximately, the
 * centroids that can be among the nprobe best -- by a rigorous bound on the difference to the reference's value -- are recomputed
 * in the reference's rounding sequence and sorted; a query in which exactly equal distances meet (the reference's order there is
 * its heap's history) is recomputed from exact distances to every centroid through that heap.  Returned distances and ids are
 * the reference's bit for bit either way.  *rankings = how many of the last coarse call's came the first way.
 * amd_ivf_set_option(h, "coarse_pick", 0) keeps the exact distances to every centroid for all queries. */
int amd_ivf_last_coarse_pick(amd_ivf_t* h, uint64_t* rankings);

/* ------------------------------------------------------------------------------------------------
 * Asynchronous form of amd_ivf_search_adaptive (same arguments, same results).  submit returns at once with a ticket; the
 * search runs on one of `depth` internal search contexts of the handle (amd_ivf_set_async_depth, 1..16, default 4, fixed by
 * the first submit; depth 0 with no ticket out releases them: their streams and workspaces are the price of the mode; each is an amd_ivf_clone: own stream and workspaces, the owner's lists, traces and resident queries);
 * further tickets queue.  wait blocks until that search has ended and returns its status (0 / -2 / -4 as the synchronous
 * call; amd_ivf_last_error() then holds its message); timing (amd_ivf_last_timing's 8 doubles + amd_ivf_last_scan_min_bytes) and diag (launches sized by a
 * hint, hints too small, queries searched again for the tie order, 1 if (D, I) were written directly) may be null.  Every
 * buffer passed to submit must stay valid, and the index and its resident queries unchanged, until the ticket has been waited
 * for; every ticket must be waited for exactly once.  One caller thread that keeps six 5000-query searches running this way (twelve
 * tickets out: bench.py's headline) reaches what six threads with a context each reach (the reference's callers would use
 * threads: IndexShards.cpp:48-120). */
int amd_ivf_set_async_depth(amd_ivf_t* h, int depth);
int amd_ivf_submit_adaptive(amd_ivf_t* h, size_t start, size_t n, size_t query_topk, float multipler, float std_m,
                            const float* require_acc, const float* gt_D, int profile, int coarse_mode, uint64_t* my_nprobe,
                            float* t_recalls, float* D, int64_t* I, uint64_t* ticket);
/* the same for amd_ivf_search_resident (IndexIVF::search with a fixed nprobe over resident queries [start, start + n)) */
int amd_ivf_submit_search_resident(amd_ivf_t* h, size_t start, size_t n, size_t k, size_t nprobe, int coarse_mode, float* D, int64_t* I,
                                   uint64_t* ticket);
/* ... and the two halves of a sharded search (IndexShards over sub-indexes that share one quantizer, IndexShards.cpp:261-311): the
 * coarse ranking of a share of the resident queries, and search_preassigned of a resident range with keys that came from elsewhere
 * (the other shards' ranks).  `keys` / `coarse_dis` / `D` / `I` must stay valid until amd_ivf_wait returns the ticket. */
int amd_ivf_submit_coarse_resident(amd_ivf_t* h, size_t start, size_t n, size_t nprobe, float* coarse_dis, int64_t* keys, int mode,
                                   uint64_t* ticket);
int amd_ivf_submit_search_resident_preassigned(amd_ivf_t* h, size_t start, size_t n, size_t k, size_t nprobe, const int64_t* keys,
                                               float* D, int64_t* I, uint64_t* ticket);
int amd_ivf_wait(amd_ivf_t* h, uint64_t ticket, double timing[9], uint64_t diag[4]);
/* tickets the asynchronous entry points have served since the handle was made, and the passes that served them (fewer where
 * option "coalesce" joined queued tickets) */
int amd_ivf_async_counts(amd_ivf_t* h, uint64_t out[2]);

/* Arithmetic the list scan of the last search ran in.  All three produce the reference's fp32 distance bit for
 * bit (utils_simd.cpp:391-443 order); the engine picks the cheapest one the data allows:
 *   0  fp32, the reference's four running sums, separate multiply and add
 *   1  fp32 with fma: lists and queries hold integers of magnitude <= 4095
 *   2  byte codes + integer dot products: lists and queries hold integers 0..255 and d * max^2 <= 2^24
 *      (SIFT / BIGANN descriptors), lists are kept as bytes on the device (1/4 of the HBM traffic) */
int amd_ivf_scan_arith(amd_ivf_t* h);
/* enable = 0: this handle (the index owner or a search context of amd_ivf_clone) scans the fp32 lists even where the byte
 * codes qualify (same results; bench.py's fp32_path leg).  enable = 1 restores the default. */
int amd_ivf_set_byte_codes(amd_ivf_t* h, int enable);

/* Options of an index: policy that can change a result's tie order, and tuning that cannot change a result at all.  The
 * reference exposes such choices as public fields of the index (nprobe, max_codes, parallel_mode ..., IndexIVF.h:97-143) and
 * through ParameterSpace::set_index_parameter(index, "name", value) (AutoTune.h) / c_api/IndexIVF_c.h:82-85 getter-setter
 * pairs; this is the same thing in C.  `h` may be the index or one of its search contexts (the option is the index's either
 * way); set it while no search is running.  get returns the effective value: what was set, else the value of the debugging
 * environment variable of the same meaning (AUNCEL_AMD_<KEY>), else the built-in default.  Unknown key: -2.
 *
 *   key               values                                                                 default
 *   "coarse_ties"     order inside runs of bit-equal coarse distances (knn_L2sqr_sse's heap   unset (-1): heap for calls of
 *                     history, utils.cpp:454-490): 0 centroid number, 1 the reference's       fewer than 20 queries (the regime
 *                     heap for every ranking, 2 search again exactly the queries whose        in which the reference ranks exact
 *                     result could depend on it                                               distances, utils.cpp:644-655), else 0
 *                     -- the ONLY option that can change returned ids (of queries whose probe order crosses such a run)
 *   "select"          0 the reference's binary heap replayed for every query, 1 sorted        1
 *                     arrays + heap replay of the queries in which equal distances met
 *   "tie_fix"         0 that replay once at the end of a search, 1 behind every round         unset: by call size / concurrency
 *   "filter"          fp32 threshold rounds: matrix-core filter + exact recomputation of what  2
 *                     it keeps, over an fp16 (2) or fp32 (1) copy of the lists; 0 vector ALU only
 *   "fixed_rounds"    fixed-nprobe search: 1 one dense round, 2 dense + threshold round       unset (0): by nprobe
 *   "round_first", "round_grow", "round_inc"   round schedule of the adaptive search           12, 12 (bytes) / 6 / 3.5, = first
 *   "direct_out"      1 results stored straight into page-locked (D, I), 0 copied at the end  1
 *   "scan_pipelined"  byte-code scan through scan_mfma_thr_kernel (two list blocks in flight per   7
 *                     wave): bit 0 dense rounds, bit 1 threshold rounds, bit 2 threshold rounds with up to 64
 *                     queries per item (scan_mfma_pair_kernel: a chunk is fetched once per 64 queries); 0: scan_mfma_kernel
 *   "plan_fused"      round planning in 3 launches (1) or 7 (0)                               1
 *   "coarse_pick"     large fixed-nprobe calls: coarse rankings from matrix-core distances (2: fp16    2
 *                     operands, 1: fp32) + exact recomputation of the candidates (amd_ivf_last_coarse_pick),
 *                     0 exact distances to every centroid
 *   "phase_timing"    HIP events around every phase (amd_ivf_last_timing): 1 always, 0 never          unset: calls of >= 20 queries
 *   "pinned_io"       per-call inputs / outputs through one page-locked block (1) or copies (0)                 1
 *   "row_lists"       threshold rounds of calls of >= 256 queries: 1 the rows' marked candidates are compacted    unset (-1): 1 when no other
 *                     into short lists before the selection (compact_rows_kernel), 0 the selection walks the masks  search of the index is running
 *   "lanes"           dense rounds of fp32 searches: 1 from a lane-ordered copy of the lists (one coalesced KiB per    1
 *                     64 vectors and 4 dimensions, no staging; the copy costs the lists' bytes once more, built by the
 *                     first fp32 search), 0 from the rows
 *   "fp32_in_flight"  searches of >= 256 queries in fp32 arithmetic that run on the index at a time; further ones      4
 *                     wait inside the call (four is the measured optimum; 0: no limit)
 *   "coalesce"        amd_ivf_submit_adaptive: how many QUEUED tickets one pass over the lists may serve together --   1
 *                     tickets that ask for the same search (parameters, require_acc / ground-truth arrays) over resident
 *                     ranges that follow each other, with result buffers that follow each other in memory.  A pass is
 *                     bound by the list stream, not by the queries probing it, so two queued 5000-query batches cost
 *                     little more than one; every query's result is what its own call would have returned.  Only
 *                     tickets already waiting are joined: a ticket alone in the queue runs alone
 *   "incremental"     changes of the lists (amd_ivf_add, amd_ivf_update_lists, amd_ivf_remove_ids) reach the device as   1
 *                     an in-place relayout in HBM that re-encodes only the blocks they touched (1), or as a full
 *                     upload of every list (0); a journal that writes more than a quarter of the entries, or an
 *                     allocation that fails, takes the full upload either way
 *   "exact_seed_nprobe"  amd_ivf_search_exact: nprobe of the seed search whose k-th distance is the list pass's     16
 *                     threshold (at most nlist; AUNCEL_AMD_EXACT_SEED is the environment's form).  Cannot change a result
 *   "exact_float"     amd_ivf_search_exact over float lists: 1 the fp16 matrix-core list pass with rescoring, 0 the general      0
 *                     way for the whole call (AUNCEL_AMD_EXACT_FLOAT is the environment's form).  Cannot change a result
 *   "exact_wide"      ... beyond 128 dimensions (128 < d <= 1024), beside "exact_float" = 1: 1 the workgroup-tiled fp16 list     0
 *                     pass with rescoring, 0 the general way for the whole call (AUNCEL_AMD_EXACT_WIDE is the environment's
 *                     form).  Cannot change a result
 *   "exact_wide_bytes" amd_ivf_search_exact over byte-coded lists beyond 128 dimensions (128 < d <= 1024): 1 the workgroup-tiled  0
 *                     byte list pass (exact integers, no rescoring), 0 the general way for the whole call; independent of
 *                     "exact_float" / "exact_wide" (AUNCEL_AMD_EXACT_WIDE_BYTES is the environment's form).  Cannot change a
 *                     result
 *   "selected_skip_empty"  the adaptive and training calls under a selector (amd_ivf_search_adaptive_selected & co): 1 a list    1
 *                     that keeps nothing under a query's selector is planned as an absent probe, 0 it is scanned and masked
 *                     (AUNCEL_AMD_SELECTED_SKIP_EMPTY is the environment's form).  Cannot change a result
 * amd_ivf_set_option(h, key, NAN) returns the key to "unset".  May be called while search contexts of the index are searching: a
 * search reads what shapes its launches once, when it starts, so the change takes effect with the searches that start after it. */
int amd_ivf_set_option(amd_ivf_t* h, const char* key, double value);
int amd_ivf_get_option(amd_ivf_t* h, const char* key, double* value);

/* ------------------------------------------------------------------------------------------------
 * Search from and into device memory.  The `_dev` forms of amd_ivf_set_queries, amd_ivf_search,
 * amd_ivf_search_preassigned, amd_ivf_search_resident, amd_ivf_search_exact and amd_ivf_search_adaptive: the query rows, the keys and
 * the results (d_x, d_keys, d_D, d_I) are DEVICE pointers on the handle's GPU; everything else is as in the host-pointer call, and
 * the results are the host-pointer call's bit for bit.  No query row and no result byte crosses the bus.
 *   d_x      n rows of d elements, columns contiguous, row stride ldx >= d ELEMENTS; nothing between the rows is read
 *   dtype    0: fp32, 1: fp16 (widened exactly: the result is that of the fp32 call on the widened values)
 *   d_D, d_I n x k floats and int64 (n x max_topk for the adaptive call), rows contiguous; padded with -1 and +-FLT_MAX as the
 *            host-pointer calls pad
 *   stream   the caller's hipStream_t (NULL: the default stream).  The engine's stream waits for what that stream holds when the
 *            call is made -- the work that produces d_x / d_keys, the last use of d_D / d_I -- before it touches any of them; no host
 *            synchronisation is needed in front of the call.  The calls without a stream argument expect d_D / d_I to be idle.
 *            Every call returns after the engine's stream has finished: the results may then be read from any stream.
 * One small synchronisation per call is kept: the range of the query values (12 bytes, computed by the kernel that reads the rows)
 * is read back before the search's arithmetic -- exact, fused or byte codes -- is chosen, because that choice is host code.
 * require_acc, gt_D, my_nprobe and t_recalls of the adaptive call stay HOST arrays, as in amd_ivf_search_adaptive.
 * Refused with -2 before anything is launched: a null pointer, a pointer that is not device memory of the handle's device, ldx < d,
 * a dtype other than 0 or 1, a pointer misaligned for its element type -- and what the host-pointer call refuses.  n == 0 returns 0
 * and touches nothing.
 * amd_ivf_last_dev_io: the handle's last `_dev` call.  out[0] bytes of query rows that crossed host -> device (0), out[1] bytes of
 * (D, I) that crossed between device and host (0; the rows of queries searched again under option "coarse_ties" = 2 are the one
 * exception, and are counted), out[2] launches of the ingest kernels, out[3] how the caller's buffers were written: 1 the search's
 * kernels stored into them, 2 a device-to-device copy did (the exact call, whose passes select into a workspace), 0 no results. */
int amd_ivf_set_queries_dev(amd_ivf_t* h, size_t n, const void* d_x, int dtype, size_t ldx, void* stream);
int amd_ivf_search_dev(amd_ivf_t* h, size_t n, const void* d_x, int dtype, size_t ldx, size_t k, size_t nprobe, int coarse_mode, float* d_D,
                       int64_t* d_I, void* stream);
int amd_ivf_search_preassigned_dev(amd_ivf_t* h, size_t n, const void* d_x, int dtype, size_t ldx, size_t k, size_t nprobe,
                                   const int64_t* d_keys, float* d_D, int64_t* d_I, void* stream);
int amd_ivf_search_resident_dev(amd_ivf_t* h, size_t start, size_t n, size_t k, size_t nprobe, int coarse_mode, float* d_D, int64_t* d_I);
int amd_ivf_search_exact_dev(amd_ivf_t* h, size_t n, const void* d_x, int dtype, size_t ldx, size_t k, float* d_D, int64_t* d_I, void* stream);
int amd_ivf_search_adaptive_dev(amd_ivf_t* h, size_t start, size_t n, size_t query_topk, float multipler, float std_m, const float* require_acc,
                                const float* gt_D, int profile, int coarse_mode, uint64_t* my_nprobe, float* t_recalls, float* d_D,
                                int64_t* d_I);
int amd_ivf_last_dev_io(amd_ivf_t* h, uint64_t out[4]);

/* ------------------------------------------------------------------------------------------------
 * Dataset files of the reference's harness (Auncel/eval/bound.cpp:29-113; host only).  Buffers are malloc'ed
 * here and released with amd_ivf_free.  Where the harness aborts (missing file, size that is not a whole number of rows,
 * short read) these return -2 and amd_ivf_last_error() says why.
 *   read_fvecs / read_ivecs   fvecs_read / ivecs_read (:29-63): every row = int32 d followed by d 4-byte values; *x is n x d.
 *   read_fbin                 fbin_read (:65-109): int32 n, int32 d, then `num` rows (0: n rows) of d values of `bytes`
 *                             bytes each: 4 = fp32; 1 = one byte per value read as a SIGNED char and widened to float,
 *                             exactly as the harness does for its u8 SIFT files.  *n is the header's count, as there.
 *   read_ibin                 ibin_read (:111-113): the same container holding int32 (ground-truth ids). */
int amd_ivf_read_fvecs(const char* path, size_t* d, size_t* n, float** x);
int amd_ivf_read_ivecs(const char* path, size_t* d, size_t* n, int32_t** x);
int amd_ivf_read_fbin(const char* path, size_t num, int bytes, size_t* d, size_t* n, float** x);
int amd_ivf_read_ibin(const char* path, size_t num, size_t* d, size_t* n, int32_t** x);
void amd_ivf_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* AUNCEL_AMD_H */
