// faiss::IndexIVFFlat (Auncel/IndexIVFFlat.h:25-58)
#pragma once
#include <unordered_map>
#include <vector>

#include "IndexIVF.h"

struct amd_ivf_selector;

namespace faiss {

struct IndexIVFFlat : IndexIVF {
    IndexIVFFlat(Index* quantizer, size_t d, size_t nlist_, MetricType = METRIC_L2);
    IndexIVFFlat() {}

    /// precomputed_idx: list numbers from a previous assignment, entries < 0 skipped (IndexIVFFlat.cpp:41-80)
    virtual void add_core(idx_t n, const float* x, const long* xids, const long* precomputed_idx);
    void add_with_ids(idx_t n, const float* x, const long* xids) override;
    void reconstruct_from_offset(idx_t list_no, idx_t offset, float* recons) const override;  ///< IndexIVFFlat.cpp:226-230
    /// IndexIVFFlat.cpp:190-224: vectors with ids new_ids[i] (< ntotal, direct map on) replaced by x[i]: the old entry leaves its
    /// list (the list's last entry takes its place), the new one is appended to the list of its nearest centroid
    virtual void update_vectors(int nv, idx_t* new_ids, const float* x);

    /// search() over the members of `sel` only, on the lists that are resident on the device (include/auncel_amd.h:
    /// amd_ivf_search_selected): the (distances, labels) an IndexIVFFlatSubset of the same selector returns, without the second index
    /// -- the selector becomes one bit per stored entry.  An IDSelectorRange or an IDSelectorBatch; any other selector is "not
    /// implemented".  The bits are made by one pass over the resident ids and kept while the lists (invlists->version) and the
    /// selector's parameters repeat: selector_passes counts the passes made, selected_info() describes the one that is kept.
    /// Fixed nprobe, the plain search only (not tune / training / time_tune, no max_codes); not for an IndexIVFFlatDedup.
    void search_selected(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels, const IDSelector& sel) const;
    /// ... with a selector per query (amd_ivf_search_selected_each): query i is searched under *sels[sel_of[i]], sel_of[i] <
    /// sels.size(); row i is what the call above returns for query i under that selector.  One coarse ranking and one pass over the
    /// lists per round serve the whole batch.  The same preconditions.  The device selectors come from the same cache: one whose
    /// parameters and lists repeat -- from an earlier table or from a call that took it alone -- is not made again
    /// (selector_passes), and selectors of equal parameters share one.  The cache keeps up to 64 selectors of tables.
    void search_selected(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels, const std::vector<const IDSelector*>& sels,
                         const uint32_t* sel_of) const;
    mutable size_t selector_passes = 0;
    /// {entries looked at, entries kept, host-to-device bytes, device bytes held} of the kept selector (zeros: none)
    void selected_info(uint64_t out[4]) const;
    /// exact top-k over every list, on the lists that are resident on the device (include/auncel_amd.h: amd_ivf_search_exact): bit for
    /// bit search_preassigned with every row of `assign` = 0 .. nlist - 1, from one pass over the lists for all queries where the
    /// lists hold bytes (d <= 128).  The plain search only (not tune / training / time_tune, no max_codes); not for an
    /// IndexIVFFlatDedup.  exact_info: the four counts of the last call (amd_ivf_last_exact); exact_detail: which list pass it ran
    /// and its candidate counts (amd_ivf_last_exact_detail).
    void search_exact(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const;
    void exact_info(uint64_t out[4]) const;
    void exact_detail(uint64_t out[4]) const;
    /// search_exact over the members of `sel` only (include/auncel_amd.h: amd_ivf_search_exact_selected): the filtered ground truth,
    /// bit for bit search_exact of an IndexIVFFlatSubset of the same selector.  The selectors and the kept bits are search_selected's:
    /// the same selector used by both calls is made once (selector_passes); exact_info / exact_detail report the call.
    void search_exact_selected(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels, const IDSelector& sel) const;
    /// every entry within `radius`, over every list (include/auncel_amd.h: amd_ivf_range_search_exact): bit for bit
    /// range_search_preassigned with every row of keys = 0 .. nlist - 1, from one pass over the lists for all queries.  `result` is
    /// made for n queries; it is filled as range_search fills it.  _selected: over the members of `sel` only (the kept selector is
    /// search_selected's).  Not for an IndexIVFFlatDedup.  range_exact_info: the four counts of the last call (amd_ivf_last_range_exact).
    void range_search_exact(idx_t n, const float* x, float radius, RangeSearchResult* result) const;
    void range_search_exact_selected(idx_t n, const float* x, float radius, RangeSearchResult* result, const IDSelector& sel) const;
    void range_exact_info(uint64_t out[4]) const;
    /// search() from and into DEVICE memory of the engine's GPU (include/auncel_amd.h: amd_ivf_search_dev): d_x holds n contiguous
    /// fp32 rows, d_D / d_I take n x k results, all three device pointers; bit for bit what search() returns for the same rows.
    /// Ordered behind `stream` (a hipStream_t; null: the default stream) and finished on return.  The plain search only; not for
    /// an IndexIVFFlatDedup (its results are expanded on the host).
    void search_dev(idx_t n, const float* d_x, idx_t k, float* d_D, idx_t* d_I, void* stream = nullptr) const;
    IndexIVFFlat(const IndexIVFFlat&) = delete;
    IndexIVFFlat& operator=(const IndexIVFFlat&) = delete;
    ~IndexIVFFlat() override;

   private:
    /// single: the call takes one selector (the one kept for such calls is replaced when `sel` is new); else one of a table's
    amd_ivf_selector* device_selector(amd_ivf* g, const IDSelector& sel, bool single = true) const;
    struct KeptSelector {  // a device selector and what it was made from
        amd_ivf_selector* s = nullptr;
        size_t version = 0;
        int kind = -1;
        idx_t a1 = 0, a2 = 0;
        std::vector<int64_t> ids;
    };
    mutable std::vector<KeptSelector> kept_;   // every device selector that is alive: sel_, and those made for a table
    mutable amd_ivf_selector* sel_ = nullptr;  // the one kept for the calls that take one selector (selected_info)
};

/// faiss::IndexIVFFlatDedup (Auncel/IndexIVFFlat.h:62-107): equal vectors are stored once; `instances` maps the id that
/// is stored to the ids of its copies, and search results are expanded from it on the host.  update_vectors / range_search /
/// reconstruct_from_offset are "not implemented" in the reference too.
struct IndexIVFFlatDedup : IndexIVFFlat {
    std::unordered_multimap<idx_t, idx_t> instances;

    IndexIVFFlatDedup(Index* quantizer, size_t d, size_t nlist_, MetricType = METRIC_L2);
    IndexIVFFlatDedup() {}

    void train(idx_t n, const float* x) override;  ///< also dedups the training set
    void add_with_ids(idx_t n, const float* x, const long* xids) override;
    void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override;
    void search_preassigned(idx_t n, const float* x, idx_t k, const idx_t* assign, const float* centroid_dis, float* distances,
                            idx_t* labels, bool store_pairs, const IVFSearchParameters* params = nullptr) const override;
    void range_search(idx_t n, const float* x, float radius, RangeSearchResult* result) const override;
    void reconstruct_from_offset(idx_t list_no, idx_t offset, float* recons) const override;
    long remove_ids(const IDSelector& sel) override;  ///< IndexIVFFlat.cpp:381-448
    void update_vectors(int nv, idx_t* new_ids, const float* x) override;  ///< "not implemented", as the reference's

   private:
    void expand_instances(idx_t n, idx_t k, float* distances, idx_t* labels) const;
};

/// A part of an IndexIVFFlat as an index of its own, cut ON THE DEVICE from the lists that are resident there (include/auncel_amd.h:
/// amd_ivf_subset): list l holds the members of src's list l in src's order, as IndexIVF::copy_subset_to would fill a host index,
/// but no row travels.  subset_type / a1 / a2 as copy_subset_to's types 0, 1, 2; an IDSelectorRange is type 0, an IDSelectorBatch
/// goes as its ids, any other selector is "not implemented".  The quantizer, interdis_cem and the tuner's traces are taken as src's
/// engine holds them.  Read-only: add / train / reset throw.  src may be destroyed first.  An IndexIVFFlatDedup is refused (its
/// `instances` map is host state a subset would have to filter too).
struct IndexIVFFlatSubset : Index {
    size_t nlist;
    size_t nprobe;
    int coarse_mode;

    IndexIVFFlatSubset(const IndexIVFFlat& src, int subset_type, idx_t a1, idx_t a2);
    IndexIVFFlatSubset(const IndexIVFFlat& src, const IDSelector& sel);
    /// The inverse: an index JOINED on the device from lists that are resident there (include/auncel_amd.h: amd_ivf_concat).  List l
    /// holds, over the parts in order, entries [begin[l], end[l]) of each part's list l with add_id added to their ids -- every part
    /// whole is IndexIVF::merge_from without the host, two parts with runs are a step of ivflib::SlidingIndexWindowDevice (IVFlib.h).
    /// A part is an IndexIVFFlat or an IndexIVFFlatSubset; no part is changed and each may be destroyed afterwards.  The quantizer,
    /// interdis_cem, the tuner's traces, nprobe and coarse_mode are part 0's; the engine refuses parts of other shapes or centroids.
    struct Part {
        const IndexIVFFlat* flat = nullptr;  // one of the two
        const IndexIVFFlatSubset* subset = nullptr;
        std::vector<uint64_t> begin, end;  // nlist entries each, or empty: 0 / the list's size
        idx_t add_id = 0;
        Part(const IndexIVFFlat* ix, idx_t add_id_ = 0) : flat(ix), add_id(add_id_) {}
        Part(const IndexIVFFlatSubset* ix, idx_t add_id_ = 0) : subset(ix), add_id(add_id_) {}
    };
    explicit IndexIVFFlatSubset(const std::vector<Part>& parts);
    size_t list_size(size_t list_no) const;
    IndexIVFFlatSubset(const IndexIVFFlatSubset&) = delete;
    IndexIVFFlatSubset& operator=(const IndexIVFFlatSubset&) = delete;
    ~IndexIVFFlatSubset() override;

    void train(idx_t n, const float* x) override;
    void add(idx_t n, const float* x) override;
    void reset() override;
    void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override;
    void range_search(idx_t n, const float* x, float radius, RangeSearchResult* result) const override;
    /// IndexIVFFlat::search_dev over the subset's own lists
    void search_dev(idx_t n, const float* d_x, idx_t k, float* d_D, idx_t* d_I, void* stream = nullptr) const;
    /// IndexIVFFlat::search_exact / exact_info / exact_detail over the subset's own lists
    void search_exact(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const;
    void exact_info(uint64_t out[4]) const;
    void exact_detail(uint64_t out[4]) const;
    /// IndexIVFFlat::range_search_exact / range_exact_info over the subset's own lists
    void range_search_exact(idx_t n, const float* x, float radius, RangeSearchResult* result) const;
    void range_exact_info(uint64_t out[4]) const;
    /// Stored vectors back, from the subset's own lists on the device -- it keeps no host rows (include/auncel_amd.h:
    /// amd_ivf_make_direct_map ...).  make_direct_map / reconstruct as IndexIVF's: the ids must be 0 .. ntotal - 1 ("direct map
    /// supported only for seuquential ids" otherwise), reconstruct without a map is "direct map is not initialized".  reconstruct_n
    /// needs no map and keeps the reference's precondition ni == 0 || (i0 >= 0 && i0 + ni <= ntotal).  search_and_reconstruct runs
    /// with the subset's nprobe / coarse_mode: search()'s (distances, labels) and the stored row of every admitted entry, rows of
    /// 0xFF bytes behind the padding.  direct_map_info: amd_ivf_direct_map_info.
    void make_direct_map(bool new_maintain_direct_map = true);
    void reconstruct(idx_t key, float* recons) const override;
    void reconstruct_n(idx_t i0, idx_t ni, float* recons) const override;
    void search_and_reconstruct(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels, float* recons) const override;
    void direct_map_info(uint64_t out[4]) const;
    bool device_bound() const override { return true; }
    amd_ivf* engine() const { return gpu_; }

   private:
    amd_ivf* gpu_ = nullptr;
    void cut(const IndexIVFFlat& src, int subset_type, idx_t a1, idx_t a2, const void* sel, size_t nsel);
};

}  // namespace faiss
