// faiss::ivflib (Auncel/IVFlib.h), the part that works on lists resident on the device
#pragma once
#include <memory>
#include <vector>

#include "IndexIVFFlat.h"

namespace faiss {
namespace ivflib {

/// IVFlib.cpp:22-57 for the index types of this mirror: the same d and metric, both IndexIVF's, and IndexIVF's own check (d, nlist,
/// code_size, "can only merge indexes of the same type").  An IndexIVFFlatSubset stands for the IndexIVFFlat it was made from.
void check_compatible_for_merge(const Index* index0, const Index* index1);

/// ivflib::SlidingIndexWindow (IVFlib.cpp:159-243) over lists that stay on the device: a window of the last slices, where step()
/// appends a slice to every list and / or drops the oldest slice from every list's front.  The reference moves the entries inside
/// host vectors; here every step makes the next window by one join on the device (IndexIVFFlatSubset's constructor from parts: the
/// window without the prefix its oldest slice gave every list, then the new slice) and no row crosses PCIe.  The window is an
/// IndexIVFFlatSubset that step() replaces: the old one is destroyed after the new one exists, so index() is to be asked again
/// after every step.
struct SlidingIndexWindowDevice {
    int n_slice = 0;  ///< slices in the window
    size_t nlist;
    /// cumulative list sizes for each slice: sizes[list][slice] (the reference's table)
    std::vector<std::vector<size_t>> sizes;

    /// index: trained, usually empty; the window starts as its lists and takes its quantizer, nprobe and coarse_mode.  It is read
    /// here and by the compatibility check of every step.
    explicit SlidingIndexWindowDevice(const IndexIVFFlat* index);

    /// Add one index to the current window and / or remove the oldest one.  sub_index: an IndexIVFFlat or an IndexIVFFlatSubset
    /// whose lists are appended, or nullptr; it is not changed (the reference leaves its sub_index alone too).  Throws "cannot
    /// remove slice: there is none" and "nothing to do???" as the reference does.
    void step(const Index* sub_index, bool remove_oldest);

    /// the current window
    const IndexIVFFlatSubset* index() const { return cur_.get(); }
    IndexIVFFlatSubset* index() { return cur_.get(); }

   private:
    const IndexIVFFlat* first_;
    std::unique_ptr<IndexIVFFlatSubset> cur_;
};

}  // namespace ivflib
}  // namespace faiss
