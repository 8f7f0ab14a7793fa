// Test driver for IndexIVFFlat::range_search_exact / range_search_exact_selected / range_exact_info and the subset index's
// (auncel_amd/csrc/host), run by tests/test_gpu_exact_range.py on a flat file: int64 {d, nlist, nb, nq, a1, a2}, float radius,
// centroids, xb (grouped by list), the list of every row (int64), xq.  Writes, three times, {lims (nq + 1, uint64), labels, distances,
// range_exact_info}: of the index, of the index under IDSelectorRange(a1, a2), of the subset of the even ids.
// usage: exact_range_driver <in.bin> <out.bin>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "AuxIndexStructures.h"
#include "IndexFlat.h"
#include "IndexIVFFlat.h"

using namespace faiss;
typedef Index::idx_t idx_t;

template <class T> static bool rd(FILE* f, std::vector<T>& v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        std::vector<int64_t> hdr(6);
        std::vector<float> rad(1);
        if (!rd(f, hdr) || !rd(f, rad)) return 2;
        const size_t d = hdr[0], nlist = hdr[1], nb = hdr[2], nq = hdr[3];
        std::vector<float> cen(nlist * d), xb(nb * d), xq(nq * d);
        std::vector<int64_t> assign(nb);
        if (!rd(f, cen) || !rd(f, xb) || !rd(f, assign) || !rd(f, xq)) return 2;
        fclose(f);
        IndexFlat q(d, METRIC_L2);
        q.add(nlist, cen.data());
        IndexIVFFlat ix(&q, d, nlist, METRIC_L2);
        ix.is_trained = true;
        std::vector<long> lists(assign.begin(), assign.end());
        ix.add_core(nb, xb.data(), nullptr, lists.data());  // ids 0 .. nb - 1, each row in its list
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        uint64_t info[4];
        auto put = [&](const RangeSearchResult& r) {
            std::vector<uint64_t> lims(r.lims, r.lims + nq + 1);
            fwrite(lims.data(), sizeof(uint64_t), lims.size(), o);
            fwrite(r.labels, sizeof(idx_t), r.lims[nq], o);
            fwrite(r.distances, sizeof(float), r.lims[nq], o);
            fwrite(info, sizeof(uint64_t), 4, o);
        };
        {
            RangeSearchResult r(nq);
            ix.range_search_exact(nq, xq.data(), rad[0], &r);
            ix.range_exact_info(info);
            put(r);
        }
        {
            RangeSearchResult r(nq);
            IDSelectorRange sel(hdr[4], hdr[5]);
            ix.range_search_exact_selected(nq, xq.data(), rad[0], &r, sel);
            ix.range_exact_info(info);
            put(r);
        }
        {
            RangeSearchResult r(nq);
            IndexIVFFlatSubset even(ix, 1, 2, 0);  // (copy_subset_to type 1: id % 2 == 0)
            even.range_search_exact(nq, xq.data(), rad[0], &r);
            even.range_exact_info(info);
            put(r);
        }
        fclose(o);
        printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION: %s\n", e.what());
        return 3;
    }
}
