// Test driver for IndexIVFFlat::search_exact / exact_info and the subset index's (auncel_amd/csrc/host), run by
// tests/test_gpu_exact.py on a flat file: int64 {d, nlist, nb, nq, k}, centroids, xb (grouped by list), the list of every row (int64),
// xq.  Writes D, I, exact_info of the index, then the same of the subset of the even ids.
// usage: exact_driver <in.bin> <out.bin>
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
        std::vector<int64_t> hdr(5);
        if (!rd(f, hdr)) return 2;
        const size_t d = hdr[0], nlist = hdr[1], nb = hdr[2], nq = hdr[3], k = hdr[4];
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
        std::vector<float> D(nq * k);
        std::vector<idx_t> I(nq * k);
        uint64_t info[4];
        auto put = [&] {
            fwrite(D.data(), sizeof(float), D.size(), o);
            fwrite(I.data(), sizeof(idx_t), I.size(), o);
            fwrite(info, sizeof(uint64_t), 4, o);
        };
        ix.search_exact(nq, xq.data(), k, D.data(), I.data());
        ix.exact_info(info);
        put();
        IndexIVFFlatSubset even(ix, 1, 2, 0);  // (copy_subset_to type 1: id % 2 == 0)
        even.search_exact(nq, xq.data(), k, D.data(), I.data());
        even.exact_info(info);
        put();
        fclose(o);
        printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION: %s\n", e.what());
        return 3;
    }
}
