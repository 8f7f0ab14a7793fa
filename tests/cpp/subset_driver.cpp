// Test driver for IndexIVFFlatSubset (auncel_amd/csrc/host): an index cut on the device from the resident lists of an IndexIVFFlat by an
// IDSelectorRange and by an IDSelectorBatch, each against an IndexIVFFlat that is filled on the host with the members of every list in
// list order (IndexIVF::copy_subset_to type 0 for the range; the same loop with sel.is_member for the batch).  It runs on a bundle
// prepared by tests/test_gpu_subset_mirror.py and writes what came out to a second bundle.
// usage: subset_driver <in.tb> <out.tb>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../auncel_amd/csrc/host/AuxIndexStructures.h"
#include "../../auncel_amd/csrc/host/FaissException.h"
#include "../../auncel_amd/csrc/host/IndexFlat.h"
#include "../../auncel_amd/csrc/host/IndexIVFFlat.h"
#include "../../include/auncel_amd.h"
#include "../../oracle/tbundle.h"

using namespace faiss;
typedef Index::idx_t idx_t;

struct Setup {
    size_t d, nlist, nprobe, k;
    MetricType mt;
    const tb::Tensor *cen, *xb, *xq;
    explicit Setup(const tb::Bundle& in)
        : d(in.scalar<size_t>("d")), nlist(in.scalar<size_t>("nlist")), nprobe(in.scalar<size_t>("nprobe")), k(in.scalar<size_t>("k")),
          mt(in.scalar<int>("metric") == 0 ? METRIC_INNER_PRODUCT : METRIC_L2), cen(&in.get("centroids")), xb(&in.get("xb")),
          xq(&in.get("xq")) {}
};

static std::unique_ptr<IndexIVFFlat> make_index(const Setup& s, IndexFlat& q) {
    std::unique_ptr<IndexIVFFlat> ix(new IndexIVFFlat(&q, s.d, s.nlist, s.mt));
    ix->is_trained = true;
    ix->coarse_mode = 0;  // (the expectations come from the exact coarse path)
    ix->nprobe = s.nprobe;
    return ix;
}

static void put_search(tb::Bundle& out, const std::string& p, const Setup& s, const Index& ix) {
    const size_t nq = s.xq->dims[0];
    std::vector<float> D(nq * s.k);
    std::vector<idx_t> I(nq * s.k);
    ix.search(nq, s.xq->as<float>(), s.k, D.data(), I.data());
    out.put_f32(p + "D", {nq, s.k}, D.data());
    out.put_i64(p + "I", {nq, s.k}, I.data());
    out.put_scalar_i64(p + "ntotal", ix.ntotal);
}

// the members of every list of src, in list order, into a host index
static void fill_by_selector(const IndexIVFFlat& src, IndexIVFFlat& other, const IDSelector& sel) {
    for (size_t l = 0; l < src.nlist; l++) {
        const size_t n = src.invlists->list_size(l);
        const idx_t* ids = src.invlists->get_ids(l);
        const uint8_t* codes = src.invlists->get_codes(l);
        for (size_t i = 0; i < n; i++) {
            if (!sel.is_member(ids[i])) continue;
            other.invlists->add_entry(l, ids[i], codes + i * src.code_size);
            other.ntotal++;
        }
    }
}

template <class F> static int64_t throws(F f, const char* word = nullptr) {
    try {
        f();
    } catch (const FaissException& e) {
        return !word || strstr(e.what(), word) ? 1 : 0;
    }
    return 0;
}

struct OddSelector : IDSelector {
    bool is_member(idx_t id) const override { return id & 1; }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        tb::Bundle in = tb::Bundle::load(argv[1]), out;
        Setup s(in);
        const size_t nb = s.xb->dims[0];
        IndexFlat q(s.d, s.mt);
        q.add(s.nlist, s.cen->as<float>());
        q.coarse_mode = 0;
        auto src = make_index(s, q);
        src->add(nb, s.xb->as<float>());
        const idx_t r0 = in.scalar<int64_t>("range_lo"), r1 = in.scalar<int64_t>("range_hi");
        const tb::Tensor& bt = in.get("batch");
        std::vector<idx_t> batch(bt.as<int64_t>(), bt.as<int64_t>() + bt.numel());

        IDSelectorRange rsel(r0, r1);
        IndexIVFFlatSubset by_range(*src, rsel);
        auto host_range = make_index(s, q);
        src->copy_subset_to(*host_range, 0, r0, r1);
        put_search(out, "range_dev_", s, by_range);
        put_search(out, "range_host_", s, *host_range);

        IDSelectorBatch bsel((long)batch.size(), batch.data());
        IndexIVFFlatSubset by_batch(*src, bsel);
        auto host_batch = make_index(s, q);
        fill_by_selector(*src, *host_batch, bsel);
        put_search(out, "batch_dev_", s, by_batch);
        put_search(out, "batch_host_", s, *host_batch);

        IndexIVFFlatSubset by_type(*src, 1, 4, 2);  // (copy_subset_to type 1: id % 4 == 2)
        auto host_type = make_index(s, q);
        src->copy_subset_to(*host_type, 1, 4, 2);
        put_search(out, "mod_dev_", s, by_type);
        put_search(out, "mod_host_", s, *host_type);

        uint64_t ls[4] = {0, 0, 0, 0};
        amd_ivf_last_subset(by_range.engine(), ls);
        out.put_u64("range_last_subset", {4}, ls);
        out.put_scalar_i64("throws_add", throws([&] { by_range.add(1, s.xb->as<float>()); }));
        out.put_scalar_i64("throws_train", throws([&] { by_range.train(1, s.xb->as<float>()); }));
        out.put_scalar_i64("throws_reset", throws([&] { by_range.reset(); }));
        OddSelector odd;
        out.put_scalar_i64("throws_selector", throws([&] { IndexIVFFlatSubset x(*src, odd); }, "not implemented"));
        out.put_scalar_i64("throws_type", throws([&] { IndexIVFFlatSubset x(*src, 3, 2, 0); }, "not implemented"));
        IndexIVFFlatDedup dd(&q, s.d, s.nlist, s.mt);
        dd.is_trained = true;
        out.put_scalar_i64("throws_dedup", throws([&] { IndexIVFFlatSubset x(dd, 0, 0, 10); }, "not implemented"));
        // the source goes first: the subset still answers
        src.reset();
        put_search(out, "range_after_", s, by_range);
        out.save(argv[2]);
        printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION: %s\n", e.what());
        return 3;
    }
}
