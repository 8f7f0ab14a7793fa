// Test driver for IndexIVFFlat::search_selected (auncel_amd/csrc/host): the plain search of an IndexIVFFlat under an IDSelectorRange
// and an IDSelectorBatch, on the lists that are resident on the device.  It runs on a bundle prepared by
// tests/test_gpu_selector_mirror.py and writes (D, I), the list of every stored id, and how many membership passes were made after
// each call to a second bundle; the test compares the results with the CPU oracle over the filtered lists.
// usage: selector_driver <in.tb> <out.tb>
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

struct OddSelector : IDSelector {
    bool is_member(idx_t id) const override { return id & 1; }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        tb::Bundle in = tb::Bundle::load(argv[1]), out;
        const size_t d = in.scalar<size_t>("d"), nlist = in.scalar<size_t>("nlist"), nprobe = in.scalar<size_t>("nprobe"), k = in.scalar<size_t>("k");
        const MetricType mt = in.scalar<int>("metric") == 0 ? METRIC_INNER_PRODUCT : METRIC_L2;
        const tb::Tensor &cen = in.get("centroids"), &xb = in.get("xb"), &xb2 = in.get("xb2"), &xq = in.get("xq");
        const size_t nb = xb.dims[0], nb2 = xb2.dims[0], nq = xq.dims[0];
        IndexFlat q(d, mt);
        q.add(nlist, cen.as<float>());
        q.coarse_mode = 0;
        IndexIVFFlat ix(&q, d, nlist, mt);
        ix.is_trained = true;
        ix.coarse_mode = 0;  // (the expectations come from the exact coarse path)
        ix.nprobe = nprobe;
        ix.add(nb, xb.as<float>());
        const idx_t r0 = in.scalar<int64_t>("range_lo"), r1 = in.scalar<int64_t>("range_hi");
        const tb::Tensor& bt = in.get("batch");
        std::vector<idx_t> batch(bt.as<int64_t>(), bt.as<int64_t>() + bt.numel());
        IDSelectorRange rsel(r0, r1);
        IDSelectorBatch bsel((long)batch.size(), batch.data());

        std::vector<int64_t> passes;
        auto run = [&](const std::string& p, const IDSelector& sel) {
            std::vector<float> D(nq * k);
            std::vector<idx_t> I(nq * k);
            ix.search_selected(nq, xq.as<float>(), k, D.data(), I.data(), sel);
            out.put_f32(p + "D", {nq, k}, D.data());
            out.put_i64(p + "I", {nq, k}, I.data());
            uint64_t info[4];
            ix.selected_info(info);
            out.put_u64(p + "info", {4}, info);
            passes.push_back((int64_t)ix.selector_passes);
        };
        auto put_assign = [&](const std::string& name) {  // the list of every stored id (ids are 0 .. ntotal - 1, in the order added)
            std::vector<int64_t> assign((size_t)ix.ntotal, -1);
            for (size_t l = 0; l < nlist; l++) {
                const idx_t* ids = ix.invlists->get_ids(l);
                for (size_t i = 0; i < ix.invlists->list_size(l); i++) assign[(size_t)ids[i]] = (int64_t)l;
            }
            out.put_i64(name, {assign.size()}, assign.data());
        };
        put_assign("assign");
        run("range_", rsel);     // a pass
        run("range2_", rsel);    // the same selector again: none
        run("batch_", bsel);     // other parameters: a pass
        run("batch2_", bsel);    // none
        IDSelectorRange same(r0, r1);
        run("range3_", same);    // the first one's parameters in another object: a pass (the batch replaced it)
        std::vector<float> D0(nq * k);
        std::vector<idx_t> I0(nq * k);
        ix.search(nq, xq.as<float>(), k, D0.data(), I0.data());  // the plain search in between leaves the kept selector alone
        run("range4_", same);    // none
        ix.add(nb2, xb2.as<float>());
        put_assign("assign_added");
        run("added_", same);     // the lists changed: a pass
        out.put_i64("passes", {passes.size()}, passes.data());
        OddSelector odd;
        int64_t refused = 0;
        try {
            ix.search_selected(nq, xq.as<float>(), k, D0.data(), I0.data(), odd);
        } catch (const FaissException& e) {
            refused = strstr(e.what(), "not implemented") ? 1 : 0;
        }
        out.put_scalar_i64("throws_selector", refused);
        out.save(argv[2]);
        printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION: %s\n", e.what());
        return 3;
    }
}
