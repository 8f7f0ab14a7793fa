// Test driver for the vector form of IndexIVFFlat::search_selected (auncel_amd/csrc/host): one batch under a selector per query, the
// table an IDSelectorRange, an IDSelectorBatch, a second range and the first range's parameters in another object.  It runs on a
// bundle prepared by tests/test_gpu_selector_each_mirror.py and writes the mixed call's (D, I), the (D, I) of every selector used
// alone, the list of every stored id and how many membership passes were made after each call; the test compares with the CPU oracle.
// usage: selector_each_driver <in.tb> <out.tb>
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

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        tb::Bundle in = tb::Bundle::load(argv[1]), out;
        const size_t d = in.scalar<size_t>("d"), nlist = in.scalar<size_t>("nlist"), nprobe = in.scalar<size_t>("nprobe"), k = in.scalar<size_t>("k");
        const MetricType mt = in.scalar<int>("metric") == 0 ? METRIC_INNER_PRODUCT : METRIC_L2;
        const tb::Tensor &cen = in.get("centroids"), &xb = in.get("xb"), &xq = in.get("xq"), &so = in.get("sel_of");
        const size_t nb = xb.dims[0], nq = xq.dims[0];
        IndexFlat q(d, mt);
        q.add(nlist, cen.as<float>());
        q.coarse_mode = 0;
        IndexIVFFlat ix(&q, d, nlist, mt);
        ix.is_trained = true;
        ix.coarse_mode = 0;  // (the expectations come from the exact coarse path)
        ix.nprobe = nprobe;
        ix.add(nb, xb.as<float>());
        const idx_t r0 = in.scalar<int64_t>("range_lo"), r1 = in.scalar<int64_t>("range_hi"), s0 = in.scalar<int64_t>("range2_lo"),
                    s1 = in.scalar<int64_t>("range2_hi");
        const tb::Tensor& bt = in.get("batch");
        std::vector<idx_t> batch(bt.as<int64_t>(), bt.as<int64_t>() + bt.numel());
        IDSelectorRange rsel(r0, r1), rsel2(s0, s1), again(r0, r1);
        IDSelectorBatch bsel((long)batch.size(), batch.data());
        const std::vector<const IDSelector*> table = {&rsel, &bsel, &rsel2, &again};
        std::vector<uint32_t> sel_of(nq);
        for (size_t i = 0; i < nq; i++) sel_of[i] = (uint32_t)so.as<int64_t>()[i];

        std::vector<int64_t> assign((size_t)ix.ntotal, -1);  // the list of every stored id (ids are 0 .. ntotal - 1, in the order added)
        for (size_t l = 0; l < nlist; l++) {
            const idx_t* ids = ix.invlists->get_ids(l);
            for (size_t i = 0; i < ix.invlists->list_size(l); i++) assign[(size_t)ids[i]] = (int64_t)l;
        }
        out.put_i64("assign", {assign.size()}, assign.data());

        std::vector<int64_t> passes;
        std::vector<float> D(nq * k);
        std::vector<idx_t> I(nq * k);
        auto put = [&](const std::string& p) {
            out.put_f32(p + "D", {nq, k}, D.data());
            out.put_i64(p + "I", {nq, k}, I.data());
            passes.push_back((int64_t)ix.selector_passes);
        };
        ix.search_selected(nq, xq.as<float>(), k, D.data(), I.data(), rsel);  // alone first: a pass
        put("range_");
        ix.search_selected(nq, xq.as<float>(), k, D.data(), I.data(), table, sel_of.data());  // two passes: the batch, the second range
        put("each_");
        ix.search_selected(nq, xq.as<float>(), k, D.data(), I.data(), table, sel_of.data());  // none
        put("each2_");
        ix.search_selected(nq, xq.as<float>(), k, D.data(), I.data(), bsel);  // made for the table: none
        put("batch_");
        ix.search_selected(nq, xq.as<float>(), k, D.data(), I.data(), rsel2);  // none
        put("range2_");
        ix.search(nq, xq.as<float>(), k, D.data(), I.data());  // the plain search in between leaves them alone
        ix.search_selected(nq, xq.as<float>(), k, D.data(), I.data(), table, sel_of.data());  // none
        put("each3_");
        out.put_i64("passes", {passes.size()}, passes.data());
        int64_t refused = 0;
        std::vector<uint32_t> bad = sel_of;
        bad[nq / 2] = (uint32_t)table.size();
        try {
            ix.search_selected(nq, xq.as<float>(), k, D.data(), I.data(), table, bad.data());
        } catch (const FaissException& e) {
            refused = strstr(e.what(), "sel_of[") ? 1 : 0;
        }
        out.put_scalar_i64("throws_sel_of", refused);
        out.save(argv[2]);
        printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION: %s\n", e.what());
        return 3;
    }
}
