// Test driver for the stored-vectors-back calls of IndexIVFFlatSubset (auncel_amd/csrc/host): make_direct_map + reconstruct,
// reconstruct_n and search_and_reconstruct of an index cut on the device -- it keeps no host rows -- against the same calls on a host
// IndexIVFFlat that copy_subset_to fills, whose implementations walk the host invlists as the reference's do.  It runs on a bundle
// prepared by tests/test_gpu_reconstruct_mirror.py and writes what came out to a second bundle.
// usage: reconstruct_driver <in.tb> <out.tb>
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

template <class F> static int64_t throws(F f, const char* word = nullptr) {
    try {
        f();
    } catch (const FaissException& e) {
        return !word || strstr(e.what(), word) ? 1 : 0;
    }
    return 0;
}

// the three kinds of call on one index, under the prefix p
static void put_calls(tb::Bundle& out, const std::string& p, const Index& ix, const tb::Tensor& xq, size_t k, const std::vector<idx_t>& keys,
                      idx_t i0, idx_t ni) {
    const size_t d = (size_t)ix.d, nq = xq.dims[0];
    std::vector<float> rec(keys.size() * d, -7.f);
    for (size_t i = 0; i < keys.size(); i++) ix.reconstruct(keys[i], rec.data() + i * d);
    out.put_f32(p + "rec", {keys.size(), d}, rec.data());
    std::vector<float> recn((size_t)ni * d, -7.f);
    ix.reconstruct_n(i0, ni, recn.data());
    out.put_f32(p + "recn", {(size_t)ni, d}, recn.data());
    std::vector<float> D(nq * k), R(nq * k * d);
    std::vector<idx_t> I(nq * k);
    ix.search_and_reconstruct(nq, xq.as<float>(), k, D.data(), I.data(), R.data());
    out.put_f32(p + "D", {nq, k}, D.data());
    out.put_i64(p + "I", {nq, k}, I.data());
    out.put_f32(p + "R", {nq, k, d}, R.data());
    out.put_scalar_i64(p + "ntotal", ix.ntotal);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        tb::Bundle in = tb::Bundle::load(argv[1]), out;
        const size_t d = in.scalar<size_t>("d"), nlist = in.scalar<size_t>("nlist"), nprobe = in.scalar<size_t>("nprobe"), k = in.scalar<size_t>("k");
        const MetricType mt = in.scalar<int>("metric") == 0 ? METRIC_INNER_PRODUCT : METRIC_L2;
        const tb::Tensor &cen = in.get("centroids"), &xb = in.get("xb"), &xq = in.get("xq"), &kt = in.get("keys");
        const idx_t m = in.scalar<int64_t>("slice"), i0 = in.scalar<int64_t>("i0"), ni = in.scalar<int64_t>("ni");
        const std::vector<idx_t> keys(kt.as<int64_t>(), kt.as<int64_t>() + kt.numel());
        IndexFlat q(d, mt);
        q.add(nlist, cen.as<float>());
        q.coarse_mode = 0;
        auto make_index = [&] {
            std::unique_ptr<IndexIVFFlat> ix(new IndexIVFFlat(&q, d, nlist, mt));
            ix->is_trained = true;
            ix->coarse_mode = 0;
            ix->nprobe = nprobe;
            return ix;
        };
        auto src = make_index();
        src->add(xb.dims[0], xb.as<float>());

        // copy_subset_to's type 2 takes the share [a1 / ntotal, a2 / ntotal) of every list: with (0, m = ntotal) the slice is every
        // entry, and its ids are 0 .. m - 1
        IndexIVFFlatSubset dev(*src, 2, 0, m);
        auto host = make_index();
        src->copy_subset_to(*host, 2, 0, m);
        out.put_scalar_i64("throws_nomap", throws([&] { float r[4096]; dev.reconstruct(0, r); }, "direct map is not initialized"));
        dev.make_direct_map();
        host->make_direct_map();
        put_calls(out, "dev_", dev, xq, k, keys, i0, ni);
        put_calls(out, "host_", *host, xq, k, keys, i0, ni);
        uint64_t info[4] = {0, 0, 0, 0};
        dev.direct_map_info(info);
        out.put_u64("dev_info", {4}, info);

        // reconstruct_n keeps the reference's precondition: ni == 0 || (i0 >= 0 && i0 + ni <= ntotal)
        std::vector<float> scratch((size_t)(m + 16) * d);
        out.put_scalar_i64("throws_rn_past", throws([&] { dev.reconstruct_n(m - 5, 10, scratch.data()); }));
        out.put_scalar_i64("throws_rn_negative", throws([&] { dev.reconstruct_n(-1, 2, scratch.data()); }));
        out.put_scalar_i64("throws_rn_host_past", throws([&] { host->reconstruct_n(m - 5, 10, scratch.data()); }));
        out.put_scalar_i64("ok_rn_empty", 1 - throws([&] { dev.reconstruct_n(m + 100, 0, scratch.data()); }));
        out.put_scalar_i64("ok_rn_whole", 1 - throws([&] { dev.reconstruct_n(0, m, scratch.data()); }));
        out.put_scalar_i64("throws_key", throws([&] { dev.reconstruct(m, scratch.data()); }, "invalid key"));

        // ids that are not 0 .. ntotal - 1 (id % 4 == 2): no direct map, with the reference's message; reconstruct_n has no such need
        IndexIVFFlatSubset mod(*src, 1, 4, 2);
        out.put_scalar_i64("throws_nonsequential", throws([&] { mod.make_direct_map(); }, "direct map supported only for"));
        out.put_scalar_i64("throws_nonsequential_reconstruct", throws([&] { mod.reconstruct(2, scratch.data()); }, "direct map is not initialized"));
        out.save(argv[2]);
        printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION: %s\n", e.what());
        return 3;
    }
}
