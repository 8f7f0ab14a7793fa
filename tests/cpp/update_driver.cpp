// Test driver for the in-place changes of the host-side mirror (auncel_amd/csrc/host): IndexIVFFlat::update_vectors,
// IndexIVF::merge_from and the journal that IndexIVF::sync_engine hands to the engine (amd_ivf_update_lists).  It runs the flows
// on a bundle prepared by tests/test_host_update.py and writes what came out to a second bundle, which the test compares with
// Python restatements of the reference and with the CPU oracle.
// usage: update_driver <update|merge> <in.tb> <out.tb>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

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

template <class IX> static std::unique_ptr<IX> make_index(const Setup& s, IndexFlat& q) {
    std::unique_ptr<IX> ix(new IX(&q, s.d, s.nlist, s.mt));
    ix->is_trained = true;
    ix->coarse_mode = 0;  // (the expectations come from the exact coarse path)
    ix->nprobe = s.nprobe;
    return ix;
}

static std::unique_ptr<IndexFlat> make_quantizer(const Setup& s) {
    std::unique_ptr<IndexFlat> q(new IndexFlat(s.d, s.mt));
    q->add(s.nlist, s.cen->as<float>());
    q->coarse_mode = 0;
    return q;
}

// the lists (CSR), a search of xq, and the engine's report of its last refresh of the lists
static void put_index(tb::Bundle& out, const std::string& p, const Setup& s, const IndexIVF& ix) {
    std::vector<int64_t> off(s.nlist + 1, 0), ids;
    std::vector<float> codes;
    for (size_t l = 0; l < s.nlist; l++) {
        const size_t n = ix.invlists->list_size(l);
        off[l + 1] = off[l] + (int64_t)n;
        const idx_t* li = ix.invlists->get_ids(l);
        const float* lc = reinterpret_cast<const float*>(ix.invlists->get_codes(l));
        ids.insert(ids.end(), li, li + n);
        codes.insert(codes.end(), lc, lc + n * s.d);
    }
    out.put_i64(p + "off", {s.nlist + 1}, off.data());
    out.put_i64(p + "ids", {ids.size()}, ids.data());
    out.put_f32(p + "codes", {ids.size(), s.d}, codes.data());
    out.put_scalar_i64(p + "ntotal", ix.ntotal);
    if (ix.ntotal == 0) return;
    const size_t nq = s.xq->dims[0];
    std::vector<float> D(nq * s.k);
    std::vector<idx_t> I(nq * s.k);
    ix.search(nq, s.xq->as<float>(), s.k, D.data(), I.data());
    out.put_f32(p + "D", {nq, s.k}, D.data());
    out.put_i64(p + "I", {nq, s.k}, I.data());
    uint64_t lu[4] = {0, 0, 0, 0};
    amd_ivf_last_update(ix.engine(), lu);
    out.put_u64(p + "last_update", {4}, lu);
}

template <class F> static int64_t throws(F f) {
    try {
        f();
    } catch (const FaissException&) {
        return 1;
    }
    return 0;
}

static void run_update(const tb::Bundle& in, tb::Bundle& out) {
    Setup s(in);
    const tb::Tensor &uid = in.get("upd_ids"), &ux = in.get("upd_x");
    const size_t nb = s.xb->dims[0], nu = uid.numel();
    auto q = make_quantizer(s);
    auto ix = make_index<IndexIVFFlat>(s, *q);
    ix->make_direct_map(true);
    ix->add(nb, s.xb->as<float>());
    put_index(out, "before_", s, *ix);  // (the first search sends the lists whole)
    out.put_i64("before_direct_map", {ix->direct_map.size()}, ix->direct_map.data());
    std::vector<idx_t> assign(nu);
    q->assign(nu, ux.as<float>(), assign.data());
    out.put_i64("upd_assign", {nu}, assign.data());
    std::vector<idx_t> ids(uid.as<int64_t>(), uid.as<int64_t>() + nu);
    ix->update_vectors((int)nu, ids.data(), ux.as<float>());
    put_index(out, "after_", s, *ix);
    out.put_i64("after_direct_map", {ix->direct_map.size()}, ix->direct_map.data());
    // the reference's refusals: no direct map, an id out of range, the Dedup index
    auto plain = make_index<IndexIVFFlat>(s, *q);
    plain->add(nb, s.xb->as<float>());
    idx_t one = 0, bad = (idx_t)nb + 5;
    out.put_scalar_i64("throws_no_direct_map", throws([&] { plain->update_vectors(1, &one, ux.as<float>()); }));
    out.put_scalar_i64("throws_out_of_range", throws([&] { ix->update_vectors(1, &bad, ux.as<float>()); }));
    auto dedup = make_index<IndexIVFFlatDedup>(s, *q);
    out.put_scalar_i64("throws_dedup", throws([&] { dedup->update_vectors(1, &one, ux.as<float>()); }));
}

static void run_merge(const tb::Bundle& in, tb::Bundle& out) {
    Setup s(in);
    const size_t nb = s.xb->dims[0], half = nb / 2;
    const int64_t add_id = in.scalar<int64_t>("add_id");
    auto q = make_quantizer(s);
    auto a = make_index<IndexIVFFlat>(s, *q);
    auto b = make_index<IndexIVFFlat>(s, *q);
    a->add(half, s.xb->as<float>());
    b->add(nb - half, s.xb->as<float>() + half * s.d);
    put_index(out, "a_", s, *a);
    put_index(out, "b_", s, *b);
    a->merge_from(*b, add_id);
    put_index(out, "merged_", s, *a);
    put_index(out, "other_", s, *b);
    // incompatible: another nlist, another type
    IndexFlat q2(s.d, s.mt);
    q2.add(s.nlist / 2, s.cen->as<float>());
    IndexIVFFlat c(&q2, s.d, s.nlist / 2, s.mt);
    out.put_scalar_i64("throws_nlist", throws([&] { a->merge_from(c, 0); }));
    auto dd = make_index<IndexIVFFlatDedup>(s, *q);
    out.put_scalar_i64("throws_type", throws([&] { a->merge_from(*dd, 0); }));
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    try {
        tb::Bundle in = tb::Bundle::load(argv[2]), out;
        const std::string cmd = argv[1];
        if (cmd == "update") run_update(in, out);
        else if (cmd == "merge") run_merge(in, out);
        else return 2;
        out.save(argv[3]);
        printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION: %s\n", e.what());
        return 3;
    }
}
