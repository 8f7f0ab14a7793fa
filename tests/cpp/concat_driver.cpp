// Test driver for the joins of the host-side mirror (auncel_amd/csrc/host): IndexIVFFlatSubset's constructor from parts and
// ivflib::SlidingIndexWindowDevice (IVFlib.h).  The rows of a bundle prepared by tests/test_gpu_concat_mirror.py are dealt to slice
// indexes; after every step of a scripted window the device window, an index joined from the window's slices as whole parts, and an
// IndexIVFFlat filled on the host with the slices' lists one after the other are searched, and what came out goes to a second bundle.
// usage: concat_driver <in.tb> <out.tb>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../auncel_amd/csrc/host/AuxIndexStructures.h"
#include "../../auncel_amd/csrc/host/FaissException.h"
#include "../../auncel_amd/csrc/host/IVFlib.h"
#include "../../auncel_amd/csrc/host/IndexFlat.h"
#include "../../auncel_amd/csrc/host/IndexIVFFlat.h"
#include "../../include/auncel_amd.h"
#include "../../oracle/tbundle.h"

using namespace faiss;
typedef Index::idx_t idx_t;
typedef IndexIVFFlatSubset::Part Part;

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

// list l of `other` grows by list l of src, ids shifted: InvertedLists::merge_from without emptying src
static void append_lists(const IndexIVFFlat& src, IndexIVFFlat& other, idx_t add_id) {
    for (size_t l = 0; l < src.nlist; l++) {
        const size_t n = src.invlists->list_size(l);
        const idx_t* ids = src.invlists->get_ids(l);
        const uint8_t* codes = src.invlists->get_codes(l);
        for (size_t i = 0; i < n; i++) {
            other.invlists->add_entry(l, ids[i] + add_id, codes + i * src.code_size);
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

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        tb::Bundle in = tb::Bundle::load(argv[1]), out;
        Setup s(in);
        const size_t nb = s.xb->dims[0];
        IndexFlat q(s.d, s.mt);
        q.add(s.nlist, s.cen->as<float>());
        q.coarse_mode = 0;
        // the slices: row i goes to slice slice_of[i] with id i, in row order
        const tb::Tensor& so = in.get("slice_of");
        const size_t nslice = in.scalar<size_t>("nslice");
        std::vector<std::unique_ptr<IndexIVFFlat>> slices;
        for (size_t t = 0; t < nslice; t++) {
            std::vector<float> x;
            std::vector<long> ids;
            for (size_t i = 0; i < nb; i++) {
                if ((size_t)so.as<int64_t>()[i] != t) continue;
                x.insert(x.end(), s.xb->as<float>() + i * s.d, s.xb->as<float>() + (i + 1) * s.d);
                ids.push_back((long)i);
            }
            slices.push_back(make_index(s, q));
            slices.back()->add_with_ids((idx_t)ids.size(), x.data(), ids.data());
        }

        auto first = make_index(s, q);
        ivflib::SlidingIndexWindowDevice win(first.get());
        out.put_scalar_i64("throws_none", throws([&] { win.step(nullptr, true); }, "cannot remove slice: there is none"));
        out.put_scalar_i64("throws_nothing", throws([&] { win.step(nullptr, false); }, "nothing to do???"));
        IndexFlat q2(s.d, s.mt);
        q2.add(s.nlist / 2, s.cen->as<float>());
        IndexIVFFlat other_nlist(&q2, s.d, s.nlist / 2, s.mt);
        other_nlist.is_trained = true;
        out.put_scalar_i64("throws_nlist", throws([&] { win.step(&other_nlist, false); }));
        IndexFlat q3(s.d + 4, s.mt);
        IndexIVFFlat other_d(&q3, s.d + 4, s.nlist, s.mt);
        other_d.is_trained = true;
        out.put_scalar_i64("throws_d", throws([&] { win.step(&other_d, false); }));
        IndexIVFFlatDedup dd(&q, s.d, s.nlist, s.mt);
        dd.is_trained = true;
        out.put_scalar_i64("throws_type", throws([&] { win.step(&dd, false); }, "same type"));
        out.put_scalar_i64("refused_ntotal", win.index()->ntotal);
        out.put_scalar_i64("refused_n_slice", win.n_slice);

        // five steps over the three branches: (slice to add or -1, remove the oldest)
        const int script[5][2] = {{0, 0}, {1, 0}, {2, 1}, {-1, 1}, {3, 1}};
        std::vector<size_t> held;  // the slices in the window, oldest first
        for (int step = 0; step < 5; step++) {
            const int add = script[step][0];
            const bool rm = script[step][1] != 0;
            win.step(add >= 0 ? slices[add].get() : nullptr, rm);
            if (rm) held.erase(held.begin());
            if (add >= 0) held.push_back((size_t)add);
            const std::string p = "step" + std::to_string(step) + "_";
            std::vector<Part> parts;
            auto host = make_index(s, q);
            for (size_t t : held) {
                parts.push_back(Part(slices[t].get()));
                append_lists(*slices[t], *host, 0);
            }
            IndexIVFFlatSubset joined(parts);
            put_search(out, p + "win_", s, *win.index());
            put_search(out, p + "parts_", s, joined);
            put_search(out, p + "host_", s, *host);
            out.put_scalar_i64(p + "n_slice", win.n_slice);
            // the reference's table: sizes[list][slice] = the list's entries up to and including that slice
            int64_t table_ok = 1;
            for (size_t l = 0; l < s.nlist; l++) {
                size_t run = 0;
                table_ok &= win.sizes[l].size() == held.size();
                for (size_t j = 0; j < held.size() && table_ok; j++) {
                    run += slices[held[j]]->invlists->list_size(l);
                    table_ok &= win.sizes[l][j] == run;
                }
                table_ok &= win.index()->list_size(l) == run;
            }
            out.put_scalar_i64(p + "sizes_ok", table_ok);
        }

        // a merge with shifted ids (IndexIVF::merge_from's add_id), one part of it a joined index itself, runs on the other
        {
            const idx_t shift = 100000;
            IndexIVFFlatSubset ab(std::vector<Part>{Part(slices[0].get()), Part(slices[1].get(), shift)});
            Part cut(slices[2].get(), -7);
            cut.begin.assign(s.nlist, 0);
            cut.end.resize(s.nlist);
            for (size_t l = 0; l < s.nlist; l++) {
                const size_t n = slices[2]->invlists->list_size(l);
                cut.begin[l] = n / 3;
                cut.end[l] = n - n / 4;
            }
            IndexIVFFlatSubset abc(std::vector<Part>{Part(&ab), cut});
            auto host = make_index(s, q);
            append_lists(*slices[0], *host, 0);
            append_lists(*slices[1], *host, shift);
            auto host2 = make_index(s, q);
            for (size_t l = 0; l < s.nlist; l++) {
                for (size_t i = 0; i < host->invlists->list_size(l); i++) {
                    host2->invlists->add_entry(l, host->invlists->get_ids(l)[i], host->invlists->get_codes(l) + i * host->code_size);
                    host2->ntotal++;
                }
                for (size_t i = cut.begin[l]; i < cut.end[l]; i++) {
                    host2->invlists->add_entry(l, slices[2]->invlists->get_ids(l)[i] - 7, slices[2]->invlists->get_codes(l) + i * host->code_size);
                    host2->ntotal++;
                }
            }
            put_search(out, "shift_dev_", s, ab);
            put_search(out, "shift_host_", s, *host);
            put_search(out, "runs_dev_", s, abc);
            put_search(out, "runs_host_", s, *host2);
            uint64_t lc[4] = {0, 0, 0, 0};
            amd_ivf_last_concat(abc.engine(), lc);
            out.put_u64("runs_last_concat", {4}, lc);
            out.put_scalar_i64("throws_add", throws([&] { abc.add(1, s.xb->as<float>()); }));
        }
        // the slices go first: the window still answers
        slices.clear();
        put_search(out, "after_win_", s, *win.index());
        out.save(argv[2]);
        printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION: %s\n", e.what());
        return 3;
    }
}
