// reconstruct_args.h as a program of its own (built with -fsanitize=address,undefined by tests/test_reconstruct_abi_cpu.py): the
// decoding of position labels against a brute-force loop over ragged lists, the id window at the ends of the int64 range, and the
// argument checks of the entry points.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../auncel_amd/csrc/reconstruct_args.h"

using namespace amdivf;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                           \
        }                                                         \
    } while (0)

int main() {
    // ---- labels against list sizes 0, 1, 31, 32, 33, 65 (twice, in two orders, so that empty lists stand first, last and between)
    const std::vector<std::vector<uint64_t>> worlds = {{0, 1, 31, 32, 33, 65}, {65, 0, 33, 0, 32, 31, 1, 0}};
    for (const auto& sizes : worlds) {
        const uint64_t nlist = sizes.size();
        std::vector<uint64_t> off(nlist + 1, 0);
        for (uint64_t l = 0; l < nlist; l++) off[l + 1] = off[l] + sizes[l];
        // brute force: every (list, offset) pair of a box around the lists, stored or not
        std::vector<int64_t> labels;
        for (uint64_t l = 0; l < nlist + 2; l++)
            for (uint64_t o = 0; o < 70; o++) {
                const int64_t label = recon_label(l, o);
                labels.push_back(label);
                CHECK(recon_label_list(label) == l && recon_label_offset(label) == o);
                uint64_t want_row = 0;
                bool stored = false;
                for (uint64_t ll = 0, row = 0; ll < nlist; ll++)
                    for (uint64_t oo = 0; oo < sizes[ll]; oo++, row++)
                        if (ll == l && oo == o) stored = true, want_row = row;
                uint64_t row = ~0ull;
                CHECK(recon_label_row(label, off.data(), nlist, &row) == stored);
                if (stored) CHECK(row == want_row);
                else CHECK(row == ~0ull);  // (nothing is written for a refused label)
            }
        uint64_t row = 0;
        // -1 and the other negative labels decode to lists that do not exist; the largest offset of a list that does
        CHECK(!recon_label_row(-1, off.data(), nlist, &row));
        CHECK(!recon_label_row(-2, off.data(), nlist, &row));
        CHECK(!recon_label_row(INT64_MIN, off.data(), nlist, &row));
        CHECK(!recon_label_row(INT64_MAX, off.data(), nlist, &row));
        CHECK(!recon_label_row(recon_label(0, 0xffffffffull), off.data(), nlist, &row));
        // first_bad_label: -1 passes, the first label outside stops it
        std::vector<int64_t> good;
        for (uint64_t l = 0; l < nlist; l++)
            for (uint64_t o = 0; o < sizes[l]; o++) good.push_back(recon_label(l, o));
        good.push_back(-1);
        CHECK(recon_first_bad_label(good.data(), good.size(), off.data(), nlist) == good.size());
        CHECK(recon_first_bad_label(good.data(), 0, off.data(), nlist) == 0);
        for (uint64_t l = 0; l < nlist; l++) {
            std::vector<int64_t> v = good;
            v[3] = recon_label(l, sizes[l]);  // offset == size
            CHECK(recon_first_bad_label(v.data(), v.size(), off.data(), nlist) == 3);
        }
        std::vector<int64_t> v = good;
        v.back() = recon_label(nlist, 0);  // list == nlist
        CHECK(recon_first_bad_label(v.data(), v.size(), off.data(), nlist) == v.size() - 1);
        v.back() = -2;
        CHECK(recon_first_bad_label(v.data(), v.size(), off.data(), nlist) == v.size() - 1);
    }

    // ---- the id window at the ends of the int64 range
    CHECK(recon_window_error(0, 0).empty());
    CHECK(recon_window_error(0, INT64_MAX).empty());
    CHECK(recon_window_error(INT64_MIN, INT64_MAX).empty());
    CHECK(recon_window_error(INT64_MIN, 0).empty());
    CHECK(recon_window_error(1, INT64_MAX - 1).empty());
    CHECK(recon_window_error(INT64_MAX, 0).empty());
    CHECK(recon_window_error(1, INT64_MAX).find("overflows") != std::string::npos);
    CHECK(recon_window_error(INT64_MAX, 1).find("overflows") != std::string::npos);
    CHECK(recon_window_error(INT64_MAX, INT64_MAX).find("overflows") != std::string::npos);
    CHECK(recon_window_error(0, -1).find("negative") != std::string::npos);
    CHECK(recon_window_error(5, INT64_MIN).find("negative") != std::string::npos);
    struct W {
        int64_t lo;
        uint64_t n;
    };
    const W windows[] = {{0, 10}, {-5, 10}, {INT64_MIN, 3}, {INT64_MAX - 3, 3}, {INT64_MIN, (uint64_t)INT64_MAX}, {-1, (uint64_t)INT64_MAX},
                         {1000000000000ll, 4}, {7, 0}};
    const int64_t probes[] = {INT64_MIN, INT64_MIN + 1, INT64_MIN + 2, INT64_MIN + 3, -6, -5, -1, 0, 4, 5, 9, 10, 999999999999ll,
                              1000000000000ll, 1000000000003ll, 1000000000004ll, INT64_MAX - 4, INT64_MAX - 3, INT64_MAX - 1, INT64_MAX};
    for (const W& w : windows)
        for (int64_t id : probes) {
            uint64_t slot = 0;
            const bool in = recon_in_window(id, w.lo, w.n, &slot);
            // the same in 128-bit integers
            const __int128 rel = (__int128)id - (__int128)w.lo;
            const bool want = rel >= 0 && rel < (__int128)w.n;
            CHECK(in == want);
            if (want) CHECK(slot == (uint64_t)rel);
        }

    // ---- argument checks
    int dummy = 0;
    const void* p = &dummy;
    CHECK(recon_n_args_error(false, 0, 1, p).find("null handle") != std::string::npos);
    CHECK(recon_n_args_error(true, 0, 1, nullptr).find("null argument") != std::string::npos);
    CHECK(recon_n_args_error(true, 0, 0, nullptr).empty());
    CHECK(recon_n_args_error(true, 0, -3, p).find("negative") != std::string::npos);
    CHECK(recon_n_args_error(true, INT64_MAX - 1, 2, p).find("overflows") != std::string::npos);
    CHECK(recon_n_args_error(true, -7, 20, p).empty());
    CHECK(recon_keys_args_error("reconstruct", false, 1, p, p).find("reconstruct: null handle") != std::string::npos);
    CHECK(recon_keys_args_error("reconstruct", true, 1, nullptr, p).find("null argument") != std::string::npos);
    CHECK(recon_keys_args_error("reconstruct", true, 1, p, nullptr).find("null argument") != std::string::npos);
    CHECK(recon_keys_args_error("reconstruct", true, 0, nullptr, nullptr).empty());
    CHECK(recon_keys_args_error("reconstruct_from_offsets", true, 2, p, p).empty());
    CHECK(recon_search_args_error(false, true, 0, 1, 1, p, p, p).find("null handle") != std::string::npos);
    CHECK(recon_search_args_error(true, true, 0, 1, 0, p, p, p).find("k must be positive") != std::string::npos);
    CHECK(recon_search_args_error(true, false, 0, 1, 1, p, p, p).find("null argument") != std::string::npos);
    CHECK(recon_search_args_error(true, true, 0, 1, 1, nullptr, p, p).find("null argument") != std::string::npos);
    CHECK(recon_search_args_error(true, true, 0, 1, 1, p, nullptr, p).find("null argument") != std::string::npos);
    CHECK(recon_search_args_error(true, true, 0, 1, 1, p, p, nullptr).find("null argument") != std::string::npos);
    CHECK(recon_search_args_error(true, true, ~(size_t)0, 2, 1, p, p, p).find("range") != std::string::npos);
    CHECK(recon_search_args_error(true, false, 0, 0, 1, nullptr, nullptr, nullptr).empty());
    CHECK(recon_search_args_error(true, true, 5, 7, 3, p, p, p).empty());
    const int64_t ids[] = {0, 4, 2, 5, -1};
    CHECK(recon_first_bad_id(ids, 3, 5) == 3);
    CHECK(recon_first_bad_id(ids, 5, 5) == 3);
    CHECK(recon_first_bad_id(ids, 5, 6) == 4);
    CHECK(recon_first_bad_id(ids, 0, 0) == 0);
    CHECK(recon_first_bad_id(ids, 1, 0) == 0);

    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("DONE\n");
    return 0;
}
