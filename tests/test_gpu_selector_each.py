"""One batch searched under a selector per query (amd_ivf_search_selected_each and its preassigned / resident siblings,
keep_rows_each_kernel in ivf_selector.hip).  The expected value of row i is row i of the pinned CPU oracle's search_preassigned over
the lists with the non-members of selector sel_of[i] removed -- test_gpu_selector.py's `expected`, assembled row by row; it never
comes from the code under test.  I is compared for equality, D by bits, statistics as integers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_selector import CONFIGS, case, configure, expected, same
from test_gpu_subset import filtered, oracle_lists, selector
from test_gpu_update import K, NPROBE, NQ, Model, bits, handle, make_case

pytestmark = pytest.mark.gpu

SELS = ["range_third", "mod_3_1", "bits_half", "bits_1pct", "bits_none", "bits_all", "bits_lists"]
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "selector_each_child.py")
FATAL = (-6, -11, 134, 139)


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def mixed(n, nsel=len(SELS), seed=29):
    """neighbouring queries under different selectors"""
    return np.random.RandomState(seed).randint(0, nsel, size=n).astype(np.uint32)


def runs(n, nsel=len(SELS), seed=31):
    """long runs of one selector, in a shuffled order of the selectors"""
    order = np.random.RandomState(seed).permutation(nsel)
    return np.repeat(order, (n + nsel - 1) // nsel)[:n].astype(np.uint32)


def rows(oracle, name, capi, sel_of, names=SELS):
    """(eD, eI): row i from the oracle over the lists filtered by selector sel_of[i]"""
    per = [expected(oracle, name, s, capi) for s in names]
    eD = np.stack([per[j][4][i] for i, j in enumerate(sel_of)])
    eI = np.stack([per[j][5][i] for i, j in enumerate(sel_of)])
    return eD, eI


_heap = {}


def heap_updates(oracle, name, capi, sel_of, names=SELS):
    """the oracle's nheap_updates of the batch: per selector, its search_preassigned over that selector's lists for the queries that
    carry it (a query's admissions are its own selector's sequence), summed"""
    metric, cen, assign, xb, xq, model = case(name)
    total = 0
    for j, s in enumerate(names):
        g = np.nonzero(np.asarray(sel_of) == j)[0]
        if len(g) == 0:
            continue
        key = (name, s, g.tobytes())
        if key not in _heap:
            args, want, cd, ck, eD, eI, est = expected(oracle, name, s, capi)
            gD, gI, gst = oracle.search_preassigned(oracle_lists(oracle, metric, cen, want), xq[g], K, ck[g], cd[g])
            assert np.array_equal(gI, eI[g]) and np.array_equal(bits(gD), bits(eD[g]))  # (a query's result does not depend on its batch)
            _heap[key] = gst[2]
        total += _heap[key]
    return total


def parent_ndis(oracle, name, capi):
    metric, cen, assign, xb, xq, model = case(name)
    _, _, cd, ck, _, _, _ = expected(oracle, name, SELS[0], capi)
    return oracle.search_preassigned(oracle_lists(oracle, metric, cen, model), xq, K, ck, cd)[2][1]


def make_selectors(capi, h, model, names=SELS):
    return [h.selector(*selector(capi, s, model)[0]) for s in names]


def close_all(sels):
    for s in sels:
        s.close()


@pytest.mark.parametrize("name", ["sift_l2", "l2_96", "ip_96", "odd_30", "bytes_960"])
def test_mixed_batches_equal_the_oracle(capi, oracle, name):
    """test 1: all three entry points, the four (byte codes, filter) configurations, a draw whose neighbours differ and one with long
    runs; nheap_updates is the sum of the queries' own selectors' admissions, ndis the parent's"""
    metric, cen, assign, xb, xq, model = case(name)
    _, _, cd, ck, _, _, _ = expected(oracle, name, SELS[0], capi)
    ndis = parent_ndis(oracle, name, capi)
    h = handle(capi, metric, cen, xb, assign, 1)
    h.set_queries(xq)
    sels = make_selectors(capi, h, model)
    for what, sel_of in (("mixed", mixed(NQ)), ("runs", runs(NQ))):
        assert len(set(sel_of.tolist())) == len(SELS)
        if what == "mixed":
            assert (sel_of[1:] != sel_of[:-1]).mean() > 0.5
        eD, eI = rows(oracle, name, capi, sel_of)
        heap = heap_updates(oracle, name, capi, sel_of)
        for byte, filt in CONFIGS:
            configure(h, byte, filt)
            for entry, call in (("preassigned", lambda: h.search_preassigned_selected_each(sels, sel_of, xq, K, ck, cd)),
                                ("search", lambda: h.search_selected_each(sels, sel_of, xq, K, NPROBE)),
                                ("resident", lambda: h.search_resident_selected_each(sels, sel_of, 0, NQ, K, NPROBE))):
                h.stats(reset=True)
                got = call()
                st = h.stats()
                same(got, eD, eI, (what, byte, filt, entry))
                assert st["nheap_updates"] == heap and st["ndis"] == ndis and st["nq"] == NQ, (what, byte, filt, entry, st, heap, ndis)
            # a slice of the resident queries: query start + i is searched under sel_of[i]
            got = h.search_resident_selected_each(sels, sel_of[40:140], 40, 100, K, NPROBE)
            same(got, eD[40:140], eI[40:140], (what, byte, filt, "resident slice"))
    close_all(sels)
    h.close()


@pytest.mark.parametrize("select", [1, 0])
@pytest.mark.parametrize("row_lists", [0, 1])
@pytest.mark.parametrize("name", ["sift_l2", "l2_96", "ip_96"])
def test_threshold_rounds_carry_each_querys_bits(capi, oracle, name, row_lists, select):
    """test 2: fixed_rounds 2 -- a dense round (the keep words are written), then a threshold round (they are ANDed into the scan's
    marks; on the float cases between the filter and the rescoring)"""
    metric, cen, assign, xb, xq, model = case(name)
    _, _, cd, ck, _, _, _ = expected(oracle, name, SELS[0], capi)
    h = handle(capi, metric, cen, xb, assign, 1)
    h.set_option("fixed_rounds", 2)
    h.set_option("row_lists", row_lists)
    h.set_option("select", select)
    sels = make_selectors(capi, h, model)
    for sel_of in (mixed(NQ), runs(NQ)):
        eD, eI = rows(oracle, name, capi, sel_of)
        h.stats(reset=True)
        same(h.search_preassigned_selected_each(sels, sel_of, xq, K, ck, cd), eD, eI)
        assert h.stats()["nheap_updates"] == heap_updates(oracle, name, capi, sel_of)
        thr_bytes = h.last_timing_detail()["min_bytes_thr"]
        print(name, "row_lists", row_lists, "select", select, "min_bytes_thr", thr_bytes, "filter", h.last_filter())
        assert thr_bytes > 0, "no threshold round ran"
        if name == "sift_l2":
            assert h.scan_arith() == 2
        else:
            assert h.last_filter()[0] >= 1, "the threshold round did not go through the filter"
        same(h.search_selected_each(sels, sel_of, xq, K, NPROBE), eD, eI)
    close_all(sels)
    h.close()


@pytest.mark.parametrize("fixed_rounds", [None, 2])
@pytest.mark.parametrize("name", ["sift_l2", "odd_30", "bytes_960"])
def test_small_calls(capi, oracle, name, fixed_rounds):
    """test 3: calls of 1, 19, 32 and 33 queries (plan_one_kernel, plan_small_kernel, the coarse ranking of fewer than 20 queries);
    sel_of is not constant inside a call, and a call's first query is not the table's first selector"""
    metric, cen, assign, xb, xq, model = case(name)
    _, _, cd, ck, _, _, _ = expected(oracle, name, SELS[0], capi)
    h = handle(capi, metric, cen, xb, assign, 1)
    h.set_option("fixed_rounds", fixed_rounds)
    sels = make_selectors(capi, h, model)
    sel_of = mixed(NQ)
    eD, eI = rows(oracle, name, capi, sel_of)
    for byte in (1, 0):
        h.set_byte_codes(byte)
        for n0, n in ((0, 1), (7, 1), (40, 19), (100, 32), (3, 33)):
            q = slice(n0, n0 + n)
            assert n == 1 or len(set(sel_of[q].tolist())) > 1
            same(h.search_preassigned_selected_each(sels, sel_of[q], xq[q], K, ck[q], cd[q]), eD[q], eI[q], (byte, n0, n))
            same(h.search_selected_each(sels, sel_of[q], xq[q], K, NPROBE), eD[q], eI[q], (byte, n0, n))
    close_all(sels)
    h.close()


def run_child(name, tmp, tag, env_extra, sel_of):
    d = tmp / tag
    d.mkdir()
    np.save(str(d / "sel_of.npy"), sel_of)
    out = str(d / "out.npz")
    env = dict(os.environ)
    env.pop("AUNCEL_AMD_DIST_BUDGET_MB", None)
    env.pop("AUNCEL_AMD_SEG_CAP_PAIRS", None)
    env.update(env_extra)
    p = subprocess.run([sys.executable, CHILD, name, out] + SELS, env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(f"child {tag}: exit {p.returncode}\n{p.stdout}")
    if p.returncode in FATAL:
        pytest.fail(f"child {tag} ended with {p.returncode}; no further child is started\n{p.stdout}")
    assert p.returncode == 0, p.stdout
    return np.load(out)


def test_deferred_queries_keep_their_own_selectors(capi, oracle, tmp_path):
    """test 4: under AUNCEL_AMD_DIST_BUDGET_MB=1 and AUNCEL_AMD_SEG_CAP_PAIRS=256 a round holds 32 of the 256 queries (8 probes each,
    rows padded to 1024 floats: 8192 floats a query against 2^18), the others are deferred to later passes, and launch position p of
    a pass is not query p: the results are the oracle's all the same, in more planning passes than without the knobs"""
    name = "sift_l2"
    sel_of = mixed(NQ)
    eD, eI = rows(oracle, name, capi, sel_of)
    heap, ndis = heap_updates(oracle, name, capi, sel_of), parent_ndis(oracle, name, capi)
    base = run_child(name, tmp_path, "baseline", {}, sel_of)
    cut = run_child(name, tmp_path, "cut", {"AUNCEL_AMD_DIST_BUDGET_MB": "1", "AUNCEL_AMD_SEG_CAP_PAIRS": "256"}, sel_of)
    for byte in (1, 0):
        for got, what in ((base, "baseline"), (cut, "cut")):
            same((got[f"b{byte}/D"], got[f"b{byte}/I"]), eD, eI, (byte, what))
            assert got[f"b{byte}/stats"].tolist()[2:] == [ndis, heap] and got[f"b{byte}/stats"][0] == NQ, (byte, what, got[f"b{byte}/stats"])
        r0, r1 = float(base[f"b{byte}/rounds"]), float(cut[f"b{byte}/rounds"])
        print("byte", byte, "planning passes", r0, "->", r1)
        assert r0 >= 1 and r1 > r0, (byte, r0, r1)


@pytest.mark.parametrize("name", ["sift_l2", "l2_96"])
def test_equivalences(capi, oracle, name):
    """test 5: one selector in the table is search_selected; a permuted table with sel_of remapped, a table that holds a selector
    twice and one that holds unused ones give the same bits; the same call twice around a larger unfiltered search does too"""
    metric, cen, assign, xb, xq, model = case(name)
    _, _, cd, ck, _, _, _ = expected(oracle, name, SELS[0], capi)
    h = handle(capi, metric, cen, xb, assign, 1)
    sels = make_selectors(capi, h, model)
    rs = np.random.RandomState(41)
    big = np.tile(xq, (4, 1))
    for byte in (1, 0):
        h.set_byte_codes(byte)
        for j in (1, 3):  # nsel == 1
            e = expected(oracle, name, SELS[j], capi)
            one = h.search_selected(sels[j], xq, K, NPROBE)
            same(one, e[4], e[5])
            same(h.search_selected_each([sels[j]], np.zeros(NQ, np.uint32), xq, K, NPROBE), *one)
            same(h.search_preassigned_selected_each([sels[j]], np.zeros(NQ, np.uint32), xq, K, ck, cd), *one)
        sel_of = mixed(NQ)
        eD, eI = rows(oracle, name, capi, sel_of)
        first = h.search_selected_each(sels, sel_of, xq, K, NPROBE)
        same(first, eD, eI)
        perm = rs.permutation(len(SELS))  # table position p holds selector perm[p]
        inv = np.argsort(perm).astype(np.uint32)
        same(h.search_selected_each([sels[p] for p in perm], inv[sel_of], xq, K, NPROBE), *first)
        # the same selector twice (positions 4 and 9, half of its queries each), and entries no query names (0 and 1)
        longer = [sels[4], sels[5]] + sels + [sels[2]]
        moved = sel_of + 2
        moved[(sel_of == 2) & (np.arange(NQ) % 2 == 0)] = len(longer) - 1
        same(h.search_selected_each(longer, moved, xq, K, NPROBE), *first)
        # the handle's history: a larger unfiltered search in between
        h.search(big, K, NPROBE)
        same(h.search_selected_each(sels, sel_of, xq, K, NPROBE), *first)
    close_all(sels)
    h.close()


def test_coarse_ties_redo(capi, oracle):
    """test 6: option coarse_ties = 2 on grid data whose coarse rankings are full of equal distances (test_gpu_coarse_ties.py's recipe,
    centroids duplicated), rankings of more than 128 entries: a call of 19 queries ranks with the reference's heap order and a call
    of 60 takes the oracle's ranking preassigned; every query keeps its own selector"""
    rs = np.random.RandomState(77)
    nlist, d, nb, nq, nprobe, metric = 300, 8, 4000, 60, 150, 1
    cen = rs.randint(0, 6, size=(nlist, d)).astype(np.float32)
    cen[nlist // 2:nlist // 2 + 20] = cen[:20]  # duplicated centroids
    xb = rs.randint(0, 6, size=(nb, d)).astype(np.float32)
    xq = rs.randint(0, 6, size=(nq, d)).astype(np.float32)
    assign = oracle.knn(metric, xb, cen, 1)[1][:, 0]
    model = Model(nlist, d, xb, assign)
    names = ["mod_3_1", "bits_half", "range_third", "bits_all"]
    cd, ck = oracle.knn(metric, xq, cen, nprobe)
    per = []
    for s in names:
        args, rule = selector(capi, s, model)
        per.append(oracle.search_preassigned(oracle_lists(oracle, metric, cen, filtered(model, rule)), xq, K, ck, cd))
    sel_of = mixed(nq, len(names))
    eD = np.stack([per[j][0][i] for i, j in enumerate(sel_of)])
    eI = np.stack([per[j][1][i] for i, j in enumerate(sel_of)])
    assert any(not np.array_equal(per[0][1][i], per[1][1][i]) for i in range(nq))
    h = handle(capi, metric, cen, xb, assign, 1)
    h.set_option("coarse_ties", 2)
    sels = make_selectors(capi, h, model, names)
    for byte in (1, 0):
        h.set_byte_codes(byte)
        before = h.coarse_tie_rows()
        for q in (slice(0, 19), slice(30, 49), slice(5, 6)):
            same(h.search_selected_each(sels, sel_of[q], xq[q], K, nprobe), eD[q], eI[q], (byte, q))
        assert h.coarse_tie_rows() > before, "no ranking went through the heap's tie order"
        same(h.search_preassigned_selected_each(sels, sel_of, xq, K, ck, cd), eD, eI, (byte, "preassigned"))
    close_all(sels)
    h.close()


def test_refusals_on_a_live_handle(capi, oracle):
    """test 7: a stale selector (after amd_ivf_add), a selector of another index, a null entry, an index out of range: -2 each, the
    message names the position, D and I are untouched, and the handle goes on searching"""
    C = capi.C
    name = "l2_96"
    metric, cen, assign, xb, xq, model = case(name)
    h = handle(capi, metric, cen, xb, assign, 1)
    other = handle(capi, metric, cen, xb, assign, 1)
    L = capi.lib()
    names = ["mod_3_1", "bits_half", "range_third"]
    sels = make_selectors(capi, h, model, names)
    foreign = other.selector(capi.SUBSET_ID_MOD, 2, 0)
    sel_of = mixed(NQ, len(names))
    eD, eI = rows(oracle, name, capi, sel_of, names)
    _, _, cd, ck, _, _, _ = expected(oracle, name, names[0], capi)
    h.set_queries(xq)
    u32p, f32p, i64p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_int64)

    def refused(table, so, word, nsel=None):
        """all three entry points through the raw ABI, on result arrays with a pattern in them"""
        D = np.full((NQ, K), 7.5, np.float32)
        I = np.full((NQ, K), -77, np.int64)
        t = (C.c_void_p * len(table))(*[s._s.value if s is not None else None for s in table])
        so = np.ascontiguousarray(so, dtype=np.uint32)
        ns = C.c_size_t(len(table) if nsel is None else nsel)
        a = (h._h, t, ns, so.ctypes.data_as(u32p))
        n, k, p = C.c_size_t(NQ), C.c_size_t(K), C.c_size_t(NPROBE)
        out = (D.ctypes.data_as(f32p), I.ctypes.data_as(i64p))
        for rc in (L.amd_ivf_search_selected_each(*a, n, xq.ctypes.data_as(f32p), k, p, 0, *out),
                   L.amd_ivf_search_preassigned_selected_each(*a, n, xq.ctypes.data_as(f32p), k, p, ck.ctypes.data_as(i64p), None, *out),
                   L.amd_ivf_search_resident_selected_each(*a, C.c_size_t(0), n, k, p, 0, *out)):
            assert rc == -2
            assert word in L.amd_ivf_last_error().decode(), L.amd_ivf_last_error()
            assert (D == 7.5).all() and (I == -77).all(), "a refused call wrote results"

    same(h.search_selected_each(sels, sel_of, xq, K, NPROBE), eD, eI)
    refused([sels[0], foreign, sels[2]], sel_of, "selector 1 of the table was made on another index")
    refused([sels[0], sels[1], None], sel_of, "selector 2 of the table is null")
    refused([sels[0], sels[1], foreign], np.zeros(NQ, np.uint32), "selector 2 of the table was made on another index")  # (used or not)
    bad = sel_of.copy()
    bad[123] = 3
    refused(sels, bad, "sel_of[123] = 3")
    bad[123] = 0xffffffff
    refused(sels, bad, "sel_of[123] = 4294967295")
    refused(sels, sel_of, "nsel == 0", nsel=0)
    # a resident range that wraps, and one that ends behind the resident queries
    D, I = np.full((4, K), 7.5, np.float32), np.full((4, K), -77, np.int64)
    t = (C.c_void_p * 3)(*[s._s.value for s in sels])
    for start, n, word in ((2 ** 64 - 1, 4, "wraps"), (NQ - 2, 4, "out of bounds")):
        rc = L.amd_ivf_search_resident_selected_each(h._h, t, C.c_size_t(3), sel_of.ctypes.data_as(u32p), C.c_size_t(start), C.c_size_t(n),
                                                     C.c_size_t(K), C.c_size_t(NPROBE), 0, D.ctypes.data_as(f32p), I.ctypes.data_as(i64p))
        assert rc == -2 and word in L.amd_ivf_last_error().decode() and (D == 7.5).all() and (I == -77).all()
    # no queries: 0, nothing written (not even with an empty table)
    assert L.amd_ivf_search_selected_each(h._h, t, C.c_size_t(0), sel_of.ctypes.data_as(u32p), C.c_size_t(0), None, C.c_size_t(K),
                                          C.c_size_t(NPROBE), 0, D.ctypes.data_as(f32p), I.ctypes.data_as(i64p)) == 0
    assert (D == 7.5).all() and (I == -77).all()
    same(h.search_selected_each(sels, sel_of, xq, K, NPROBE), eD, eI, "after the refusals")
    # stale: amd_ivf_add changes the lists under every selector of the table
    h.add(xq[:5].copy(), np.arange(9001, 9006, dtype=np.int64), np.arange(5, dtype=np.int64))
    refused(sels, sel_of, "selector 0 of the table is stale")
    with pytest.raises(capi.EngineError) as err:
        h.search_selected_each(sels, sel_of, xq, K, NPROBE)
    assert err.value.code == -2
    close_all(sels)
    # the handle is still usable: new selectors over the lists as they are now
    m2 = Model(cen.shape[0], cen.shape[1], xb, assign)
    m2.add(xq[:5].copy(), np.arange(9001, 9006, dtype=np.int64), np.arange(5))
    per = [expected(oracle, name, s, capi, model=m2) for s in names]
    eD2 = np.stack([per[j][4][i] for i, j in enumerate(sel_of)])
    eI2 = np.stack([per[j][5][i] for i, j in enumerate(sel_of)])
    sels = make_selectors(capi, h, m2, names)
    same(h.search_selected_each(sels, sel_of, xq, K, NPROBE), eD2, eI2, "after the add")
    close_all(sels)
    foreign.close()
    h.close()
    other.close()
