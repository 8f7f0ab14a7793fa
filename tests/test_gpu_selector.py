"""Search under an id selector without a subset index (amd_ivf_selector_create, amd_ivf_search_selected ..., ivf_selector.hip): the
keep bits of the selector enter every round of a fixed-nprobe search of the PARENT's lists.  The expected value is the pinned CPU
oracle over the lists with the non-members removed (the numpy restatement of copy_subset_to in test_gpu_subset.py), and the same
call on amd_ivf_subset of the same selector.  Every comparison is of bits or of integers."""
import functools

import numpy as np
import pytest

from test_gpu_subset import filtered, oracle_lists, selector
from test_gpu_update import K, NPROBE, NQ, Model, bits, handle, make_case

pytestmark = pytest.mark.gpu

CASES = ["sift_l2", "l2_96", "ip_96", "odd_30", "ragged", "bytes_200", "bytes_960"]
SELECTORS = ["range_third", "mod_3_1", "slice_mid", "bits_half", "bits_1pct", "bits_all", "bits_none", "batch_200", "bits_lists"]
# (byte codes, "filter"): the byte path where the lists qualify, fp32 with the filter the engine picks, the fp16 and the fp32 filter
CONFIGS = [(1, None), (0, None), (0, 2), (0, 1)]


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


@functools.lru_cache(maxsize=None)
def case(name):
    metric, cen, assign, xb, xq = make_case(name)
    return metric, cen, assign, xb, xq, Model(cen.shape[0], cen.shape[1], xb, assign)


_expected = {}


def expected(oracle, name, sel_name, capi, model=None):
    """(kind, a1, a2, sel), the filtered lists, and the oracle's (D, I, stats) over them at (K, NPROBE); computed once"""
    key = (name, sel_name)
    if model is not None or key not in _expected:
        metric, cen, assign, xb, xq, m0 = case(name)
        m = model if model is not None else m0
        args, rule = selector(capi, sel_name, m)
        want = filtered(m, rule)
        cd, ck = oracle.knn(metric, xq, cen, NPROBE)
        eD, eI, est = oracle.search_preassigned(oracle_lists(oracle, metric, cen, want), xq, K, ck, cd)
        out = (args, want, cd, ck, eD, eI, est)
        if model is not None:
            return out
        _expected[key] = out
    return _expected[key]


def same(got, eD, eI, what=None):
    D, I = got
    assert np.array_equal(I, eI), what
    assert np.array_equal(bits(D), bits(eD)), what


def configure(h, byte, filt):
    h.set_byte_codes(byte)
    h.set_option("filter", filt)


@pytest.mark.parametrize("sel_name", SELECTORS)
@pytest.mark.parametrize("name", CASES)
def test_selected_search_equals_the_oracle_and_the_subset(capi, oracle, name, sel_name):
    """checks 1 and 2: search_preassigned_selected and search_selected of the parent against the oracle over the filtered lists and
    against search of parent.subset(...); nheap_updates is the filtered lists', ndis the parent's"""
    metric, cen, assign, xb, xq, model = case(name)
    (kind, a1, a2, sel), want, cd, ck, eD, eI, est = expected(oracle, name, sel_name, capi)
    _, _, pst = oracle.search_preassigned(oracle_lists(oracle, metric, cen, model), xq, K, ck, cd)
    parent = handle(capi, metric, cen, xb, assign, 1)
    sub = parent.subset(kind, a1, a2, sel)
    same(sub.search(xq, K, NPROBE), eD, eI, "subset")
    with parent.selector(kind, a1, a2, sel) as s:
        assert s.info()[1] == sum(len(i) for i in want.ids)
        for byte, filt in CONFIGS:
            configure(parent, byte, filt)
            configure(sub, byte, filt)
            sD, sI = sub.search(xq, K, NPROBE)
            parent.stats(reset=True)
            got = parent.search_preassigned_selected(s, xq, K, ck, cd)
            st = parent.stats()
            same(got, eD, eI, (byte, filt, "preassigned"))
            same(got, sD, sI, (byte, filt, "preassigned / subset"))
            assert st["nheap_updates"] == est[2] and st["ndis"] == pst[1], (st, est, pst)
            got = parent.search_selected(s, xq, K, NPROBE)
            same(got, eD, eI, (byte, filt, "search"))
            same(got, sD, sI, (byte, filt, "search / subset"))
        if sel_name == "bits_none":
            assert (eI == -1).all()
        if sel_name == "bits_1pct":
            # fewer than k members: at NPROBE probes some cases still find k among the ~15 members they probe (sift_l2 and bytes_960
            # do for every query), so the same selector again at 2 probes, where a query reaches ~4 members and some reach none
            cd2, ck2 = oracle.knn(metric, xq, cen, 2)
            pD, pI, pst2 = oracle.search_preassigned(oracle_lists(oracle, metric, cen, want), xq, K, ck2, cd2)
            assert (pI[:, -1] == -1).all() and (pI[:, 0] == -1).any() and (pI[:, 0] >= 0).any(), "the padding is not exercised"
            for byte, filt in CONFIGS:
                configure(parent, byte, filt)
                configure(sub, byte, filt)
                parent.stats(reset=True)
                got = parent.search_preassigned_selected(s, xq, K, ck2, cd2)
                assert parent.stats()["nheap_updates"] == pst2[2]
                same(got, pD, pI, (byte, filt, "padding, preassigned"))
                same(parent.search_selected(s, xq, K, 2), pD, pI, (byte, filt, "padding, search"))
                same(sub.search(xq, K, 2), pD, pI, (byte, filt, "padding, subset"))
        if sel_name == "bits_all":
            configure(parent, 1, None)
            same(parent.search(xq, K, NPROBE), eD, eI, "unfiltered")
    sub.close()
    parent.close()


@pytest.mark.parametrize("select", [1, 0])
@pytest.mark.parametrize("row_lists", [0, 1])
@pytest.mark.parametrize("name", ["sift_l2", "l2_96", "ip_96"])
def test_threshold_rounds_carry_the_keep_bits(capi, oracle, name, row_lists, select):
    """check 3: fixed_rounds 2 -- a dense round over the first probes, a threshold round over the rest -- with the selection reading
    the threshold round's rows from the mask walk (row_lists 0) and from compact_rows_kernel's lists (1); select 0: the heap kernels"""
    metric, cen, assign, xb, xq, model = case(name)
    parent = handle(capi, metric, cen, xb, assign, 1)
    parent.set_option("fixed_rounds", 2)
    parent.set_option("row_lists", row_lists)
    parent.set_option("select", select)
    for sel_name in ("bits_half", "bits_lists", "bits_1pct", "mod_3_1"):
        (kind, a1, a2, sel), want, cd, ck, eD, eI, est = expected(oracle, name, sel_name, capi)
        with parent.selector(kind, a1, a2, sel) as s:
            parent.stats(reset=True)
            same(parent.search_preassigned_selected(s, xq, K, ck, cd), eD, eI, sel_name)
            assert parent.stats()["nheap_updates"] == est[2]
            thr_bytes = parent.last_timing_detail()["min_bytes_thr"]
            print(name, sel_name, "row_lists", row_lists, "select", select, "min_bytes_thr", thr_bytes, "filter", parent.last_filter())
            assert thr_bytes > 0, "no threshold round ran"
            if name == "sift_l2":
                assert parent.scan_arith() == 2
            else:
                assert parent.last_filter()[0] >= 1, "the threshold round did not go through the filter"
            same(parent.search_selected(s, xq, K, NPROBE), eD, eI, sel_name)
    parent.close()


@pytest.mark.parametrize("fixed_rounds", [None, 2])
@pytest.mark.parametrize("name", ["sift_l2", "odd_30", "bytes_960"])
def test_small_calls(capi, oracle, name, fixed_rounds):
    """check 4: calls of 1, 19 and 32 queries are planned by plan_one_kernel / plan_small_kernel"""
    metric, cen, assign, xb, xq, model = case(name)
    parent = handle(capi, metric, cen, xb, assign, 1)
    parent.set_option("fixed_rounds", fixed_rounds)
    for sel_name in ("mod_3_1", "bits_1pct", "bits_lists"):
        (kind, a1, a2, sel), want, cd, ck, eD, eI, est = expected(oracle, name, sel_name, capi)
        with parent.selector(kind, a1, a2, sel) as s:
            for byte in (1, 0):
                parent.set_byte_codes(byte)
                for n0, n in ((0, 1), (7, 1), (40, 19), (100, 32), (3, 33)):
                    q = slice(n0, n0 + n)
                    same(parent.search_preassigned_selected(s, xq[q], K, ck[q], cd[q]), eD[q], eI[q], (sel_name, byte, n0, n))
                    same(parent.search_selected(s, xq[q], K, NPROBE), eD[q], eI[q], (sel_name, byte, n0, n))
    parent.close()


@pytest.mark.parametrize("name", ["sift_l2", "ip_96"])
def test_search_resident_selected(capi, oracle, name):
    """check 5: two slices of the resident queries, from the owner and from a clone"""
    metric, cen, assign, xb, xq, model = case(name)
    (kind, a1, a2, sel), want, cd, ck, eD, eI, est = expected(oracle, name, "range_third", capi)
    parent = handle(capi, metric, cen, xb, assign, 1)
    parent.set_queries(xq)
    c = parent.clone()
    with parent.selector(kind, a1, a2, sel) as s:
        for h in (parent, c):
            for start, n in ((0, 100), (100, NQ - 100)):
                same(h.search_resident_selected(s, start, n, K, NPROBE), eD[start:start + n], eI[start:start + n], (start, n))
    c.close()
    parent.close()


@pytest.mark.parametrize("name", ["sift_l2", "l2_96"])
def test_two_selectors_alive_at_once(capi, oracle, name):
    """check 6: two selectors of one index used alternately, from the owner and from a clone; the parent's own search and its
    layout are what they were"""
    metric, cen, assign, xb, xq, model = case(name)
    ea = expected(oracle, name, "mod_3_1", capi)
    eb = expected(oracle, name, "bits_half", capi)
    parent = handle(capi, metric, cen, xb, assign, 1)
    D0, I0 = parent.search(xq, K, NPROBE)
    before = parent.layout_digest()
    sa, sb = parent.selector(*ea[0]), parent.selector(*eb[0])
    c = parent.clone()
    for h in (parent, c, parent):
        for s, e in ((sa, ea), (sb, eb), (sa, ea), (sb, eb)):
            same(h.search_selected(s, xq, K, NPROBE), e[4], e[5])
            same(h.search_preassigned_selected(s, xq, K, e[3], e[2]), e[4], e[5])
        same(h.search(xq, K, NPROBE), D0, I0, "unfiltered, between")
    sa.close()
    same(parent.search_selected(sb, xq, K, NPROBE), eb[4], eb[5])
    sb.close()
    c.close()
    same(parent.search(xq, K, NPROBE), D0, I0, "unfiltered, after")
    assert parent.layout_digest() == before
    parent.close()


@pytest.mark.parametrize("name", ["sift_l2", "ip_96"])
def test_a_selector_goes_stale_with_the_lists(capi, oracle, name):
    """check 7: after amd_ivf_add a search with the old selector returns -2; a new selector sees the added rows"""
    metric, cen, assign, xb, xq, _ = case(name)
    nlist, d = cen.shape
    model = Model(nlist, d, xb, assign)
    parent = handle(capi, metric, cen, xb, assign, 1)
    args, _ = selector(capi, "mod_3_1", model)
    old = parent.selector(*args)
    e = expected(oracle, name, "mod_3_1", capi)
    same(parent.search_selected(old, xq, K, NPROBE), e[4], e[5])
    rs = np.random.RandomState(4)
    lists = rs.randint(0, nlist, size=40)
    x = xq[:40].copy()  # (rows the queries will find: the new members reach the results)
    ids = np.arange(3001, 3001 + 3 * len(lists), 3, dtype=np.int64)  # (3001 % 3 == 1: the selector keeps them)
    parent.add(x, ids, lists)
    model.add(x, ids, lists)
    L = capi.lib()
    c = parent.clone()
    for h in (parent, c):
        for call in (lambda: h.search_selected(old, xq, K, NPROBE), lambda: h.search_preassigned_selected(old, xq, K, e[3], e[2]),
                     lambda: h.search_resident_selected(old, 0, 1, K, NPROBE)):
            with pytest.raises(capi.EngineError) as err:
                call()
            assert err.value.code == -2 and "stale" in L.amd_ivf_last_error().decode()
    c.close()
    old.close()
    args, want, cd, ck, eD, eI, est = expected(oracle, name, "mod_3_1", capi, model=model)
    assert np.isin(eI, ids).any(), "no added row among the results"
    with parent.selector(*args) as new:
        assert new.info()[0] == len(xb) + len(lists)
        same(parent.search_selected(new, xq, K, NPROBE), eD, eI)
        same(parent.search_preassigned_selected(new, xq, K, ck, cd), eD, eI)
        # ... and the other calls that change the lists
        parent.remove_ids(ids[:3])
        with pytest.raises(capi.EngineError) as err:
            parent.search_selected(new, xq, K, NPROBE)
        assert err.value.code == -2
    parent.close()


@pytest.mark.parametrize("sel_name", SELECTORS)
def test_selector_info(capi, oracle, sel_name):
    """check 8: looked-at, kept, host-to-device bytes (the subset test's own bound) and the device bytes a selector holds: a bit per
    padded entry, 4 bytes of count per word, the per-list table"""
    metric, cen, assign, xb, xq, model = case("ragged")
    nlist = cen.shape[0]
    (kind, a1, a2, sel), rule = selector(capi, sel_name, model)
    want = filtered(model, rule)
    parent = handle(capi, metric, cen, xb, assign, 1)
    with parent.selector(kind, a1, a2, sel) as s:
        looked, kept, h2d, held = s.info()
        print(sel_name, s.info())
        assert looked == len(xb) == parent.ntotal
        assert kept == sum(len(i) for i in want.ids)
        assert h2d <= (0 if sel is None else 8 * len(sel)) + 16 * (nlist + 1) + 65536
        nwords = sum((len(i) + 63) // 64 for i in model.ids)
        assert 0 < held <= 8 * nwords + 4 * nwords + 4 * nlist, (held, nwords)
    parent.close()


def test_refusals(capi, oracle):
    """check 9, and the argument checks of amd_ivf_subset"""
    metric, cen, assign, xb, xq, model = case("l2_96")
    parent = handle(capi, metric, cen, xb, assign, 1)
    other = handle(capi, metric, cen, xb, assign, 1)
    L = capi.lib()

    def refused(f, word=None):
        with pytest.raises(capi.EngineError) as e:
            f()
        assert e.value.code == -2, e.value
        if word:
            assert word in L.amd_ivf_last_error().decode(), L.amd_ivf_last_error()

    s = parent.selector(capi.SUBSET_ID_MOD, 2, 0)
    # a selector of another index (the same lists, but not the same index); of a subset of the index
    refused(lambda: other.search_selected(s, xq, K, NPROBE), "another index")
    sub = parent.subset(capi.SUBSET_ID_MOD, 2, 0)
    refused(lambda: sub.search_selected(s, xq, K, NPROBE), "another index")
    sub.close()
    # the index is not destroyed under a live selector, and says how many there are
    s2 = parent.selector(capi.SUBSET_ID_RANGE, 0, 50)
    refused(parent.close, "2 selector")
    s2.close()
    refused(parent.close, "1 selector")
    assert parent.search_selected(s, xq, K, NPROBE)[0].shape == (NQ, K)  # (still a valid handle)
    # bad arguments
    for bad in ((3, 2, 0), (4, 2, 0), (7, 0, 0), (-1, 0, 0), (capi.SUBSET_ID_MOD, 0, 0), (capi.SUBSET_ID_MOD, -3, 0), (capi.SUBSET_SLICE, 10, 5),
                (capi.SUBSET_SLICE, 0, len(xb) + 1)):
        refused(lambda: parent.selector(*bad))
    out = capi.C.c_void_p()
    for kind in (capi.SUBSET_ID_BITS, capi.SUBSET_ID_BATCH):
        assert L.amd_ivf_selector_create(parent._h, kind, capi.C.c_int64(0), capi.C.c_int64(0), None, capi.C.c_size_t(4), capi.C.byref(out)) == -2
    c = parent.clone()
    refused(lambda: c.selector(capi.SUBSET_ID_MOD, 2, 0))
    c.close()
    parent.set_queries(xq)
    t = parent.submit_search_resident(0, NQ, K, NPROBE)
    refused(lambda: parent.selector(capi.SUBSET_ID_MOD, 2, 0), "tickets")
    parent.wait(t)
    # an empty SLICE and an empty index are valid
    with parent.selector(capi.SUBSET_SLICE, 5, 5) as e:
        assert e.info()[:2] == (len(xb), 0)
        assert (parent.search_selected(e, xq[:5], K, NPROBE)[1] == -1).all()
    empty = capi.Handle(cen.shape[1], cen.shape[0], metric, 0)
    empty.set_centroids(cen)
    with empty.selector(capi.SUBSET_ID_RANGE, 0, 100) as e:
        assert e.info()[:2] == (0, 0)
        assert (empty.search_selected(e, xq[:5], K, NPROBE)[1] == -1).all()
    empty.close()
    s.close()
    parent.close()
    other.close()
