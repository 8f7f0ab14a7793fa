"""The scan's arithmetic choice at the edges of its exactness rule (IntRange in ivf_engine.hip), on every path that makes it.

Cases, rule and model: tests/arith_edge_cases.py; their premise -- on every teeth case a fused sum differs from the reference's on
pairs a search RETURNS -- holds without a GPU in tests/test_arith_edge_cases_cpu.py.  Here every case must report the arithmetic
the rule gives (amd_ivf_scan_arith: the list scan's) and equal the pinned oracle bit for bit: (D, I), range results, statistics,
coarse rankings.  The reference is always the oracle, never a second run of the engine.  A call fused one step outside the rule,
a call site that joins the wrong pair of ranges, a range left too narrow by a change of the lists, or a fused kernel reached with
fused = 0 unset fails the bits of a teeth case; a rule that is too timid fails the reported arithmetic of an inside case."""
import numpy as np
import pytest

import arith_edge_cases as E
from arith_edge_cases import bits

gpu = pytest.mark.gpu
FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def new_handle(capi, c):
    h = capi.Handle(c["d"], c["nlist"], c["metric"], 0)
    h.set_centroids(c["cen"])
    h.set_lists_from_assign(c["xb"], c["assign"])
    return h


def same(got, want, tag):
    """(D, I) against the oracle's"""
    assert np.array_equal(got[1], want[1]), tag
    assert np.array_equal(bits(got[0]), bits(want[0])), tag


def searched(h, fn, *args, **kw):
    """a search and the statistics it added: (D, I), [nlist, ndis, nheap_updates]"""
    h.stats(reset=True)
    out = fn(*args, **kw)
    st = h.stats()
    return out, [st["nlist"], st["ndis"], st["nheap_updates"]]


# ------------------------------------------------------------------------------------------------------------------------------
# search_preassigned: every work-item shape (calls of 3 / 70 / 300 queries), both fp32 scan kernels (lanes), one and two rounds,
# the threshold round with and without the matrix-core filter, both selections
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", E.NAMES)
def test_search_preassigned(capi, name):
    c = E.case(name)
    h = new_handle(capi, c)
    for nq in E.CALLS:
        xq, keys = c["xq"][:nq], c["keys"][:nq]
        for k in E.KS:
            eD, eI, est = E.expected(name, nq, k)
            for rounds in (1, 2):
                for select in (0, 1):
                    for lanes in (0, 1):
                        for flt in (0, 2):
                            for key, v in (("fixed_rounds", rounds), ("select", select), ("lanes", lanes), ("filter", flt)):
                                h.set_option(key, v)
                            (D, I), st = searched(h, h.search_preassigned, xq, k, keys)
                            tag = f"{name} nq={nq} k={k} rounds={rounds} select={select} lanes={lanes} filter={flt}"
                            assert h.scan_arith() == c["arith"], tag
                            same((D, I), (eD, eI), tag)
                            assert st == list(est), tag
    for key in ("fixed_rounds", "select", "lanes", "filter"):
        h.set_option(key, None)
    eD, eI, est = E.expected(name, 70, 10, store_pairs=True)
    (D, I), st = searched(h, h.search_preassigned, c["xq"][:70], 10, c["keys"][:70], store_pairs=True)
    assert h.scan_arith() == c["arith"]
    same((D, I), (eD, eI), (name, "store_pairs"))
    assert st == list(est)
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the engine's own coarse ranking: the centroids' range against the queries', whatever the lists hold
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", E.NAMES)
def test_own_coarse_ranking(capi, oracle, name):
    c = E.case(name)
    h = new_handle(capi, c)
    for nq in E.CALLS:
        xq = c["xq"][:nq]
        for nprobe in (E.NPROBE, E.NLIST):
            ecd, eck = oracle.knn(c["metric"], xq, c["cen"], nprobe)
            cd, ck = h.coarse(xq, nprobe, mode=0)
            assert np.array_equal(ck, eck), (name, nq, nprobe)
            assert np.array_equal(bits(cd), bits(ecd)), (name, nq, nprobe)
        for k in (10, 100):
            _, _, eD, eI, est = E.expected_ranked(name, nq, k)
            (D, I), st = searched(h, h.search, xq, k, E.NPROBE, coarse_mode=0)
            assert h.scan_arith() == c["arith"], (name, nq, k)
            same((D, I), (eD, eI), (name, nq, k))
            assert st == list(est), (name, nq, k)
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the other search forms
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", E.NAMES)
def test_range_search(capi, oracle, name):
    """the radius sits on a probed pair whose fused sum has other bits than the oracle's distance (teeth cases), so that the pair is
    inside at one value and outside at the other: a wrongly fused scan changes the result's membership"""
    c = E.case(name)
    h = new_handle(capi, c)
    lists = E.oracle_lists(c)
    nq = 70
    xq = c["xq"][:nq]
    for own in (False, True):
        keys = E.expected_ranked(name, nq, 10)[1] if own else c["keys"][:nq]
        radius, flips = E.flipping_radius(name, nq, keys)
        assert flips if c["teeth"] else not (flips and c["arith"] >= 1), (name, own)
        elims, elab, edis, est = oracle.range_search_preassigned(lists, xq, radius, keys)
        assert 0 < elims[-1] < E.probed_mask(c["assign"], keys).sum()
        h.stats(reset=True)
        if own:
            lims, lab, dis = h.range_search(xq, radius, E.NPROBE, coarse_mode=0)
        else:
            lims, lab, dis = h.range_search(xq, radius, E.NPROBE, keys=keys)
        st = h.stats()
        assert h.scan_arith() == c["arith"], (name, own)
        assert np.array_equal(lims, elims) and np.array_equal(lab, elab), (name, own)
        assert np.array_equal(bits(dis), bits(edis)), (name, own)
        assert [st["nlist"], st["ndis"]] == list(est), (name, own)
    h.close()


@gpu
@pytest.mark.parametrize("name", E.NAMES)
def test_timed_and_exact_search(capi, oracle, name):
    """search_timed with all the time in the world is search(); search_exact the general way (exact_float unset) is
    search_preassigned over every list in list-number order"""
    c = E.case(name)
    h = new_handle(capi, c)
    lists = E.oracle_lists(c)
    for nq in (70, 300):
        xq = c["xq"][:nq]
        _, _, eD, eI, _ = E.expected_ranked(name, nq, 10)
        h.set_queries(xq)
        D, I, used = h.search_timed(0, nq, 10, E.NPROBE, np.full(nq, 1e9, np.float32), coarse_mode=0)
        assert h.scan_arith() == c["arith"], (name, nq)
        assert (used == E.NPROBE).all()
        same((D, I), (eD, eI), (name, nq, "timed"))
        D, I, used = h.search_timed_x(xq, 0, 10, E.NPROBE, np.full(nq, 1e9, np.float32), coarse_mode=0)
        assert h.scan_arith() == c["arith"], (name, nq)
        same((D, I), (eD, eI), (name, nq, "timed_x"))
    nq = 70
    xq = c["xq"][:nq]
    every = np.tile(np.arange(E.NLIST, dtype=np.int64), (nq, 1))
    eD, eI, _ = oracle.search_preassigned(lists, xq, 10, every, np.zeros(every.shape, np.float32))
    D, I = h.search_exact(xq, 10)
    if c["arith"] != 2:  # (byte lists take a list pass of their own, which reports no scan arithmetic)
        assert h.scan_arith() == c["arith"], name
    same((D, I), (eD, eI), (name, "exact"))
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the scanner: one query against one list, or a run of one
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", E.NAMES)
def test_scanner(capi, oracle, name):
    c = E.case(name)
    metric, is_l2 = c["metric"], c["metric"] == E.L2
    h = new_handle(capi, c)
    lists = E.oracle_lists(c)
    want, fused = E.model_tables(name, 70)
    k = 100

    def fresh():
        return np.full(k, FMAX if is_l2 else -FMAX, dtype=np.float32), np.full(k, -1, dtype=np.int64)

    for q in (0, 1, 5):
        x = c["xq"][q]
        for l in (1, 2, 6):
            b, e = int(lists.off[l]), int(lists.off[l + 1])
            codes, ids = lists.codes[b:e], lists.ids[b:e]
            for pairs in (False, True):
                simi, idxi = fresh()
                wsimi, widxi = fresh()
                nup = h.scan_codes(x, l, simi, idxi, store_pairs=pairs)
                assert nup == oracle.scan_codes(metric, x, codes, ids, l, pairs, wsimi, widxi), (name, q, l)
                assert np.array_equal(bits(simi), bits(wsimi)) and np.array_equal(idxi, widxi), (name, q, l, pairs)
            # one entry: the first whose fused sum would differ (teeth cases), and the list's first
            differ = np.nonzero(bits(fused[q, ids]) != bits(want[q, ids]))[0]
            for o in {0, int(differ[0]) if len(differ) else 0}:
                assert bits(h.distance_to_code(x, l, o)) == bits(want[q, ids[o]]), (name, q, l, o)
        # a run of the long list across the tile edges at 128 and 256
        l, a, n = 6, 100, 200
        b = int(lists.off[l]) + a
        codes, ids = lists.codes[b:b + n], lists.ids[b:b + n]
        simi, idxi = fresh()
        wsimi, widxi = fresh()
        nup = h.scan_codes_at(x, l, a, n, simi, idxi)
        assert nup == oracle.scan_codes(metric, x, codes, ids, l, False, wsimi, widxi), (name, q)
        assert np.array_equal(bits(simi), bits(wsimi)) and np.array_equal(idxi, widxi), (name, q)
        od = want[q, ids]
        radius, _ = E.radius_on_teeth(metric, od, fused[q, ids])
        pos, dis = h.scan_codes_range(x, l, a, n, radius)
        keep = np.nonzero(od < radius if is_l2 else od > radius)[0]
        assert 0 < len(keep) < n
        assert np.array_equal(pos, keep.astype(np.uint32)), (name, q)
        assert np.array_equal(bits(dis), bits(od[keep])), (name, q)
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# resident queries
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_resident_queries(capi, oracle):
    """The contract: the range of the RESIDENT SET decides, not the slice's.  A set whose last row alone breaks the rule is scanned
    in the reference's order (scan_arith 0) even by a slice without that row -- the range is taken once, by set_queries; the same
    rows set without the last one are scanned fused (1).  The bits are the oracle's either way."""
    name = E.LIFE_CASE
    c = E.case(name)
    h = new_handle(capi, c)
    x = E.resident_rows()
    n = E.NQ
    lists = E.oracle_lists(c)
    _, eck, eD, eI, _ = E.expected_ranked(name, n, 10)
    pD, pI, _ = E.expected(name, n, 10)
    # the slice that holds the last row, under the oracle's ranking
    tail = x[n - 69:]
    tcd, tck = oracle.knn(c["metric"], tail, c["cen"], E.NPROBE)
    tD, tI, _ = oracle.search_preassigned(lists, tail, 10, tck, tcd)
    for rows, arith in ((x, 0), (x[:-1], 1), (x, 0)):
        h.set_queries(rows)
        for start, m in ((0, n), (0, 70), (64, 130)):
            same(h.search_resident(start, m, 10, E.NPROBE), (eD[start:start + m], eI[start:start + m]), (arith, start, m))
            assert h.scan_arith() == arith, (arith, start, m)
            same(h.search_resident_preassigned(start, m, 10, c["keys"][start:start + m]), (pD[start:start + m], pI[start:start + m]),
                 (arith, start, m, "preassigned"))
            assert h.scan_arith() == arith, (arith, start, m)
            cd, ck = h.coarse_resident(start, m, E.NPROBE, mode=0)
            assert np.array_equal(ck, eck[start:start + m])
        D, I, used = h.search_timed(0, n, 10, E.NPROBE, np.full(len(rows), 1e9, np.float32), coarse_mode=0)
        assert h.scan_arith() == arith
        same((D, I), (eD, eI), (arith, "timed"))
        if arith == 0:
            same(h.search_resident(n - 69, 70, 10, E.NPROBE), (tD, tI), "tail")
            assert h.scan_arith() == 0
    # the caller's rows are ranged call by call
    same(h.search(x[:n], 10, E.NPROBE), (eD, eI), "host rows")
    assert h.scan_arith() == 1
    same(h.search(tail, 10, E.NPROBE), (tD, tI), "host tail")
    assert h.scan_arith() == 0
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the lists' range over the handle's life
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("incremental", [1, 0])
def test_ranges_over_the_handles_life(capi, incremental):
    """An inside-rule index; one row that makes the spread 4097 comes (add, update_lists) and goes (remove_ids, update_lists back):
    the arithmetic follows, 1 -> 0 -> 1, and the bits are the oracle's over the lists as they stand.  Subsets take the range of
    what they keep; a clone reports its owner's choice."""
    c, f = E.case(E.LIFE_CASE), E.life()
    xq, keys, k = c["xq"], c["keys"], E.LIFE_K
    base, added, updated = (E.life_expected(s)[:2] for s in ("base", "added", "updated"))
    h = new_handle(capi, c)
    h.set_option("incremental", incremental)

    def check(handle, want, arith, tag):
        same(handle.search_preassigned(xq, k, keys), want, tag)
        assert handle.scan_arith() == arith, tag

    check(h, base, 1, "base")
    h.add(f["w"], xids=np.array([E.LIFE_ID]), precomputed_idx=np.array([E.LIFE_LIST]))
    check(h, added, 0, "added")
    cl = h.clone()
    check(cl, added, 0, "clone, added")
    assert h.scan_arith() == 0
    cl.close()
    without = h.subset(capi.SUBSET_ID_RANGE, 0, E.LIFE_ID)
    check(without, base, 1, "subset without the row")
    without.close()
    with_row = h.subset(capi.SUBSET_ID_RANGE, 0, E.LIFE_ID + 1)
    check(with_row, added, 0, "subset with the row")
    with_row.close()
    assert h.remove_ids(np.array([E.LIFE_ID])) == 1
    check(h, base, 1, "removed")
    sizes = np.array(E.LENGTHS)
    where = np.array([(E.LIFE_OVERWRITE[0] << 32) | E.LIFE_OVERWRITE[1]], dtype=np.uint64)
    h.update_lists(sizes, where, np.array([f["over"]]), f["w"])
    check(h, updated, 0, "overwritten")
    cl = h.clone()
    check(cl, updated, 0, "clone, overwritten")
    cl.close()
    h.update_lists(sizes, where, np.array([f["over"]]), c["xb"][f["over"]][None, :])
    check(h, base, 1, "written back")
    h.close()
