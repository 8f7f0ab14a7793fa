"""Float searches at the ends of the fp32 range: norms and products that overflow, NaN and infinite elements, subnormal distances
(worlds and model: tests/extreme_range_cases.py; their premises hold without a GPU in tests/test_extreme_range_cases_cpu.py).

Everything is the pinned oracle's, bit for bit: ids, distance bits and the statistics (nlist, ndis, nheap_updates), for every query of
every call -- nothing is excluded.  The matrix-core filter of threshold rounds (ivf_filter.hip) decides which candidates are
recomputed at all; its error bound is derived for finite arithmetic, and outside it the rule is "kept and rescored": a query or a row
whose norm lies outside the bound's range (filter_bound_u: overflowing, NaN, or so small that products leave the normal range)
is not filtered.  The filter still runs on these worlds (last_filter() counts its rounds): no call leaves it.  None of them has a
usable fp16 scale (a non-finite element, or magnitudes outside 2^+-24), so under option "filter" = 2 the fp16 copy is refused and
the fp32 copy serves (layout_digest: no fp16 copy, an fp32 copy), and the exact calls go the general way for every query
(last_exact: none answered by a list pass).

On an MI355X, with the keep test `t > u` alone (as it stood): l2_norm_overflow, ip_norm_overflow and integers_2p62 failed at every
d in every form with a filtered round, in the exact calls and on the clone; nonfinite_l2 and subnormal passed; nonfinite_ip failed
in every form with the sorted selection, which returned a NaN among a query's first k candidates as its best inner product
(select_sorted_kernel's first-block fill)."""
import numpy as np
import pytest

import extreme_range_cases as X
from extreme_range_cases import bits

pytestmark = pytest.mark.gpu
CASES = [(name, d) for name in X.WORLDS for d in X.DS]


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


@pytest.fixture(autouse=True)
def quiet():
    with np.errstate(all="ignore"):
        yield


def new_handle(capi, w):
    h = capi.Handle(w["d"], w["nlist"], w["metric"], 0)
    h.set_centroids(w["cen"])
    h.set_lists_from_assign(w["xb"], w["assign"])
    return h


def same(got, want, tag):
    bad = np.nonzero((got[1] != want[1]).any(axis=1) | (bits(got[0]) != bits(want[0])).any(axis=1))[0]
    assert bad.size == 0, (tag, "queries", bad[:8], got[1][bad[0]], want[1][bad[0]], got[0][bad[0]], want[0][bad[0]])


def searched(h, fn, *args, **kw):
    h.stats(reset=True)
    out = fn(*args, **kw)
    st = h.stats()
    return out, [st["nlist"], st["ndis"], st["nheap_updates"]]


def check_forms(h, name, d, owner=True):
    """search_preassigned under every (fixed_rounds, filter, lanes), both selections on one form, and search() over the engine's own
    exact coarse ranking"""
    w = X.world(name, d)
    cd, ck = X.ranked(name, d)
    eD, eI, est = X.expected(name, d)
    for rounds in (1, 2):
        for flt in (0, 1, 2):
            for lanes in (0, 1):
                for select in ((0, 1) if (rounds, flt, lanes) == (2, 2, 1) else (1,)):
                    for key, v in (("fixed_rounds", rounds), ("filter", flt), ("lanes", lanes), ("select", select)):
                        h.set_option(key, v)
                    tag = f"{name} d={d} rounds={rounds} filter={flt} lanes={lanes} select={select}"
                    (D, I), st = searched(h, h.search_preassigned, w["xq"], X.K, ck, cd)
                    same((D, I), (eD, eI), tag)
                    assert st == list(est), (tag, st, list(est))
                    if rounds == 2 and flt != 0:
                        assert h.last_filter()[0] >= 1, tag  # (the filter ran: no call leaves it)
                    if flt == 2 and owner:
                        dg = h.layout_digest()
                        assert dg[4] == 0 and dg[5] != 0, tag  # (the fp16 copy is refused, the fp32 copy serves)
    for key in ("fixed_rounds", "filter", "lanes", "select"):
        h.set_option(key, None)
    (D, I), st = searched(h, h.search, w["xq"], X.K, X.NPROBE, coarse_mode=0)
    same((D, I), (eD, eI), f"{name} d={d} search")
    assert st == list(est), (name, d, "search", st, list(est))


@pytest.mark.parametrize("name,d", CASES)
def test_search_forms(capi, name, d):
    h = new_handle(capi, X.world(name, d))
    check_forms(h, name, d)
    h.close()


@pytest.mark.parametrize("name,d", CASES)
def test_exact_calls(capi, oracle, name, d):
    """search_exact, search_exact_selected (id % 3 == 0) and range_search_exact equal the oracle over every list, or over the subset;
    with option "exact_float" (d <= 128) / "exact_wide" (d = 200) set, the fp16 list pass is refused and every query goes the general
    way: a search over every list through the same threshold rounds"""
    w = X.world(name, d)
    h = new_handle(capi, w)
    h.set_option("exact_float" if d <= 128 else "exact_wide", 1)
    eD, eI, _ = X.expected_exact(name, d)
    D, I = h.search_exact(w["xq"], X.K)
    last = h.last_exact()
    same((D, I), (eD, eI), (name, d, "exact"))
    assert last[0] == 0 and last[1] + last[2] == X.NQ, last
    sD, sI, _ = X.expected_exact(name, d, selected=True)
    with h.selector(capi.SUBSET_ID_MOD, 3, 0) as s:
        D, I = h.search_exact_selected(s, w["xq"], X.K)
        last = h.last_exact()
    same((D, I), (sD, sI), (name, d, "exact selected"))
    assert last[0] == 0 and last[1] + last[2] == X.NQ, last
    radius = X.exact_radius(name, d)
    elims, elab, edis, _ = oracle.range_search_preassigned(X.oracle_lists(w), w["xq"], radius, X.identity_keys(X.NQ))
    assert 0 < elims[-1] < X.NQ * X.NB
    lims, lab, dis = h.range_search_exact(w["xq"], radius)
    assert np.array_equal(lims, elims) and np.array_equal(lab, elab), (name, d, "range")
    assert np.array_equal(bits(dis), bits(edis)), (name, d, "range")
    h.close()


@pytest.mark.parametrize("name", ["nonfinite_l2", "nonfinite_ip"])
@pytest.mark.parametrize("d", X.DS)
def test_clean_queries_after_the_nonfinite_ones(capi, name, d):
    """the handle that has just served the NaN and the infinite query serves the clean queries alone: nothing is left behind in
    thresholds, masks or survivor lists"""
    w = X.world(name, d)
    cd, ck = X.ranked(name, d)
    h = new_handle(capi, w)
    for flt in (2, 1):
        h.set_option("filter", flt)
        h.set_option("fixed_rounds", 2)
        same(h.search_preassigned(w["xq"], X.K, ck, cd), X.expected(name, d)[:2], (name, d, flt, "all"))
        eD, eI, est = X.expected(name, d, queries="clean")
        (D, I), st = searched(h, h.search_preassigned, w["xq"][w["clean"]], X.K, ck[w["clean"]], cd[w["clean"]])
        same((D, I), (eD, eI), (name, d, flt, "clean"))
        assert st == list(est) and h.last_filter()[0] >= 1
    h.close()


def test_a_clone_serves_the_same(capi):
    name, d = "l2_norm_overflow", 128
    h = new_handle(capi, X.world(name, d))
    c = h.clone()
    check_forms(c, name, d, owner=False)
    c.close()
    h.close()
