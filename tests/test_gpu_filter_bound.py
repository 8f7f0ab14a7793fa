"""The error bound that the list-side fp16 kernels drop candidates by -- exact_float_constant(d, false) = (2 d + 32) 2^-24 + 2^-10 +
2^-12 behind the keep rule of exact_args.h -- on data whose operands all round the same way (filter_bound_cases.py): the fp16 product
of a query with half of the stored rows is short by 0.5 .. 0.8 of 2^-10 |x| |y|, where Gaussian, clustered and one-ulp-copy data
reach a few per cent of it.  A kernel that read the fp32 form's constant, computed its own from a wrong d, or scaled the product by
a wrong power of two passes on those; here it drops true neighbours (test_filter_bound_cases_cpu.py holds, without a GPU, in how many
queries).  Every comparison is of bits or of counts taken from the reference:

  a. the exact float pass (scan_all_f16_kernel): (D, I) are the oracle's over all lists, and the pass's own counts are the
     reference's -- the queries it answers are those without a tie in their best k + 1 reference distances, and the candidates left
     after rescoring are exactly the stored entries whose reference distance is at or within the seed's k-th.  The counts matter: with
     the seed over every list the k-th neighbour lies ON the threshold, a dropped entry leaves fewer than k candidates and the query
     goes the general way, right again; with a mid seed the threshold lies a few ranks beyond and a dropped neighbour is a wrong result.
  b. the same under a selector that keeps every second id (the KEEP form of the pass), the counts over the members only.
  c. the fp16 filter of threshold rounds (scan_filter_kernel<.., HALF> at 4, 6 and 8 pieces, scan_filter_wide_kernel<.., HALF> and the
     one-wave form beyond 128 dimensions), list 0 holding three quarters of the rows as every query's first probe so that the later
     rounds' thresholds are near final; under both copies the filter can stream, as test_gpu_filter.py.
  d. one case of (c) under the selector (rescore_kernel<.., KEEP>).

What this data cannot see: a constant short by the 2^-12 term alone (filter_bound_cases.py)."""
import numpy as np
import pytest

import filter_bound_cases as fb

pytestmark = pytest.mark.gpu

N, K, NLIST = fb.N, fb.K, fb.NLIST


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


@pytest.fixture(params=[2, 1], ids=["fp16", "fp32"])
def form(request, monkeypatch):
    monkeypatch.setenv("AUNCEL_AMD_FILTER", str(request.param))
    return request.param


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def identity_keys():
    return np.tile(np.arange(NLIST, dtype=np.int64), (N, 1))


def make_handle(capi, c):
    h = capi.Handle(c.d, NLIST, c.metric, 0)
    h.set_centroids(c.cen)
    h.set_lists_from_assign(c.xb, c.assign)
    return h


_REFERENCE = {}


def reference(oracle, key, c):
    """of the stored rows of `c` (a case, or its members under the selector), computed once per case: the oracle's lists, its (D, I)
    over every list, the queries with a tie in their best k + 1 distances, and the reference distance of every (query, entry) pair
    -- the oracle's own result at k = every entry, sorted"""
    if key not in _REFERENCE:
        lists = oracle.Lists(c.metric, c.cen, c.xb, c.assign, c.ids)
        keys, zeros = identity_keys(), np.zeros((N, NLIST), np.float32)
        all_D, _, _ = oracle.search_preassigned(lists, c.xq, len(c.xb), keys, zeros)
        eD, eI, _ = oracle.search_preassigned(lists, c.xq, K, keys, zeros)
        assert np.array_equal(bits(all_D[:, :K]), bits(eD))
        b = bits(all_D[:, :K + 1])
        tied = (b[:, 1:] == b[:, :-1]).any(axis=1)
        for a in (all_D, eD, eI, tied):
            a.setflags(write=False)
        _REFERENCE.clear()  # (the tests of a case follow each other: one case's n x nb distances are kept)
        _REFERENCE[key] = (lists, eD, eI, int(tied.sum()), all_D)
    return _REFERENCE[key]


def check_exact_call(oracle, h, c, ref, depth, D, I, what):
    """(D, I) and the counts of the exact call `h` has just answered, against the reference at the seed depth the call used"""
    lists, eD, eI, ties, all_D = ref
    last, det = h.last_exact(), h.last_exact_detail()
    cd, ck = oracle.knn(c.metric, c.xq, c.cen, depth)
    sD, sI, _ = oracle.search_preassigned(lists, c.xq, K, ck, cd)
    assert (sI[:, K - 1] >= 0).all()
    valid = int(fb.within(c.metric, all_D, sD[:, K - 1]).sum())
    bad = np.nonzero((I != eI).any(axis=1) | (bits(D) != bits(eD)).any(axis=1))[0]
    print(what, "seed depth", depth, "last_exact", last, "detail", det, "reference: ties", ties, "valid", valid, "wrong queries", bad.size)
    assert bad.size == 0, (what, "queries", bad[:8], I[bad[0]], eI[bad[0]])
    assert det[0] == 2, "the call did not take the fp16 pass"
    assert last[2] == 0, "queries left the pass for another reason than a tie: candidates were dropped"
    assert last[0] == N - ties and last[1] == ties
    assert det[2] == valid, "the candidates at or within the threshold are not the reference's"
    assert det[1] >= det[2] and det[1] == last[3]
    assert det[3] <= fb.CAP // 4  # (no case passes by overflowing the slots)


# ------------------------------------------------------------------------------------------ a. the exact float pass
@pytest.mark.parametrize("depth", ["tight", "mid"])
@pytest.mark.parametrize("metric,d,W,mid,seed", fb.EXACT_CASES)
def test_exact_float_pass_keeps_every_entry_within_the_threshold(capi, oracle, metric, d, W, mid, seed, depth):
    c = fb.case(metric, d, W, seed=seed)
    ref = reference(oracle, ("all", metric, d, W, seed), c)
    s = fb.TIGHT if depth == "tight" else mid
    h = make_handle(capi, c)
    h.set_option("exact_float", 1)
    h.set_option("exact_seed_nprobe", s)
    D, I = h.search_exact(c.xq, K)
    check_exact_call(oracle, h, c, ref, s, D, I, (metric, d, W, depth))
    h.close()


# ------------------------------------------------------------------------------------------ b. ... under a selector
@pytest.mark.parametrize("option", fb.SELECTED_OPTION)
@pytest.mark.parametrize("metric,d,W,seed", fb.SELECTED_CASES)
def test_exact_float_pass_under_a_selector(capi, oracle, metric, d, W, seed, option):
    c = fb.case(metric, d, W, seed=seed)
    m = fb.every_second(c)
    ref = reference(oracle, ("members", metric, d, W, seed), m)
    h = make_handle(capi, c)
    h.set_option("exact_float", 1)
    h.set_option("exact_seed_nprobe", option)
    with h.selector(capi.SUBSET_ID_MOD, 2, 1, None) as s:
        assert s.info()[1] == len(m.xb)
        D, I = h.search_exact_selected(s, c.xq, K)
        check_exact_call(oracle, h, m, ref, fb.selected_depth(option), D, I, (metric, d, W, "selected", option))
    h.close()


# ------------------------------------------------------------------------------------------ c. the filter in threshold rounds
def run_dense_first(capi, oracle, metric, d):
    c = fb.case(metric, d, fb.spread(metric), "dense")
    lists = oracle.Lists(metric, c.cen, c.xb, c.assign)
    keys, zeros = identity_keys(), np.zeros((N, NLIST), np.float32)  # list 0, the dense one, first
    eD, eI, est = oracle.search_preassigned(lists, c.xq, K, keys, zeros)
    h = make_handle(capi, c)
    h.stats(reset=True)
    D, I = h.search_preassigned(c.xq, K, keys, zeros)
    launches, kept = h.last_filter()
    st = h.stats()
    bad = np.nonzero((I != eI).any(axis=1) | (bits(D) != bits(eD)).any(axis=1))[0]
    print("dense first", metric, d, "filter launches", launches, "kept", kept, "wrong queries", bad.size)
    assert launches >= 1, "the search did not go through the filter"
    assert np.array_equal(I, eI), ("queries", bad[:8])
    assert np.array_equal(bits(D), bits(eD))
    assert [st["nlist"], st["ndis"], st["nheap_updates"]] == list(est)
    h.close()


@pytest.mark.parametrize("metric", [fb.L2, fb.IP])
@pytest.mark.parametrize("d", fb.FILTER_D)
def test_filter_rounds_keep_every_neighbour(capi, oracle, form, d, metric):
    run_dense_first(capi, oracle, metric, d)


@pytest.mark.parametrize("metric", [fb.L2, fb.IP])
@pytest.mark.parametrize("d", fb.NARROW_D)
def test_filter_rounds_in_the_one_wave_form(capi, oracle, form, monkeypatch, d, metric):
    monkeypatch.setenv("AUNCEL_AMD_FILTER_NARROW", "1")
    run_dense_first(capi, oracle, metric, d)


# ------------------------------------------------------------------------------------------ d. ... under a selector
def test_filter_rounds_under_a_selector(capi, oracle, form):
    metric, d = fb.FILTER_SELECTED
    c = fb.case(metric, d, fb.spread(metric), "dense")
    m = fb.every_second(c)
    keys, zeros = identity_keys(), np.zeros((N, NLIST), np.float32)
    _, _, pst = oracle.search_preassigned(oracle.Lists(metric, c.cen, c.xb, c.assign), c.xq, K, keys, zeros)
    eD, eI, est = oracle.search_preassigned(oracle.Lists(metric, m.cen, m.xb, m.assign, m.ids), c.xq, K, keys, zeros)
    h = make_handle(capi, c)
    with h.selector(capi.SUBSET_ID_MOD, 2, 1, None) as s:
        assert s.info()[1] == len(m.xb)
        h.stats(reset=True)
        D, I = h.search_preassigned_selected(s, c.xq, K, keys, zeros)
        launches, kept = h.last_filter()
        st = h.stats()
    bad = np.nonzero((I != eI).any(axis=1) | (bits(D) != bits(eD)).any(axis=1))[0]
    print("dense first, selected", "filter launches", launches, "kept", kept, "wrong queries", bad.size)
    assert launches >= 1, "the search did not go through the filter"
    assert np.array_equal(I, eI), ("queries", bad[:8])
    assert np.array_equal(bits(D), bits(eD))
    assert st["nheap_updates"] == est[2] and st["ndis"] == pst[1], (st, est, pst)
    h.close()
