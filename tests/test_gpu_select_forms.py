"""Top-k selection at every form k chooses (ivf_select.hip: launch_select_sorted, launch_replay, launch_tie_fix), bit for bit against
the pinned oracle, over the small fixed worlds of select_form_cases.py (whose preconditions test_select_form_cases_cpu.py asserts):

  select_sorted_kernel  k <= 128: one register (KC = 10), two (KC = 100), two interleaved with k at run time (everything else:
                        2 and 3 -- entry 1 is the first in the second register --, 9, 11, 63 .. 65, 99, 101, 127, 128)
  replay_kernel         register heap k <= 127 ("select" 0), LDS heap at k = 128 under "select" 0 and always from 129 on
  tie_fix_kernel        register heap k <= 127, LDS heap at k = 128: the only sorted array with an LDS replay

in fixed-nprobe searches (test a), under a selector (d), under the stop rule (e) and with k going up and down on one handle (f).
Tests b, c and e read amd_ivf_last_tie_fixed: the replay runs for at least the queries that select_form_cases.replay_counts says
need it -- equal values among their final k, or an edge tie that the admissions split -- and for none where no two candidate
distances are equal.  The count asserted is the second of replay_counts' three, which is never below the first (the split edge
ties alone); at k = 2 and 3 it holds queries only the `amb` note of select_sorted_kernel can flag."""
import numpy as np
import pytest

import select_form_cases as sc
from select_form_cases import A_CASES, A_IP_CASE, A_N, K_FIXED, NQ
from test_gpu_subset import id_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


@pytest.fixture(scope="module")
def handles(capi, oracle):
    """one handle per (world, metric), opened at first use and kept for the module"""
    made = {}

    def get(name, metric):
        if (name, metric) not in made:
            w = sc.world(name, metric)
            h = capi.Handle(w["d"], sc.NLIST, metric, 0)
            h.set_centroids(w["cen"])
            h.set_lists_from_assign(w["xb"], w["assign"])
            made[(name, metric)] = h
        return made[(name, metric)]

    yield get
    for h in made.values():
        h.close()


@pytest.fixture(scope="module")
def adaptive_handles(capi, oracle):
    made = {}

    def get(variant):
        if variant not in made:
            w = sc.adaptive_world(variant)
            h = capi.Handle(w["d"], sc.A_NLIST, w["metric"], 0)
            h.set_centroids(w["cen"])
            h.set_lists_from_assign(w["xb"], w["assign"])
            h.set_interdis(None)
            h.set_queries(w["xq"])
            made[variant] = h
        return made[variant]

    yield get
    for h in made.values():
        h.close()


class options:
    """h.set_option for the block, back to unset behind it"""

    def __init__(self, h, **kv):
        self.h, self.kv = h, kv

    def __enter__(self):
        for key, value in self.kv.items():
            self.h.set_option(key, value)

    def __exit__(self, *exc):
        for key in self.kv:
            self.h.set_option(key, None)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, tag):
    D, I = got
    assert D.shape == want[0].shape and np.array_equal(I, want[1]), tag
    assert np.array_equal(bits(D), bits(want[0])), tag


def plain(h, w, k, tag, store_pairs=False):
    eD, eI, est = sc.expected(w["name"], w["metric"], k, store_pairs)
    h.stats(reset=True)
    got = h.search_preassigned(w["xq"], k, w["keys"], w["dis"], store_pairs=store_pairs)
    st = h.stats()
    same(got, (eD, eI), tag)
    assert [st["nlist"], st["ndis"], st["nheap_updates"]] == list(est), (tag, st, est)


# ---- a. fixed nprobe, every k ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("select", [1, 0])
@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("name", ["ties", "distinct"])
def test_every_k_equals_the_oracle(handles, name, metric, select):
    h, w = handles(name, metric), sc.world(name, metric)
    for rounds in (1, 2):
        with options(h, select=select, fixed_rounds=rounds):
            for k in K_FIXED:
                for pairs in (False, True):
                    plain(h, w, k, f"{name} metric={metric} select={select} rounds={rounds} k={k} pairs={pairs}", pairs)


# ---- b. the replay runs where it must, and only there -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [1, 0])
def test_tie_replay_runs_for_the_queries_that_need_it(handles, metric):
    h, w = handles("ties", metric), sc.world("ties", metric)
    held = [k for k in sc.held_to_tie_condition(metric) if k <= 128]
    assert len(held) >= 12
    for rounds in (1, 2):
        with options(h, select=1, fixed_rounds=rounds):
            for k in held:
                tag = f"ties metric={metric} rounds={rounds} k={k}"
                plain(h, w, k, tag)
                split, need, alone = sc.replay_counts("ties", metric, k)
                fixed = h.last_tie_fixed()
                print("[select forms]", tag, "replayed", fixed, "split / need / for the split alone", (split, need, alone))
                assert need >= split and fixed >= need, (tag, fixed, split, need)
                assert fixed <= NQ, tag


@pytest.mark.parametrize("metric", [1, 0])
def test_tie_replay_does_not_run_without_equal_distances(handles, metric):
    h, w = handles("distinct", metric), sc.world("distinct", metric)
    for rounds in (1, 2):
        with options(h, select=1, fixed_rounds=rounds):
            for k in K_FIXED:
                if k <= 128:
                    tag = f"distinct metric={metric} rounds={rounds} k={k}"
                    plain(h, w, k, tag)
                    assert h.last_tie_fixed() == 0, tag


# ---- c. the replay at the end of the search or behind every round --------------------------------------------------------------------
@pytest.mark.parametrize("tie_fix", [0, 1])
@pytest.mark.parametrize("metric", [1, 0])
def test_tie_fix_final_and_eager(handles, metric, tie_fix):
    h, w = handles("ties", metric), sc.world("ties", metric)
    for rounds in (1, 2):
        with options(h, select=1, tie_fix=tie_fix, fixed_rounds=rounds):
            for k in sc.TIE_FIX_K:
                tag = f"ties metric={metric} tie_fix={tie_fix} rounds={rounds} k={k}"
                plain(h, w, k, tag)
                assert h.last_tie_fixed() >= sc.replay_counts("ties", metric, k)[1], tag
                plain(h, w, k, tag + " pairs", store_pairs=True)


# ---- d. under a selector --------------------------------------------------------------------------------------------------------------
def _selectors(capi, h, metric):
    m = sc.members(metric)
    nwords = (len(m) + 63) // 64 + 2
    return [h.selector(capi.SUBSET_ID_BITS, 0, 0, id_bits(np.nonzero(x)[0], nwords)) for x in (m, ~m)]


@pytest.mark.parametrize("select", [1, 0])
@pytest.mark.parametrize("metric", [1, 0])
def test_selected_search_equals_the_members_only_oracle(capi, handles, metric, select):
    h, w = handles("ties", metric), sc.world("ties", metric)
    sels = _selectors(capi, h, metric)
    try:
        for rounds in (1, 2):
            with options(h, select=select, fixed_rounds=rounds):
                for k in sc.SELECTED_K:
                    tag = f"selected metric={metric} select={select} rounds={rounds} k={k}"
                    eD, eI, est = sc.expected("ties", metric, k, selected=True)
                    h.stats(reset=True)
                    got = h.search_preassigned_selected(sels[0], w["xq"], k, w["keys"], w["dis"])
                    st = h.stats()
                    same(got, (eD, eI), tag)
                    # (as tests/test_gpu_selector.py: the heap updates are the filtered lists', the distances computed the parent's)
                    assert st["nheap_updates"] == est[2] and st["ndis"] == sc.expected("ties", metric, k)[2][1], (tag, st, est)
                    if rounds == 1:  # ... and ranked by the engine (the keys are the oracle's ranking of the same centroids)
                        same(h.search_selected(sels[0], w["xq"], k, sc.NPROBE), (eD, eI), tag + " ranked")
    finally:
        for s in sels:
            s.close()


@pytest.mark.parametrize("metric", [1, 0])
def test_selector_per_query_equals_the_single_selector_rows(capi, handles, metric):
    h, w = handles("ties", metric), sc.world("ties", metric)
    sels = _selectors(capi, h, metric)
    sel_of = (np.arange(NQ) % 3 == 1).astype(np.uint32)  # neighbours differ, and runs of two
    try:
        for select in (1, 0):
            with options(h, select=select):
                for k in sc.EACH_K:
                    tag = f"each metric={metric} select={select} k={k}"
                    single = [h.search_preassigned_selected(s, w["xq"], k, w["keys"], w["dis"]) for s in sels]
                    same(single[0], sc.expected("ties", metric, k, selected=True)[:2], tag)
                    same(single[1], sc.expected("ties", metric, k, selected="complement")[:2], tag + " complement")
                    D, I = h.search_preassigned_selected_each(sels, sel_of, w["xq"], k, w["keys"], w["dis"])
                    for q in range(NQ):
                        assert np.array_equal(I[q], single[sel_of[q]][1][q]), (tag, q)
                        assert np.array_equal(bits(D[q]), bits(single[sel_of[q]][0][q])), (tag, q)
    finally:
        for s in sels:
            s.close()


# ---- e. under the stop rule -------------------------------------------------------------------------------------------------------------
def adaptive(capi, h, variant, K, qk, tag):
    w = sc.adaptive_world(variant)
    eD, eI, est, e_np, e_rec, gtD = sc.expected_adaptive(variant, K, qk)
    my_np = np.zeros(A_N, dtype=np.uint64)
    t_rec = np.zeros(A_N, dtype=np.float32)
    h.stats(reset=True)
    D, I = h.search_adaptive(0, A_N, qk, sc.A_MULTIPLER, sc.A_STD_M, w["req"], my_np, t_rec, gt_D=gtD)
    st = h.stats()
    assert np.array_equal(my_np.astype(np.int64), e_np), tag
    same((D, I), (eD, eI), tag)
    assert np.array_equal(bits(t_rec), bits(e_rec)), tag
    assert [st["nlist"], st["ndis"], st["nheap_updates"]] == list(est), (tag, st, est)


@pytest.mark.parametrize("select", [1, 0])
@pytest.mark.parametrize("variant", sc.A_VARIANTS)
def test_adaptive_every_heap_form(capi, adaptive_handles, monkeypatch, variant, select):
    h, w = adaptive_handles(variant), sc.adaptive_world(variant)
    for K, qk in A_CASES:
        h.set_tuner(K, w["traces"], capi.arcos_table())
        for nld in ("16", "32"):
            monkeypatch.setenv("AUNCEL_AMD_REPLAY_NLD", nld)
            tag = f"adaptive {variant} select={select} K={K} query_topk={qk} nld={nld}"
            with options(h, select=select):
                adaptive(capi, h, variant, K, qk, tag)
                if variant == "grid" and select == 1 and K <= 128:
                    assert h.last_tie_fixed() >= 1, tag


@pytest.mark.parametrize("select", [1, 0])
def test_adaptive_inner_product(capi, adaptive_handles, select):
    h, w = adaptive_handles("unit"), sc.adaptive_world("unit")
    K, qk = A_IP_CASE
    h.set_tuner(K, w["traces"], capi.arcos_table())
    with options(h, select=select):
        adaptive(capi, h, "unit", K, qk, f"adaptive unit select={select} K={K} query_topk={qk}")


# ---- f. one handle, k going up and down ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("select", [1, 0])
@pytest.mark.parametrize("metric", [1, 0])
def test_k_up_and_down_on_one_handle(capi, oracle, metric, select):
    """the log, the `amb` array and the heap buffers are sized by the call: a fresh handle, so that every buffer's first size is
    k = 128's and each later call finds what a call of another stride left"""
    w = sc.world("ties", metric)
    h = capi.Handle(w["d"], sc.NLIST, metric, 0)
    h.set_centroids(w["cen"])
    h.set_lists_from_assign(w["xb"], w["assign"])
    try:
        with options(h, select=select, fixed_rounds=2):
            for rep in range(2):
                for k in sc.UP_AND_DOWN_K:
                    plain(h, w, k, f"up and down metric={metric} select={select} rep={rep} k={k}")
    finally:
        h.close()
