"""Preconditions of test_gpu_select_forms.py, asserted through the oracle alone (no GPU): the worlds of select_form_cases.py put equal
distances where the selection forms differ, the adaptive cases raise nothing and stop at different probes, the selector leaves what
the tests say it leaves.  A world that stopped doing so would let the GPU tests pass for nothing."""
import numpy as np
import pytest

import select_form_cases as sc
from select_form_cases import A_CASES, A_IP_CASE, A_N, K_FIXED, NLIST, NQ


@pytest.fixture(scope="module", autouse=True)
def built(oracle):
    return oracle


def test_lists_are_ragged_and_queries_fill_two_blocks_unevenly():
    assert sc.SIZES[0] == 0 and 0 < sc.SIZES[1] < 64 and sum(sc.SIZES) == sc.NB
    assert NQ > 64 and NQ % 4 == 2  # two query blocks; the last workgroup of four waves is half full
    for name in sc.DIMS:
        for metric in (1, 0):
            w = sc.world(name, metric)
            assert np.array_equal(np.bincount(w["assign"], minlength=NLIST), sc.SIZES)
            assert w["keys"].shape == (NQ, sc.NPROBE) and (w["keys"] >= 0).all()
            # every k of K_FIXED has a (k + 1)-th candidate with every query: no k is left out of the tie condition for lack of one
            assert min(len(c) for c in sc.candidates(name, metric)) > max(K_FIXED)
            # some query probes the empty list, some the short one
            assert (w["keys"] == 0).any() and (w["keys"] == 1).any()


@pytest.mark.parametrize("metric", [1, 0])
def test_ties_world_has_a_tie_across_the_edge_of_every_heap(metric):
    """at least half of the queries have their k-th and (k + 1)-th best candidate distances bit-equal.  No k of K_FIXED is left out:
    every query has more than 161 candidates, and the condition holds at all sixteen (at most 2 may miss it)"""
    held = sc.held_to_tie_condition(metric)
    for k in K_FIXED:
        have, tied = sc.edge_tie_counts("ties", metric, k)
        assert have == NQ, k
        print("ties", metric, "k", k, "edge ties", tied, "split / need replay / need it for the split alone", sc.replay_counts("ties", metric, k))
    assert len(K_FIXED) - len(held) <= 2, held
    assert held == K_FIXED  # (what the world gives today; the GPU test reads `held`)


@pytest.mark.parametrize("metric", [1, 0])
def test_ties_world_splits_edge_ties_and_some_need_the_replay_for_that_alone(metric):
    """the admissions split an edge tie (a value equal to the new worst was evicted) at every k > 1, and at k = 2 and 3 some queries'
    final k values are all different, so that only the `amb` note sends them through the replay; k = 1 can split nothing"""
    assert sc.replay_counts("ties", metric, 1) == (0, 0, 0)
    for k in K_FIXED[1:]:
        split, need, alone = sc.replay_counts("ties", metric, k)
        assert split >= 10 and need >= split, (k, split, need)
    assert sc.replay_counts("ties", metric, 2)[2] >= 10 and sc.replay_counts("ties", metric, 3)[2] >= 1


@pytest.mark.parametrize("metric", [1, 0])
def test_distinct_world_has_no_equal_candidate_distances(metric):
    for q, c in enumerate(sc.candidates("distinct", metric)):
        assert len(np.unique(c.view(np.uint32))) == len(c), q
    for k in K_FIXED:
        assert sc.replay_counts("distinct", metric, k) == (0, 0, 0), k
        assert sc.edge_tie_counts("distinct", metric, k) == (NQ, 0), k


@pytest.mark.parametrize("metric", [1, 0])
def test_selector_keeps_two_fifths_of_every_list_but_one(metric):
    w, m = sc.world("ties", metric), sc.members(metric)
    emptied = 0
    for l in range(NLIST):
        rows = w["assign"] == l
        if not rows.any():
            continue
        if not m[rows].any():
            emptied += 1
            continue
        assert 0.3 <= m[rows].mean() <= 0.5, l
    assert emptied >= 1 and 0.35 < m.mean() < 0.45
    # the members-only results differ from the parent's, and from the complement's
    for k in sc.SELECTED_K:
        assert not np.array_equal(sc.expected("ties", metric, k, selected=True)[1], sc.expected("ties", metric, k)[1]), k
    for k in sc.EACH_K:
        assert not np.array_equal(sc.expected("ties", metric, k, selected=True)[1], sc.expected("ties", metric, k, selected="complement")[1]), k


@pytest.mark.parametrize("variant", sc.A_VARIANTS)
def test_adaptive_cases_raise_nothing_and_stop_at_different_probes(variant):
    w = sc.adaptive_world(variant)
    assert w["xq"].shape == (A_N, sc.A_D) and set(np.unique(w["req"]).tolist()) == {np.float32(0.5), np.float32(0.9), np.float32(0.99)}
    for K, qk in A_CASES:
        my_np = sc.expected_adaptive(variant, K, qk)[3]  # (raises what the oracle raises)
        assert my_np.min() >= 1 and len(np.unique(my_np)) > 1, (K, qk)
        ties = sc.adaptive_edge_ties(variant, K, qk)
        print("adaptive", variant, K, qk, "nprobe", int(my_np.min()), int(my_np.max()), "edge ties", ties)
        if variant == "grid":
            assert 4 * ties >= A_N, (K, qk, ties)


def test_adaptive_inner_product_case_raises_nothing():
    w = sc.adaptive_world("unit")
    K, qk = A_IP_CASE
    assert np.bincount(w["assign"], minlength=sc.A_NLIST).min() >= K
    assert np.allclose(np.linalg.norm(w["xb"], axis=1), 0.9, atol=1e-5)
    my_np = sc.expected_adaptive("unit", K, qk)[3]
    assert len(np.unique(my_np)) > 1
