"""What test_gpu_adaptive_filter.py requires of its data (adaptive_filter_cases.py), asserted from the oracle and the numpy model alone:
the oracle's stop points are where the round floors need them, the schedule model says what it should, inner-product lists hold K
vectors, and on the coherently rounded rows the fp16 constant keeps every entry a round's threshold admits while the fp32 form's
constant loses one for most queries.  The floors are conditions on the data: a case that misses one gets another seed."""
import numpy as np
import pytest

import adaptive_filter_cases as ac


@pytest.fixture(scope="module")
def arcos(oracle):
    return oracle.arcos_table()


def test_schedule_model():
    sizes = np.full(64, 94)
    assert ac.default_first(20, sizes) == 15 and ac.default_first(20, np.full(64, 2000)) == 1 and ac.default_first(128, np.full(8, 10)) == 16
    assert ac.stages("one_probe", 20, sizes, 64)[:9] == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert ac.stages("three_two", 20, sizes, 64) == [3, 6, 12, 24, 48, 64]
    assert ac.stages("one_round", 20, sizes, 64) == [64]
    assert ac.stages("default", 20, sizes, 64) == [15, 64]  # (15 -> max(16, 90, 27), cut at nlist)
    np8 = np.array([1, 3, 8])
    assert [ac.rounds_floor(s, 20, sizes, 64, np8) for s in ("default", "one_probe", "three_two", "one_round")] == [1, 8, 3, 1]
    assert ac.rounds_floor("one_probe", 20, sizes, 64, np.array([1, 1])) == 1
    # under the default rule these shapes scan more probes densely than a query can run: no filter round without the override
    c = ac.form_case(64, 0)
    assert ac.default_first(c.K, c.sizes) > c.nlist // 8
    assert ac.ntraces(64) == 4 and ac.ntraces(256) == 6


@pytest.mark.parametrize("d", ac.FORM_D)
def test_form_cases_reach_the_last_stage(oracle, arcos, d):
    assert set(ac.FORM_NARROW_D) <= set(ac.FORM_D)
    for layout, (nq, few) in enumerate(ac.FORM_LAYOUTS):
        c = ac.form_case(d, layout)
        assert c.sizes[1] == 0 and c.sizes[0] > 1.5 * c.sizes[2:].mean() and len(c.xb) == ac.FORM_NB
        ck = oracle.knn(c.metric, c.xq, c.cen, 1)[1][:, 0]
        per_list = np.bincount(ck, minlength=c.nlist).max()
        assert nq / few * 0.7 <= per_list <= 128 + 40, (nq, few, per_list)  # (~ 19, ~ 37, ~ 130 queries on a list)
        for qk in (1, 10):
            p = ac.reference(oracle, arcos, ("form", d, layout), c, qk).my_nprobe
            print(d, layout, qk, np.bincount(p).tolist())
            assert p.max() == c.nlist // 8
            if qk == 10:
                assert len(np.unique(p)) >= 4 and p.min() == 1  # (queries leave in several different rounds)


@pytest.mark.parametrize("metric", [ac.L2, ac.IP])
def test_schedule_cases(oracle, arcos, metric):
    c = ac.schedule_case(metric)
    p = ac.reference(oracle, arcos, ("schedule", metric), c, 10).my_nprobe
    floors = {s: ac.rounds_floor(s, c.K, c.sizes, c.nlist, p) for s in ac.SCHEDULES}
    print(metric, np.bincount(p).tolist(), floors)
    assert floors["one_probe"] >= 8 and floors["three_two"] == 3 and floors["one_round"] == 1
    assert c.sizes.min() >= c.K


@pytest.mark.parametrize("profile", [False, True])
def test_mixed_case_spans_the_stages(oracle, arcos, profile):
    c = ac.mixed_case()
    assert c.req.min() == np.float32(0.5) and c.req.max() == np.float32(0.99) and len(np.unique(c.req)) > 100
    ref = ac.reference(oracle, arcos, "mixed", c, 10, profile)
    p = ref.my_nprobe
    print(np.bincount(p).tolist())
    assert p.min() == 1 and p.max() == c.nlist // 8 and len(np.unique(p)) >= 5
    assert np.bincount(p)[[1, 2, 3, 5, 8]].min() >= 20  # (every one of those rounds loses a real share of the queries)
    if profile:
        assert len(np.unique(ref.t_recalls)) > 3


@pytest.mark.parametrize("d", ac.COPIES_D)
def test_copies_cases_meet_ties_in_later_rounds(oracle, arcos, d):
    c = ac.copies_case(d)
    ref = ac.reference(oracle, arcos, ("copies", d), c, ac.COPIES_K)
    assert (ref.my_nprobe == c.nlist // 8).all()
    # equal and nearly equal distances among a query's results: the copies did meet in its heap
    b = ac.cp.bits(ref.D)
    assert ((b[:, 1:] == b[:, :-1]).any(axis=1)).mean() > 0.9
    # ... and candidates of probes 1 .. 7 lie on the threshold the probes before left: a stored row equal to a result row, in a later list
    lists = oracle.Lists(c.metric, c.cen, c.xb, c.assign)
    on = 0
    for r in range(1, c.nlist // 8):
        D, _, _ = oracle.search_preassigned(lists, c.xq, c.K, ref.ck[:, :r], ref.cd[:, :r])
        nxt, _, _ = oracle.search_preassigned(lists, c.xq, len(c.xb), ref.ck[:, r:r + 1], ref.cd[:, r:r + 1])
        tau = D[:, c.K - 1:c.K]
        on += int(((nxt == tau) | (nxt == np.nextafter(tau, np.float32(0))) | (nxt == np.nextafter(tau, np.float32(np.inf)))).any(axis=1).sum())
    print(d, "(query, round) pairs with a candidate on or one ulp from the threshold", on)
    assert on >= 20


@pytest.mark.parametrize("d", ac.BOUND_D)
def test_bound_cases_sit_at_the_edge_of_the_bound(oracle, arcos, d):
    c = ac.bound_case(d)
    for m in (c.xq, c.xb):
        assert ac.cp.half_scale(m) == 2.0 ** 14 and not ac.cp.held_exactly(m)
    assert c.sizes.min() > 0
    ref = ac.reference(oracle, arcos, ("bound", d), c, ac.BOUND_K)
    assert (ref.my_nprobe == c.nlist // 8).all()
    lost_real, fp32_loses, rounds = ac.bound_report(oracle, c, ref)
    print(d, "real constant drops", lost_real, "fp32 constant: queries that lose", fp32_loses, "rounds", rounds)
    assert lost_real == 0
    assert fp32_loses >= ac.BOUND_FP32_LOSES
    assert rounds == list(range(1, c.nlist // 8))  # (every filter round of the call, the last included)


@pytest.mark.parametrize("d,K", ac.IP_CASES)
def test_inner_product_lists_hold_k_vectors(oracle, arcos, d, K):
    c = ac.ip_case(d, K)
    assert c.sizes.min() >= K
    assert np.allclose(np.linalg.norm(c.xb, axis=1), 0.9, atol=1e-5)
    for qk in (1, K):
        p = ac.reference(oracle, arcos, ("ip", d, K), c, qk).my_nprobe
        print(d, K, qk, np.bincount(p).tolist())
        assert p.max() >= (8 if qk == 1 or K == 10 else 5)


def test_the_short_list_raises_in_the_oracle(oracle, arcos):
    c = ac.ip_case(64, 10, True)
    assert c.sizes[7] == 9 and np.delete(c.sizes, 7).min() >= 10
    assert oracle.knn(c.metric, c.xq[:1], c.cen, 1)[1][0, 0] == 7  # (query 0 meets it first)
    with pytest.raises(RuntimeError):
        ac.reference(oracle, arcos, "ip short", c, 10)


def test_entry_and_scale_cases(oracle, arcos):
    c = ac.entry_case()
    p = ac.reference(oracle, arcos, "entry", c, 10, True).my_nprobe
    cut = len(p) // 2 + 3
    assert p[:cut].max() == 8 and p[cut:].max() == 8
    s = ac.scale_case()
    assert ac.cp.half_scale(s.xq) == 0.0 and ac.cp.half_scale(s.xb) > 0
    ref = ac.reference(oracle, arcos, "scale", s, 10)
    assert (ref.my_nprobe == 8).all() and np.isfinite(ref.D).all()
