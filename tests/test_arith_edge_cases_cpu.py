"""The premise of tests/test_gpu_arith_edges.py, without a GPU: the cases of tests/arith_edge_cases.py are what they claim to be.

  * the unfused model is the pinned oracle, bit for bit, on every pair of every case (d = 30 and d = 100 % 8 != 0 included: the
    zero-padded tail adds nothing) -- this pins the model;
  * inside the rule the fused model is the oracle too, on every pair;
  * on every teeth case the fused model differs from the oracle on pairs the oracle's search_preassigned RETURNS at the k and the
    call the GPU test uses, and in the coarse-side cases on coarse distances among the oracle's nprobe best -- a condition on the
    inputs (a case that missed it would be drawn again), which is why a wrongly fused call cannot pass the GPU test;
  * the expected arithmetic of every case follows from the rule as arith_edge_cases.rule_arith restates it.

Observed (the tests print these): the share of all (query, row) pairs on which the fused model differs, and the returned pairs
among them for the 300-query call at k = 1 / 10 / 100 (70-query call in brackets; then under the oracle's own ranking, k = 10):
    l2_list_4097     d 16   all pairs 11.2 %   returned   7 / 193 / 2599   [2, 50, 664]     own ranking 48, 165
    l2_query_4097    d 128  all pairs  8.1 %   returned  26 / 227 / 1975   [7, 50, 454]     own ranking 49, 221
    l2_joint_4097    d 30   all pairs  5.1 %   returned   5 /  88 / 1053   [1, 15, 224]     own ranking 15, 94
    l2_centred_4097  d 100  all pairs 16.8 %   returned  41 / 519 / 4743   [11, 150, 1125]  own ranking 101, 458
    ip_4097          d 16   all pairs 45.6 %   returned  60 / 777 / 9644   [12, 175, 2154]  own ranking 182, 726
    coarse_in        d 128  all pairs  8.0 %   returned  30 / 208 / 1980   [6, 48, 441]     own ranking 42, 185
    coarse_out       d 16   coarse distances 10.4 % of 2400, 103 of the 1200 ranked ones (29 of the 70-query call's)
    coarse_out_ip    d 100  coarse distances 60.5 % of 2400, 730 of the 1200 ranked ones (173 of the 70-query call's)
    handle life      the widening row differs on 9 returned pairs once added to list 1, 8 once it overwrites an entry of list 2
    resident rows    the last row differs on 8.6 % of its pairs
Where the same range is drawn on both sides the share is above 10 %, as when the gap was first measured (15 - 22 %); a range widened
on one side only meets |t| = 4097 in half as many coordinates and shows 5 - 11 %.  A single 0.5 (l2_half_list, l2_half_query) has
no teeth at these magnitudes -- its quarter is lost in either rounding -- and is a case of the rule alone."""
import numpy as np
import pytest

import arith_edge_cases as E
from arith_edge_cases import bits


@pytest.fixture(scope="module")
def tables(oracle):
    """name -> (oracle table, unfused model, fused model), computed once a case"""
    memo = {}

    def get(name):
        if name not in memo:
            c = E.case(name)
            memo[name] = (E.oracle_table(c["metric"], c["xq"], c["xb"]), E.model_dist(c["metric"], c["xq"], c["xb"], False),
                          E.model_dist(c["metric"], c["xq"], c["xb"], True))
        return memo[name]
    return get


def probed(c, nq):
    hit = np.zeros((nq, E.NLIST), bool)
    q, p = np.nonzero(c["keys"][:nq] >= 0)
    hit[q, c["keys"][:nq][q, p]] = True
    return hit[:, c["assign"]]


@pytest.mark.parametrize("name", E.NAMES)
def test_shapes_and_extremes(name):
    c = E.case(name)
    assert c["d"] in (16, 30, 100, 128) and c["nlist"] == 8
    assert sorted(np.bincount(c["assign"], minlength=8)) == sorted(E.LENGTHS)
    assert [int((c["assign"] == l).sum()) for l in range(8)] == list(E.LENGTHS)
    # the sides reach their ranges (pokes aside), in every call, and about half of the coordinates are extremes
    for nq in E.CALLS:
        assert c["xq"][:nq].min() <= c["q_range"][0] and c["xq"][:nq].max() >= c["q_range"][1]
    assert c["xb"].min() <= c["b_range"][0] and c["xb"].max() >= c["b_range"][1]
    at = np.isin(c["xb"], c["b_range"])
    assert 0.45 < at.mean() < 0.62
    # the joint extreme is summed in a probed pair of the smallest call: query 0 against the row of list 1
    row = E.row_of(c["assign"], 1, 0)
    assert probed(c, 3)[0, row]
    lo, hi = min(c["q_range"][0], c["b_range"][0]), max(c["q_range"][1], c["b_range"][1])
    if c["metric"] == E.L2:
        assert np.abs(c["xq"][0] - c["xb"][row]).max() == hi - lo
    else:
        prod = c["xq"][0].astype(np.float64) * c["xb"][row]
        qm, bm = np.abs(c["q_range"]).max(), np.abs(c["b_range"]).max()
        assert np.abs(prod).max() == float(qm) * float(bm)
    if name in E.INSIDE:
        assert (hi - lo == E.EDGE) if c["metric"] == E.L2 else (max(-lo, hi) == E.MAG)
    if name == "l2_sym_negzero":
        assert all(np.signbit(a[a == 0]).any() for a in (c["xb"], c["xq"], c["cen"]))


@pytest.mark.parametrize("name", E.NAMES)
def test_expected_arith_follows_from_the_rule(name):
    c = E.case(name)
    for nq in E.CALLS:
        assert E.rule_arith(c["metric"], c["d"], c["xb"], c["xq"][:nq]) == c["arith"], nq
    coarse = E.rule_fused(c["metric"], c["d"], c["cen"], c["xq"])
    if c["coarse_teeth"]:
        assert not coarse and c["arith"] == 1   # the scan is fused, the coarse ranking is not
    if name == "coarse_in":
        assert coarse and c["arith"] == 0       # ... and the other way round
    # the halves: either side alone is far inside, only the pair reaches the edge / passes it
    if name in ("l2_halves", "l2_joint_4097"):
        assert np.ptp(c["xb"]) <= 2049 and np.ptp(c["xq"]) <= 2048
    # one step: every outside case with a range (not a poke) passes the edge by exactly one
    if name.endswith("_4097") and c["metric"] == E.L2:
        both = np.concatenate([c["xb"].ravel(), c["xq"].ravel()])
        assert both.max() - both.min() == E.EDGE + 1


@pytest.mark.parametrize("name", E.NAMES)
def test_unfused_model_is_the_oracle(tables, name):
    want, unfused, _ = tables(name)
    assert np.array_equal(bits(unfused), bits(want))


@pytest.mark.parametrize("name", E.NAMES)
def test_coarse_model_is_the_oracle_and_rankings_have_no_ties(oracle, name):
    c = E.case(name)
    want = E.oracle_table(c["metric"], c["xq"], c["cen"])
    assert np.array_equal(bits(E.model_dist(c["metric"], c["xq"], c["cen"], False)), bits(want))
    if E.rule_fused(c["metric"], c["d"], c["cen"], c["xq"]):
        assert np.array_equal(bits(E.model_dist(c["metric"], c["xq"], c["cen"], True)), bits(want))
    # no two centroids at one distance from a query: the ranking does not hang on a tie rule
    assert (np.diff(np.sort(want, axis=1), axis=1) != 0).all()


@pytest.mark.parametrize("name", [n for n in E.NAMES if E.SPECS[n][6] >= 1])
def test_fused_model_is_the_oracle_inside_the_rule(tables, name):
    want, _, fused = tables(name)
    assert np.array_equal(bits(fused), bits(want))


@pytest.mark.parametrize("name", E.TEETH)
def test_fused_model_differs_on_returned_pairs(tables, name, capsys):
    """see the module docstring for the observed shares"""
    c = E.case(name)
    want, _, fused = tables(name)
    share = float((bits(fused) != bits(want)).mean())
    counts = {}
    for nq in E.CALLS[1:]:
        for k in E.KS:
            D, I, _ = E.expected(name, nq, k)
            counts[nq, k] = E.returned_pairs_that_differ(c, D, I, fused)
        cd, ck, D, I, _ = E.expected_ranked(name, nq, 10)
        counts[nq, "ranked"] = E.returned_pairs_that_differ(c, D, I, fused)
    with capsys.disabled():
        print(f"\n    {name:16s} d {c['d']:<4d} all pairs {100 * share:4.1f} %   returned "
              + " / ".join(f"{counts[300, k]:4d}" for k in E.KS) + f"   (70 queries: {[counts[70, k] for k in E.KS]}, own ranking: "
              f"{counts[70, 'ranked']}, {counts[300, 'ranked']})")
    assert all(v >= 1 for v in counts.values()), counts
    # the share the same draw on both sides gave when the gap was first measured (15 - 22 %); a range widened on one side only meets
    # |t| = 4097 in half as many coordinates (query extreme against list extreme: 1/16 of them, not 1/8)
    assert share > (0.10 if c["q_range"] == c["b_range"] else 0.05)


@pytest.mark.parametrize("name", E.NAMES)
def test_range_radius_sits_on_a_teeth_pair(name):
    """the radius of the GPU range searches: on teeth cases the fused model's membership differs from the oracle's at it"""
    c = E.case(name)
    want, fused = E.model_tables(name, 70)
    is_l2 = c["metric"] == E.L2
    for keys in (c["keys"][:70], E.expected_ranked(name, 70, 10)[1]):
        radius, flips = E.flipping_radius(name, 70, keys)
        assert radius == float(np.float32(radius))
        pm = E.probed_mask(c["assign"], keys)
        inside, inside_fused = (want < radius if is_l2 else want > radius) & pm, (fused < radius if is_l2 else fused > radius) & pm
        assert 0 < inside.sum() < pm.sum()
        if c["teeth"]:
            assert flips and (inside != inside_fused).any()
        if c["arith"] >= 1:
            assert not flips and np.array_equal(inside, inside_fused)


@pytest.mark.parametrize("name", E.COARSE_TEETH)
def test_fused_model_differs_on_ranked_coarse_distances(name, capsys):
    c = E.case(name)
    want = E.oracle_table(c["metric"], c["xq"], c["cen"])
    fused = E.model_dist(c["metric"], c["xq"], c["cen"], True)
    differ = bits(fused) != bits(want)
    n_ranked = {}
    for nq in E.CALLS[1:]:
        cd, ck = E.expected_ranked(name, nq, 10)[:2]
        n_ranked[nq] = int(differ[np.arange(nq)[:, None], ck].sum())
    with capsys.disabled():
        print(f"\n    {name:16s} d {c['d']:<4d} coarse distances {100 * differ.mean():4.1f} % of {differ.size}, {n_ranked[300]} of the "
              f"{300 * E.NPROBE} ranked ones ({n_ranked[70]} of the 70-query call's)")
    assert all(v >= 1 for v in n_ranked.values()) and differ.mean() > 0.10


def test_handle_life_and_resident_rows_have_teeth(oracle, capsys):
    """the single widening row of the handle's-life test, and the last resident row: alone they take the pair out of the rule, and
    the fused model differs from the oracle on returned pairs that hold them"""
    c, f = E.case(E.LIFE_CASE), E.life()
    assert E.rule_arith(E.L2, c["d"], c["xb"], c["xq"]) == 1
    assert E.rule_arith(E.L2, c["d"], f["xb_add"], c["xq"]) == 0 and E.rule_arith(E.L2, c["d"], f["xb_upd"], c["xq"]) == 0
    assert np.ptp(np.concatenate([f["xb_add"].ravel(), c["xq"].ravel()])) == E.EDGE + 1
    want = E.oracle_table(E.L2, c["xq"], f["w"])
    assert np.array_equal(bits(E.model_dist(E.L2, c["xq"], f["w"], False)), bits(want))
    differ = (bits(E.model_dist(E.L2, c["xq"], f["w"], True)) != bits(want))[:, 0]
    n = {}
    for state, wid in (("added", E.LIFE_ID), ("updated", f["over"])):
        D, I, _ = E.life_expected(state)
        assert not (E.life_expected("base")[1] == wid).any() or state == "updated"
        q = np.nonzero((I == wid).any(axis=1))[0]
        n[state] = int(differ[q].sum())
        # ... and the oracle's value for those pairs is the table's
        assert np.array_equal(bits(D[I == wid]), bits(want[q, 0]))
    x = E.resident_rows()
    assert E.rule_arith(E.L2, c["d"], c["xb"], x) == 0 and E.rule_arith(E.L2, c["d"], c["xb"], x[:-1]) == 1
    last = E.oracle_table(E.L2, x[-1:], c["xb"])
    share = float((bits(E.model_dist(E.L2, x[-1:], c["xb"], True)) != bits(last)).mean())
    with capsys.disabled():
        print(f"\n    handle life: the widening row differs on {n['added']} returned pairs once added, {n['updated']} once it overwrites an "
              f"entry; the last resident row on {100 * share:.1f} % of its pairs")
    assert n["added"] >= 1 and n["updated"] >= 1 and share > 0.05  # (one side widened, as above)
