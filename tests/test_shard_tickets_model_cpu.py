"""The expectations of test_gpu_shard_tickets.py, checked on the CPU from the oracle and the goldens alone: the per-shard oracle
tables really are the reference's shards, and the inputs still have the edges the GPU tests are there for -- a redraw of a seed or
of a shape that made them easy fails here."""
import numpy as np
import pytest

import shard_ticket_cases as stc
from util import load_case


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", stc.GOLDEN_SHARD_CASES)
def test_oracle_shard_tables_merge_to_the_golden_shards(oracle, name):
    case, gold = load_case(name)
    nshard = int(case["nshard"])
    assert nshard >= 2
    tabs = stc.golden_shard_tables(name)
    for k in case["ks"]:
        k = int(k)
        D, I = oracle.merge_tables(case["metric"], np.stack([t[0] for t in tabs[k]]), np.stack([t[1] for t in tabs[k]]))
        assert np.array_equal(I, gold[f"I_shards_k{k}"]) and np.array_equal(bits(D), bits(gold[f"D_shards_k{k}"])), k
    # some query probes a list that a shard does not own (empty there, as in the reference's sub-indexes)
    keys = gold["coarse_keys_sse"]
    for s in range(nshard):
        assert ((keys >= 0) & (keys % nshard != s)).any(), s
    # the shards differ: a shard's table is not the merged one (an error in one shard cannot hide in every query)
    assert any(not np.array_equal(t[1], gold[f"I_shards_k{int(case['ks'][0])}"]) for t in tabs[int(case["ks"][0])])
    # shares of the queries cover them once, in order
    sh = stc.shares(case["xq"].shape[0], nshard)
    assert sh[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(sh, sh[1:])) and sh[-1][0] + sh[-1][1] == case["xq"].shape[0]


def test_golden_cases_keep_their_edges():
    case, gold = load_case("fixed_dups")
    cd = bits(gold["coarse_dis_sse"])
    assert (cd[:, 1:] == cd[:, :-1]).any(), "fixed_dups: no exactly equal coarse distances side by side"
    case, gold = load_case("fixed_ragged")
    assert case["nprobe"] > case["nlist"] and (gold["coarse_keys_sse"][:, case["nlist"]:] == -1).all()
    assert stc.PIPELINED_CASES and all(n in stc.GOLDEN_SHARD_CASES for n in stc.PIPELINED_CASES)


def test_ticket_plan_covers_what_it_says():
    plan = stc.ticket_plan()
    assert {(a, n) for a, n, _, _ in plan} == set(stc.RANGES)
    assert {p for _, _, p, _ in plan} == set(stc.NPROBES) and {k for _, _, _, k in plan} == set(stc.KS)
    for r in stc.RANGES:
        assert (r[0], r[1], min(stc.NPROBES), min(stc.KS)) in plan and (r[0], r[1], max(stc.NPROBES), max(stc.KS)) in plan
        assert 0 <= r[0] and r[0] + r[1] <= stc.SYNTH_NQ, r
    assert any(n == 0 for _, n in stc.RANGES) and any(a > 0 and a + n == stc.SYNTH_NQ for a, n in stc.RANGES)
    assert max(stc.NPROBES) > stc.SYNTH_NLIST
    # the depth-1 order: the same tickets, and every search follows one at the other end of the sizes
    alt = stc.alternating(plan)
    assert sorted(alt) == sorted(plan)
    size = [n * p * k for _, n, p, k in alt]
    med = sorted(size)[len(size) // 2]
    assert all((a >= med) != (b >= med) or a == b == med for a, b in zip(size, size[1:]))
    # ragged shares of the empty-shard case: fewer queries than shards
    q0, n = stc.EMPTY_SHARD_RANGE
    assert (q0, n) in stc.RANGES and 0 in [m for _, m in stc.shares(n, stc.EMPTY_SHARD_NSHARD)]


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("kind", sorted(stc.SYNTH_KINDS))
def test_synthetic_cases_keep_their_edges(oracle, kind, metric):
    c = stc.synth_case(kind, metric)
    d, _ = stc.SYNTH_KINDS[kind]
    assert c["xq"].shape == (stc.SYNTH_NQ, d) and c["xb"].shape == (stc.SYNTH_NB, d) and c["nlist"] == stc.SYNTH_NLIST
    sizes = np.bincount(c["assign"], minlength=c["nlist"])
    assert sizes[1] == 0 and sizes[0] > sizes[2:].max()  # one list emptied into its neighbour
    if kind == "bytes":
        assert c["xb"].min() >= 0 and c["xb"].max() <= 255 and d * 255 * 255 <= 2 ** 24
    elif kind == "wideint":
        assert d % 4 != 0 and c["xb"].max() - c["xq"].min() > 4096 and np.array_equal(c["xb"], np.rint(c["xb"]))
    else:
        assert not np.array_equal(c["xb"], np.rint(c["xb"]))
    # some query's k exceeds its candidate count (the tail of its row is (-1, +-FLT_MAX)); and the smallest probe meets the empty list
    pad = stc.FLT_MAX if metric == 1 else -stc.FLT_MAX
    D, I, _ = stc.synth_search(kind, metric, min(stc.NPROBES), max(stc.KS))
    short = (I == -1).any(1)
    assert short.any() and (bits(D[I == -1]) == bits(pad)).all()
    keys = stc.synth_coarse(kind, metric, max(stc.NPROBES))[1]
    assert (keys[:, :c["nlist"]] >= 0).all() and (keys[:, c["nlist"]:] == -1).all() and (keys == 1).any()
    # results differ from one query to the next: a slice read at the wrong offset cannot pass
    D1 = bits(stc.synth_search(kind, metric, max(stc.NPROBES), 1)[0][:, 0])
    assert (D1[1:] != D1[:-1]).all()


@pytest.mark.parametrize("metric", [1, 0])
def test_the_oracle_on_a_shard_that_owns_nothing(oracle, metric):
    kind, nprobe, k, nshard = "bytes", 5, 10, stc.EMPTY_SHARD_NSHARD
    D, I, st = stc.synth_search(kind, metric, nprobe, k, nshard, 2)
    assert (I == -1).all() and (bits(D) == bits(stc.FLT_MAX if metric == 1 else -stc.FLT_MAX)).all() and not st.any()
    assert (stc.empty_shard_assign(stc.synth_case(kind, metric)["assign"], 2) == -1).all()
    # shards 0 and 1 hold the whole index between them: their merge is the undivided search, with or without the empty table
    tabs = [stc.synth_search(kind, metric, nprobe, k, nshard, s) for s in range(nshard)]
    D2, I2 = oracle.merge_tables(metric, np.stack([t[0] for t in tabs[:2]]), np.stack([t[1] for t in tabs[:2]]))
    D3, I3 = oracle.merge_tables(metric, np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]))
    assert np.array_equal(I2, I3) and np.array_equal(bits(D2), bits(D3))
    eD, eI, _ = stc.synth_search(kind, metric, nprobe, k)
    assert np.array_equal(bits(D2), bits(eD))  # (the ids of exactly equal distances at the k-th place may differ: IndexShards.cpp:44-105)


def test_byte_query_sets_differ_row_by_row(oracle):
    A, B, big = stc.byte_query_sets()
    assert A.shape == B.shape == (stc.SYNTH_NQ, stc.SYNTH_KINDS["bytes"][0]) and big.shape[0] > 2 * A.shape[0]
    assert (A != B).any(1).all() and (A[10:60] != big[10:60]).any(1).all()
    for x in (A, B, big):
        assert x.min() >= 0 and x.max() <= 255
