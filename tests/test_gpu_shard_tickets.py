"""The two halves of a sharded search as tickets -- amd_ivf_submit_coarse_resident and amd_ivf_submit_search_resident_preassigned,
the loop of sharding.run_pipelined behind bench.py --mode shards -- against the goldens of the compiled reference and the CPU oracle,
bit for bit.  A ticket runs on one of the handle's internal contexts (an amd_ivf_clone: it reads the owner's resident queries and
keeps launch-size hints from its own previous search), so the cases here are the ones that path can get wrong on its own: slices
with start > 0, consecutive tickets of very different shapes on one context, shares of no queries, shards that own nothing, keys
padded with -1, an error delivered by wait() in front of a queued ticket, and a new resident query set of the same shape.  No
expected value comes from a synchronous call of the engine; tests/test_shard_tickets_model_cpu.py checks the inputs' edges."""
import numpy as np
import pytest

import shard_ticket_cases as stc
from util import load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    assert capi.device_count() >= 1
    return capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(D, I, eD, eI):
    return D.shape == eD.shape and I.shape == eI.shape and np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))


def out_buffers(n, k):
    """caller-provided result buffers, filled with values no search returns"""
    return np.full((n, k), np.nan, np.float32), np.full((n, k), -7, np.int64)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. golden shard cases through tickets
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", stc.GOLDEN_SHARD_CASES)
def test_golden_shards_through_tickets(capi, oracle, name):
    """one handle per list-id shard; every shard ranks its share of the queries and searches all of them over its own lists, all
    through tickets: the key rows joined are the reference's, every shard's table is the oracle's over that shard's lists, the
    merged table is the reference's IndexShards output.  Fails if a context read resident rows of its own instead of its owner's (the
    shares start at r nq / N > 0), if a probed list the shard does not own were not skipped like an empty one (the per-shard tables: a
    wrong candidate of one shard can lose the merge to another shard's better ones and go unseen there), or if a queued ticket's
    result landed in another ticket's buffers"""
    case, gold = load_case(name)
    nshard, nq, nprobe, metric = int(case["nshard"]), case["xq"].shape[0], int(case["nprobe"]), case["metric"]
    want = stc.golden_shard_tables(name)
    handles = []
    for s in range(nshard):
        h = capi.Handle(case["d"], case["nlist"], metric, 0)
        h.set_centroids(case["centroids"])
        h.set_lists_from_assign(case["xb"], stc.shard_assign(gold["assign"], nshard, s))
        h.set_queries(case["xq"])
        h.set_async_depth(2)
        handles.append(h)
    before = [h.async_counts()[0] for h in handles]
    # coarse half: every shard's share, without and with distances; all tickets out before the first wait
    share = stc.shares(nq, nshard)
    tickets = [[h.submit_coarse_resident(q0, n, nprobe, mode=0, want_dis=w) for w in (False, True)] for h, (q0, n) in zip(handles, share)]
    for w in (0, 1):
        got = [h.wait(t[w])[:2] for h, t in zip(handles, tickets)]
        for (dis, keys), (q0, n) in zip(got, share):
            assert keys.shape == (n, nprobe) and (dis is None if w == 0 else dis.shape == (n, nprobe))
        assert np.array_equal(np.concatenate([g[1] for g in got]), gold["coarse_keys_sse"]), w
        if w:
            assert np.array_equal(bits(np.concatenate([g[0] for g in got])), bits(gold["coarse_dis_sse"]))
    # search half: every shard, every k, twice -- more tickets on a handle than its depth, so some queue; waited in reverse
    jobs = []
    for rep in range(2):
        for k in case["ks"]:
            for s, h in enumerate(handles):
                out = out_buffers(nq, int(k))
                jobs.append((h.submit_search_resident_preassigned(0, nq, int(k), gold["coarse_keys_sse"], out=out), s, int(k), rep, out))
    tables = {}
    for t, s, k, rep, out in reversed(jobs):
        D, I, _, _ = handles[s].wait(t)
        assert D is out[0] and I is out[1]
        assert same(D, I, *want[k][s]), (s, k, rep)
        tables[(rep, k, s)] = (D, I)
    for rep in range(2):
        for k in case["ks"]:
            k = int(k)
            D, I = capi.merge_tables(metric, np.stack([tables[(rep, k, s)][0] for s in range(nshard)]),
                                     np.stack([tables[(rep, k, s)][1] for s in range(nshard)]))
            assert same(D, I, gold[f"D_shards_k{k}"], gold[f"I_shards_k{k}"]), (k, rep)
    for h, b in zip(handles, before):
        assert h.async_counts()[0] - b == 2 + 2 * len(case["ks"])
        h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. sharding.run_pipelined over a real handle
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", stc.PIPELINED_CASES)
def test_run_pipelined_over_a_real_handle(capi, name):
    """world size 1 over the undivided index: every step's coarse ranking and search are the engine's tickets, the merge of the one
    table is the plain search's golden (D, I).  Fails if the last step's table is not the reference's (its search ran while up to
    two later steps' tickets were out or queued on the same two contexts, into a buffer of the loop's ring), if a step were merged
    twice or not at all, or if the loop submitted more or fewer tickets than two a step.  Every step computes the same table, so
    key rows that travelled with the wrong step would not show here: the gloo rehearsal and section 1 hold that side"""
    from auncel_amd import sharding
    case, gold = load_case(name)
    nq, k, nprobe = case["xq"].shape[0], int(case["ks"][0]), int(case["nprobe"])
    h = capi.Handle(case["d"], case["nlist"], case["metric"], 0)
    h.set_centroids(case["centroids"])
    h.set_lists_from_assign(case["xb"], gold["assign"])
    h.set_queries(case["xq"])
    h.set_async_depth(2)  # (a lag of 3 keeps more searches out than run at a time)
    for lag in (1, 3):
        for ahead in (1, 2):
            before = h.async_counts()[0]
            out, acc = sharding.run_pipelined(h, case["metric"], capi.merge_tables, nq, k, nprobe, [nq], 0, None, 5, lag=lag, coarse_ahead=ahead)
            assert same(out[0], out[1], gold[f"D_k{k}"], gold[f"I_k{k}"]), (lag, ahead)
            assert acc["steps_merged"] == 5, (lag, ahead)
            assert all(np.isfinite(v) and v >= 0 for v in acc.values()), acc
            assert h.async_counts()[0] - before == 10, (lag, ahead)
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. slices and shapes against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def synth_handle(capi, c, assign=None, depth=2):
    h = capi.Handle(c["d"], c["nlist"], c["metric"], 0)
    h.set_centroids(c["cen"])
    h.set_lists_from_assign(c["xb"], c["assign"] if assign is None else assign)
    h.set_queries(c["xq"])
    h.set_async_depth(depth)
    return h


def run_plan(h, c, plan, tag):
    """a coarse ticket and a search ticket (over the oracle's keys) for every entry, all out before the first wait, waited in reverse"""
    kind, metric = c["kind"], c["metric"]
    before = h.async_counts()[0]
    jobs = []
    for i, (q0, n, nprobe, k) in enumerate(plan):
        tc = h.submit_coarse_resident(q0, n, nprobe, mode=0, want_dis=i % 2 == 0)
        out = out_buffers(n, k)
        ts = h.submit_search_resident_preassigned(q0, n, k, stc.synth_coarse(kind, metric, nprobe)[1][q0:q0 + n], out=out)
        jobs.append((tc, ts, i, out))
    for tc, ts, i, out in reversed(jobs):
        q0, n, nprobe, k = plan[i]
        what = (tag, q0, n, nprobe, k)
        D, I, _, _ = h.wait(ts)
        eD, eI, _ = stc.synth_search(kind, metric, nprobe, k)
        assert D is out[0] and I is out[1] and same(D, I, eD[q0:q0 + n], eI[q0:q0 + n]), what
        dis, keys, _, _ = h.wait(tc)
        edis, ekeys = stc.synth_coarse(kind, metric, nprobe)
        assert keys.shape == (n, nprobe) and np.array_equal(keys, ekeys[q0:q0 + n]), what
        if nprobe > c["nlist"] and n:
            assert (keys[:, c["nlist"]:] == -1).all(), what
        if i % 2 == 0:
            assert dis.shape == (n, nprobe) and np.array_equal(bits(dis), bits(edis[q0:q0 + n])), what
        else:
            assert dis is None, what
    assert h.async_counts()[0] - before == 2 * len(plan), tag


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("kind", sorted(stc.SYNTH_KINDS))
def test_ticket_slices_and_shapes(capi, oracle, kind, metric):
    """ranges at both ends and across the middle of the resident set, an empty range, nprobe from 1 to beyond nlist, k from 1 to beyond
    the candidates -- two contexts first, then ONE context on which every search follows one of the opposite size.  Fails if the row
    offset of a slice were start * d instead of start * dpad (d = 30: row 129 would begin 258 floats early), if the cached coarse
    work list of one call size served another, or if a launch size hinted by the previous search (130 x 19 x 200 before 1 x 1 x 1
    and the reverse) cut off candidates instead of only sizing a grid"""
    c = stc.synth_case(kind, metric)
    h = synth_handle(capi, c, depth=2)
    plan = stc.ticket_plan()
    run_plan(h, c, plan, "depth 2")
    # the arithmetic the data allows (include/auncel_amd.h: amd_ivf_scan_arith): signed integers up to 4000 fuse under the inner
    # product (every product below 2^24) and not under L2 (differences up to 8000)
    assert h.scan_arith() == (1 if kind == "wideint" and metric == 0 else c["arith"])
    h.set_async_depth(0)
    h.set_async_depth(1)
    run_plan(h, c, stc.alternating(plan), "depth 1")
    h.close()


@pytest.mark.parametrize("metric", [1, 0])
def test_a_shard_that_owns_nothing(capi, oracle, metric):
    """three shards, the third without a single vector: its table is all (-1, +-FLT_MAX) and changes nothing in the merge; two
    queries ranked over three shards leave one share empty"""
    kind = "bytes"
    c = stc.synth_case(kind, metric)
    q0, n = stc.EMPTY_SHARD_RANGE
    nprobe, k, nshard = 5, 10, stc.EMPTY_SHARD_NSHARD
    handles = [synth_handle(capi, c, stc.empty_shard_assign(c["assign"], s)) for s in range(nshard)]
    assert handles[2].ntotal == 0
    share = [(q0 + a, m) for a, m in stc.shares(n, nshard)]
    ct = [h.submit_coarse_resident(a, m, nprobe, mode=0, want_dis=True) for h, (a, m) in zip(handles, share)]
    st = []
    ekeys = stc.synth_coarse(kind, metric, nprobe)[1][q0:q0 + n]
    for h in handles:
        out = out_buffers(n, k)
        st.append((h.submit_search_resident_preassigned(q0, n, k, ekeys, out=out), out))
    got = [h.wait(t)[:2] for h, t in zip(handles, ct)]
    assert [g[1].shape[0] for g in got] == [m for _, m in share]
    assert np.array_equal(np.concatenate([g[1] for g in got]), ekeys)
    assert np.array_equal(bits(np.concatenate([g[0] for g in got])), bits(stc.synth_coarse(kind, metric, nprobe)[0][q0:q0 + n]))
    tabs = []
    for s, (h, (t, out)) in enumerate(zip(handles, st)):
        D, I, _, _ = h.wait(t)
        eD, eI, _ = stc.synth_search(kind, metric, nprobe, k, nshard, s)
        assert same(D, I, eD[q0:q0 + n], eI[q0:q0 + n]), s
        tabs.append((D, I))
    assert (tabs[2][1] == -1).all() and (bits(tabs[2][0]) == bits(stc.FLT_MAX if metric == 1 else -stc.FLT_MAX)).all()
    D3, I3 = capi.merge_tables(metric, np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]))
    D2, I2 = oracle.merge_tables(metric, np.stack([stc.synth_search(kind, metric, nprobe, k, nshard, s)[0][q0:q0 + n] for s in (0, 1)]),
                                 np.stack([stc.synth_search(kind, metric, nprobe, k, nshard, s)[1][q0:q0 + n] for s in (0, 1)]))
    assert same(D3, I3, D2, I2)
    for h in handles:
        h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. errors through wait
# ------------------------------------------------------------------------------------------------------------------------------
def test_errors_come_from_wait_and_the_context_goes_on(capi, oracle):
    """an invalid key is the engine's error word, delivered by that ticket's wait(); the ticket queued behind it on the same (only)
    context returns the oracle's result; a range out of bounds is refused at submit and serves no ticket.  Fails if the error word
    of the failed search outlived it on the context, if wait() kept the failed job (the second wait must not find it), or if a
    refused submit had already queued something"""
    case, gold = load_case("fixed_ragged")
    nq, k = case["xq"].shape[0], 10
    lists = oracle.Lists(case["metric"], case["centroids"], case["xb"], gold["assign"])
    eD, eI, _ = oracle.search_preassigned(lists, case["xq"], k, gold["coarse_keys_sse"], gold["coarse_dis_sse"])
    h = capi.Handle(case["d"], case["nlist"], case["metric"], 0)
    h.set_centroids(case["centroids"])
    h.set_lists_from_assign(case["xb"], gold["assign"])
    h.set_queries(case["xq"])
    h.set_async_depth(1)
    before = h.async_counts()[0]
    with pytest.raises(capi.EngineError, match="out of bounds") as e:
        h.submit_search_resident_preassigned(1, nq, k, gold["coarse_keys_sse"])
    assert e.value.code == -2
    with pytest.raises(capi.EngineError, match="out of bounds"):
        h.submit_coarse_resident(nq, 1, case["nprobe"])
    assert h.async_counts()[0] == before
    keys = gold["coarse_keys_sse"].copy()
    keys[0, 0] = case["nlist"] + 3
    bad = h.submit_search_resident_preassigned(0, nq, k, keys)
    good = h.submit_search_resident_preassigned(3, nq - 3, k, gold["coarse_keys_sse"][3:])
    with pytest.raises(capi.EngineError, match="Invalid key") as e:
        h.wait(bad)
    assert e.value.code == -2
    with pytest.raises(capi.EngineError, match="ticket"):
        h.wait(bad)
    D, I, _, _ = h.wait(good)
    assert same(D, I, eD[3:], eI[3:])
    assert h.async_counts()[0] - before == 2
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 5. a new resident query set of the same shape
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [1, 0])
def test_a_new_resident_query_set_of_the_same_shape(capi, oracle, metric):
    """byte data: the owner keeps a signed-byte view of the slice it searched last, keyed by address, length and the generation of the
    resident set; set_queries of the same shape lands in the same buffer, and the next search of the same slice must read the new rows.
    Fails if set_queries did not advance the generation (the third call would answer B with A's bytes: the ids differ, asserted below),
    or if a context of the pool kept rows or bytes of the earlier set"""
    c = stc.synth_case("bytes", metric)
    lists = stc.synth_lists("bytes", metric)
    A, B, big = stc.byte_query_sets()
    q0, n, nprobe, k = 10, 50, 5, 10

    def expect(x):
        cd, ck = oracle.knn(metric, x[q0:q0 + n], c["cen"], nprobe)
        D, I, _ = oracle.search_preassigned(lists, x[q0:q0 + n], k, ck, cd)
        return ck, D, I

    kA, DA, IA = expect(A)
    kB, DB, IB = expect(B)
    kC, DC, IC = expect(big)
    assert not np.array_equal(IA, IB)
    h = synth_handle(capi, c, depth=2)
    h.set_queries(A)
    for rep in range(2):
        D, I = h.search_resident_preassigned(q0, n, k, kA)
        assert h.scan_arith() == 2 and same(D, I, DA, IA), rep
    h.set_queries(B)
    D, I = h.search_resident_preassigned(q0, n, k, kB)
    assert same(D, I, DB, IB)
    D, I, _, _ = h.wait(h.submit_search_resident_preassigned(q0, n, k, kB))
    assert same(D, I, DB, IB)
    _, keys, _, _ = h.wait(h.submit_coarse_resident(q0, n, nprobe))
    assert np.array_equal(keys, kB)
    h.set_queries(big)  # (no ticket is out: include/auncel_amd.h keeps the resident queries unchanged while one is)
    D, I = h.search_resident_preassigned(q0, n, k, kC)
    assert same(D, I, DC, IC)
    D, I, _, _ = h.wait(h.submit_search_resident_preassigned(q0, n, k, kC))
    assert same(D, I, DC, IC)
    h.set_queries(A)
    D, I, _, _ = h.wait(h.submit_search_resident_preassigned(q0, n, k, kA))
    assert same(D, I, DA, IA)
    D, I = h.search_resident_preassigned(q0, n, k, kA)
    assert same(D, I, DA, IA)
    h.close()
