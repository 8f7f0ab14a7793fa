"""Exact k-NN over float lists (amd_ivf_search_exact through scan_all_f16_kernel + exact_rescore_kernel): (D, I) are, bit
for bit, the pinned CPU oracle's search_preassigned over every list in list-number order -- and what amd_ivf_search_preassigned returns
for those keys on the same handle -- at every piece count of the fp16 pass, both metrics, the ragged lists and batches of the byte
test; the pass serves exactly the queries without equal distances in their window (integer-valued floats counted with numpy, real
values stored twice, copies one ulp apart); the all-zero pair is kept (the non-strict keep rule); calls without a usable fp16 scale,
without the fp16 filter, with the option off or beyond 128 dimensions go the general way whole; the fp16 copy follows changes of the
lists; clones, the resident form, reused buffers; candidate overflow and a loose seed in child processes."""
import numpy as np
import pytest

from test_gpu_exact import (BATCHES, IP, L2, NB, bits, check, exact_ties, expected, ragged_assign, run_child)
from test_gpu_exact import make_handle as plain_handle
from test_gpu_update import Model, make_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def make_handle(capi, metric, cen, xb, assign):
    """the handle of the byte test with the float pass asked for (option "exact_float": off unless set)"""
    h = plain_handle(capi, metric, cen, xb, assign)
    h.set_option("exact_float", 1)
    return h


def float_case(d, nlist, seed, nq=300, nb=NB, clustered=True, ragged=True):
    """Gaussian lists and queries around Gaussian centroids (the seed search then finds most neighbours), or unclustered"""
    rs = np.random.RandomState(seed)
    assign = ragged_assign(nlist, nb) if ragged else rs.randint(0, nlist, size=nb)
    cen = rs.randn(nlist, d).astype(np.float32)
    if clustered:
        xb = (cen[assign] + 0.3 * rs.randn(nb, d)).astype(np.float32)
        xq = (cen[rs.randint(0, nlist, size=nq)] + 0.3 * rs.randn(nq, d)).astype(np.float32)
    else:
        xb = rs.randn(nb, d).astype(np.float32)
        xq = rs.randn(nq, d).astype(np.float32)
    return cen, assign, xb, xq


def fcheck(oracle, h, lists, xq, k, what="", kind=2):
    """check() of the byte test + the pass the call reports; returns (last_exact, last_exact_detail)"""
    last = check(oracle, h, lists, xq, k, what)
    # (check() ends with a search_preassigned: the exact call's counts are the handle's until the next exact call)
    det = h.last_exact_detail()
    assert det[0] == kind, (what, last, det)
    if kind == 0:
        assert last == (0, 0, len(xq), 0) and det == (0, 0, 0, 0), (what, last, det)
    else:
        assert det[1] == last[3] and det[2] <= det[1] and det[3] <= det[1], (what, last, det)
    return last, det


def oracle_ties(oracle, lists, xq, k):
    """queries in whose best k + 1 reference distances two neighbours have the same bits (the oracle's own k + 1 result)"""
    D, _ = expected(oracle, lists, xq, k + 1)
    b = bits(D)
    return (b[:, 1:] == b[:, :-1]).any(axis=1)


@pytest.mark.parametrize("d,metric,nlist", [(8, L2, 16), (8, IP, 32), (30, L2, 32), (30, IP, 16), (96, L2, 16), (96, IP, 32), (128, L2, 32), (128, IP, 16)])
def test_exact_equals_oracle_over_ragged_float_lists(capi, oracle, d, metric, nlist):
    cen, assign, xb, xq = float_case(d, nlist, seed=200 + d + metric)
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    for n, k in BATCHES:
        last, det = fcheck(oracle, h, lists, xq[:n], k, (d, metric, nlist, n, k))
        print(d, metric, n, k, "last_exact", last, "detail", det)
        assert last[0] > 0, (n, k, last, det)
        assert det[2] >= last[0] * k, (last, det)  # (a served query has at least its k best among its valid candidates)
    assert h.scan_arith() != 2
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_the_float_pass_serves_exactly_the_queries_without_ties(capi, oracle, metric):
    """integer-valued floats -8 .. 8 (no byte codes: negative values), d = 8: every distance is an exact integer in fp32, fp16 holds the
    operands as they are, and numpy's int64 arithmetic says which queries tie.  nlist = 16: the seed probes every list, so the
    threshold is the true k-th distance and `within` counts the candidates of a query up to what the bound lets through besides."""
    n, k, nlist, d = 300, 5, 16, 8
    rs = np.random.RandomState(8)
    assign = ragged_assign(nlist)
    cen = rs.randint(-8, 9, size=(nlist, d)).astype(np.float32)
    xb = rs.randint(-8, 9, size=(NB, d)).astype(np.float32)
    xq = rs.randint(-8, 9, size=(3 * n, d)).astype(np.float32)
    tied, within = exact_ties(metric, xb, xq, k)
    pick = np.nonzero(within <= 512)[0][:n]  # (half the default capacity of 1024 slots)
    assert len(pick) == n, len(pick)
    xq, ties = xq[pick], int(tied[pick].sum())
    assert ties >= n // 4 and n - ties >= n // 4, ties
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    last, det = fcheck(oracle, h, lists, xq, k, "integer floats")
    print(metric, "numpy ties", ties, "last_exact", last, "detail", det)
    assert h.scan_arith() != 2
    assert last[:3] == (n - ties, ties, 0), (last, ties, det)
    assert det[2] == int(within[pick].sum()), (det, int(within[pick].sum()))  # (the entries at or within the threshold, all of them)
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_real_valued_ties_every_other_vector_stored_twice(capi, oracle, metric):
    d, nlist, nb, n, k = 30, 16, 6000, 200, 10
    cen, assign, xb, xq = float_case(d, nlist, seed=301 + metric, nq=n, nb=nb, ragged=False)
    twice = np.arange(0, nb, 2)
    xb2 = np.concatenate([xb, xb[twice]])
    assign2 = np.concatenate([assign, (assign[twice] + 5) % nlist])  # the copy lies in another list
    lists = oracle.Lists(metric, cen, xb2, assign2)
    tied = oracle_ties(oracle, lists, xq, k)
    assert 0 < tied.sum() <= n
    h = make_handle(capi, metric, cen, xb2, assign2)
    last, det = fcheck(oracle, h, lists, xq, k, "stored twice")
    print(metric, "oracle ties", int(tied.sum()), "last_exact", last, "detail", det)
    assert last[1] == int(tied.sum()) and last[2] == 0, (last, int(tied.sum()))
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [32, 96])
def test_copies_one_ulp_apart(capi, oracle, d, metric):
    """test_gpu_filter.py's construction: every vector three times, next to four copies one ulp away in one coordinate, spread over the
    lists -- the k-th distance of a query is shared by, or within an ulp of, other entries"""
    rs = np.random.RandomState(7200 + d + metric)
    nlist, nq, k = 16, 160, 12
    cen = rs.randn(nlist, d).astype(np.float32)
    seeds = (cen[rs.randint(0, nlist, size=300)] + 0.3 * rs.randn(300, d)).astype(np.float32)
    rows = []
    for v in seeds:
        rows += [v] * 3
        for _ in range(4):
            w = v.copy()
            c = rs.randint(0, d)
            w[c] = np.nextafter(w[c], np.float32(np.inf if rs.rand() < 0.5 else -np.inf), dtype=np.float32)
            rows.append(w)
    xb = np.stack(rows).astype(np.float32)
    xb = xb[rs.permutation(len(xb))]
    assign = rs.randint(0, nlist, size=len(xb))
    xq = (seeds[rs.randint(0, len(seeds), size=nq)] + 0.05 * rs.randn(nq, d)).astype(np.float32)
    lists = oracle.Lists(metric, cen, xb, assign)
    tied = oracle_ties(oracle, lists, xq, k)
    h = make_handle(capi, metric, cen, xb, assign)
    last, det = fcheck(oracle, h, lists, xq, k, "one ulp")
    print(d, metric, "oracle ties", int(tied.sum()), "last_exact", last, "detail", det)
    assert last[:3] == (nq - int(tied.sum()), int(tied.sum()), 0), (last, int(tied.sum()))
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_zero_query_and_zero_vectors(capi, oracle, metric):
    d, nlist, nb = 30, 16, 2000
    cen, assign, xb, xq = float_case(d, nlist, seed=401, nq=20, nb=nb, ragged=False)
    zero = np.zeros((1, d), np.float32)
    # one stored zero vector, a zero query, k = 1.  L2: the pair's distance and the threshold are both 0, |x|^2 + |y|^2 = 0 leaves the
    # bound no slack -- a strict keep test drops the one entry the query needs.  IP: every entry is at 0, all of them tie
    xb1 = xb.copy()
    xb1[77] = 0
    lists = oracle.Lists(metric, cen, xb1, assign)
    h = make_handle(capi, metric, cen, xb1, assign)
    last, det = fcheck(oracle, h, lists, zero, 1, "zero query, one zero vector")
    if metric == L2:
        assert last[:3] == (1, 0, 0) and det[2] == 1, (last, det)
    fcheck(oracle, h, lists, np.concatenate([zero, xq, zero]), 1, "zero queries among others")
    h.close()
    # k + 1 stored zero vectors in different lists: L2 the zero query's window is all zeros, a tie
    k = 3
    xb2 = xb.copy()
    where = np.array([10, 500, 901, 1502])
    xb2[where] = 0
    assert len(set(assign[where])) > 1
    lists = oracle.Lists(metric, cen, xb2, assign)
    h = make_handle(capi, metric, cen, xb2, assign)
    last, det = fcheck(oracle, h, lists, zero, k, "k + 1 zero vectors")
    if metric == L2:
        assert last[:3] == (0, 1, 0) and det[2] == k + 1, (last, det)
    fcheck(oracle, h, lists, np.concatenate([xq, zero]), k, "k + 1 zero vectors, more queries")
    h.close()


@pytest.mark.parametrize("what", ["list_row_tiny", "query_row_tiny", "filter_1", "filter_0", "exact_float_0", "exact_float_unset", "d_200"])
def test_a_float_call_that_does_not_qualify_goes_the_general_way_whole(capi, oracle, what):
    n, k, metric = 40, 10, L2
    d = 200 if what == "d_200" else 96
    cen, assign, xb, xq = float_case(d, 16, seed=501, nq=n, nb=4000)
    if what == "list_row_tiny":
        xb[1234] *= np.float32(2.0 ** -20)  # its largest element is below 2^-12 of the lists': no one scale serves the matrix
    if what == "query_row_tiny":
        xq[7] *= np.float32(2.0 ** -20)
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    if what.startswith("filter_"):
        h.set_option("filter", int(what[-1]))
    if what == "exact_float_0":
        h.set_option("exact_float", 0)
    if what == "exact_float_unset":  # the default: a float call does what it did before there was a pass
        h.set_option("exact_float", float("nan"))
        assert h.get_option("exact_float") == 0
    fcheck(oracle, h, lists, xq, k, what, kind=0)
    if what == "query_row_tiny":  # the rule is the call's: the other queries alone take the pass
        fcheck(oracle, h, lists, xq[8:], k, what + ", other queries")
    if what.startswith("exact_float_"):
        h.set_option("exact_float", 1)
        assert fcheck(oracle, h, lists, xq, k, what + ", on again")[0][0] > 0
    h.close()


@pytest.mark.parametrize("what", ["l2_96", "ip_96", "query_256", "byte_codes_off"])
def test_calls_the_byte_pass_does_not_serve_take_the_float_pass(capi, oracle, what):
    """four inputs that go the general way whole by default (test_gpu_exact.py pins that), with the float pass asked for: float lists,
    and byte-valued lists whose call leaves the byte rule (a query value of 256) or whose handle has the byte codes switched off"""
    from test_gpu_exact import byte_case
    n, k = 40, 10
    if what in ("l2_96", "ip_96"):
        metric, cen, assign, xb, xq = make_case(what)
        xq = xq[:n]
    else:
        metric = L2
        cen, assign, xb, xq = byte_case(64, 16, seed=31, nq=n, nb=4000)
        if what == "query_256":
            xq[5, 3] = 256.0
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    if what == "byte_codes_off":
        h.set_byte_codes(0)
    last, det = fcheck(oracle, h, lists, xq, k, what)
    assert last[0] + last[1] == n and last[2] == 0, (last, det)
    h.close()


def test_after_changes_of_float_lists_on_a_clone_and_resident(capi, oracle):
    metric, cen, assign, xb, xq = make_case("l2_96")
    nlist, d = cen.shape
    rs = np.random.RandomState(5)
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(nlist, d, xb, assign)
    k = 10

    def lists_now():
        fx, fa, fi = model.flat()
        return oracle.Lists(metric, cen, fx, fa, fi)

    def near(to):
        return (cen[to] + 0.3 * rs.randn(len(to), d)).astype(np.float32)

    assert fcheck(oracle, h, lists_now(), xq[:70], k, "before")[0][0] > 0
    # amd_ivf_add: the journal is pending when the exact call starts; the fp16 copy follows it
    to = np.array([2] * 40 + [3, 7, 7], np.int64)
    x = near(to)
    ids = np.arange(50000, 50000 + len(to), dtype=np.int64)
    h.add(x, ids, to)
    model.add(x, ids, to)
    last, _ = fcheck(oracle, h, lists_now(), xq[:70], k, "add")
    assert last[0] > 0 and h.last_update()[0] == 1
    # amd_ivf_remove_ids
    sel = [model.ids[3][1], model.ids[3][-1]] + list(model.ids[9][:50])
    assert h.remove_ids(np.array(sel)) == model.remove_ids(sel)
    fcheck(oracle, h, lists_now(), xq[:70], k, "remove")
    # amd_ivf_update_lists: grow one list, shrink another, overwrite an entry
    sizes = [len(i) for i in model.ids]
    new_sizes = list(sizes)
    new_sizes[4] += 2
    new_sizes[10] -= 3
    where = [(4 << 32) | sizes[4], (4 << 32) | (sizes[4] + 1), (11 << 32) | 0]
    x = near(np.array([w >> 32 for w in where]))
    ids = np.arange(60000, 60000 + len(where), dtype=np.int64)
    h.update_lists(new_sizes, np.array(where, np.uint64), ids, x)
    model.update(new_sizes, where, ids, x)
    lists = lists_now()
    fcheck(oracle, h, lists, xq[:70], k, "update_lists")
    # an added row that moves the lists' scale: the whole fp16 copy is encoded again
    big = (8.0 * near(np.array([6]))).astype(np.float32)
    h.add(big, np.array([70000], np.int64), np.array([6], np.int64))
    model.add(big, np.array([70000], np.int64), np.array([6], np.int64))
    lists = lists_now()
    fcheck(oracle, h, lists, xq[:70], k, "scale moved")
    # on a clone, and the resident form over a slice that does not start at 0 (on the owner and on the clone)
    c = h.clone()
    assert fcheck(oracle, c, lists, xq[:130], k, "clone")[0][0] > 0
    eD, eI = expected(oracle, lists, xq, k)
    for ctx in (h, c):
        ctx.set_queries(xq)
        D, I = ctx.search_exact_resident(37, 150, k)
        assert np.array_equal(I, eI[37:187]) and np.array_equal(bits(D), bits(eD[37:187]))
        assert sum(ctx.last_exact()[:3]) == 150 and ctx.last_exact()[0] > 0 and ctx.last_exact_detail()[0] == 2
    c.close()
    h.close()


def test_reused_buffers_a_larger_then_a_smaller_float_call(capi, oracle):
    cen, assign, xb, xq = float_case(96, 16, seed=41, nq=300, nb=6000)
    lists = oracle.Lists(IP, cen, xb, assign)
    h = make_handle(capi, IP, cen, xb, assign)
    for n, k in ((20, 10), (300, 64), (7, 10), (260, 1), (64, 100)):
        fcheck(oracle, h, lists, xq[:n], k, ("reuse", n, k))
    h.close()


def test_byte_calls_report_their_pass_too(capi, oracle):
    from test_gpu_exact import byte_case
    cen, assign, xb, xq = byte_case(64, 16, seed=51, nq=100, nb=5000)
    h = make_handle(capi, L2, cen, xb, assign)
    last, det = fcheck(oracle, h, oracle.Lists(L2, cen, xb, assign), xq, 10, "bytes", kind=1)
    assert det[1] == det[2] == last[3] and 10 <= det[3] <= det[1], (last, det)
    h.close()


def test_float_candidate_overflow_in_a_child_process(oracle, tmp_path):
    """AUNCEL_AMD_EXACT_CAP=16: with k = 10 and a threshold from an eighth of the lists of unclustered data, queries overflow their slots"""
    cen, assign, xb, xq = float_case(64, 32, seed=61, clustered=False, nq=200)
    calls = [dict(name=f"m{m}", metric=m, cen="cen", xb="xb", assign="assign", xq="xq", k=10) for m in (L2, IP)]
    out = run_child(tmp_path, {"AUNCEL_AMD_EXACT_CAP": "16", "AUNCEL_AMD_EXACT_SEED": "4", "AUNCEL_AMD_EXACT_FLOAT": "1"}, calls, dict(cen=cen, xb=xb, assign=assign, xq=xq))
    for m in (L2, IP):
        eD, eI = expected(oracle, oracle.Lists(m, cen, xb, assign), xq, 10)
        last = out[f"m{m}/last"]
        print("cap 16, metric", m, "last_exact", last)
        assert np.array_equal(out[f"m{m}/I"], eI) and np.array_equal(bits(out[f"m{m}/D"]), bits(eD))
        assert last[2] > 0 and last[:3].sum() == len(xq) and last[3] > 0, last  # (candidates were emitted: the pass ran)


def test_a_loose_seed_over_float_lists_in_a_child_process(oracle, tmp_path):
    """AUNCEL_AMD_EXACT_SEED=1 on clustered data: the threshold comes from one list, many candidates per query"""
    cen, assign, xb, xq = float_case(128, 32, seed=71, nq=200)
    calls = [dict(name=f"m{m}", metric=m, cen="cen", xb="xb", assign="assign", xq="xq", k=10) for m in (L2, IP)]
    out = run_child(tmp_path, {"AUNCEL_AMD_EXACT_SEED": "1", "AUNCEL_AMD_EXACT_FLOAT": "1"}, calls, dict(cen=cen, xb=xb, assign=assign, xq=xq))
    for m in (L2, IP):
        eD, eI = expected(oracle, oracle.Lists(m, cen, xb, assign), xq, 10)
        last = out[f"m{m}/last"]
        print("seed 1, metric", m, "last_exact", last)
        assert np.array_equal(out[f"m{m}/I"], eI) and np.array_equal(bits(out[f"m{m}/D"]), bits(eD))
        assert last[:3].sum() == len(xq) and last[0] > 0 and last[3] >= last[0] * 10, last
