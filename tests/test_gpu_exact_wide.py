"""Exact k-NN over float lists beyond 128 dimensions (option "exact_wide": scan_all_wide_f16_kernel + exact_rescore_kernel, DESIGN.md
13.2).  (D, I) are, bit for bit, the pinned CPU oracle's search_preassigned over every list in list-number order -- and what
amd_ivf_search_preassigned returns for those keys on the same handle -- and every served call reports pass 3:
  a. the piece counts and stage edges of the tile (d = 132, 192, 200, 960: a padded last stage, exactly two stages, a tail beyond d,
     ten stages), ragged lists, batches around the query block and the 128-query tile
  b. the chunk tail: a block stream of a multiple of four blocks, of two more, and of two blocks in all
  c. rows that differ in the last eight of 200 dimensions only
  d. the pass serves exactly the queries without equal distances in their window (integer-valued floats; copies one ulp apart)
  e. the all-zero pair (the non-strict keep rule)
  f. the error bound on coherently rounded data (filter_bound_cases.py; test_exact_wide_cpu.py holds the preconditions)
  g. under a selector (the KEEP form)
  h. calls that do not qualify go the general way whole
  i. after changes of the lists, on a clone, resident queries, reused buffers
  j. candidate overflow and a loose seed in child processes
  k. a call of up to 128 dimensions on a handle with the option set takes the pass it took"""
import numpy as np
import pytest

import filter_bound_cases as fb
from test_gpu_exact import IP, L2, bits, check, exact_ties, expected, ragged_assign, run_child
from test_gpu_exact import make_handle as plain_handle
from test_gpu_exact_float import fcheck, float_case, oracle_ties
from test_gpu_exact_selected import check as sel_check
from test_gpu_subset import id_bits
from test_gpu_update import Model, make_case

pytestmark = pytest.mark.gpu

NB = 4000
BATCHES = [(1, 100), (33, 65), (128, 10), (129, 64), (257, 1)]


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def make_handle(capi, metric, cen, xb, assign, ids=None):
    h = capi.Handle(cen.shape[1], cen.shape[0], metric, 0)
    h.set_centroids(cen)
    if ids is None:
        h.set_lists_from_assign(xb, assign)
    else:
        h.set_lists_from_assign(xb, assign, ids)
    h.set_option("exact_float", 1)
    h.set_option("exact_wide", 1)
    return h


def wcheck(oracle, h, lists, xq, k, what="", kind=3):
    return fcheck(oracle, h, lists, xq, k, what, kind=kind)


def within_count(oracle, lists, xq, k, metric, ntotal):
    """the stored entries at or within every query's true k-th reference distance, summed (the oracle's own distances at k = ntotal)"""
    all_D, _ = expected(oracle, lists, xq, ntotal)
    tau = all_D[:, k - 1][:, None]
    return int((all_D <= tau if metric == L2 else all_D >= tau).sum())


# ------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [132, 192, 200, 960])
def test_exact_equals_oracle_at_every_stage_edge(capi, oracle, d, metric):
    nlist = 32
    cen, assign, xb, xq = float_case(d, nlist, seed=900 + d + metric, nq=257, nb=NB)
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    for n, k in BATCHES:
        last, det = wcheck(oracle, h, lists, xq[:n], k, (d, metric, n, k))
        print(d, metric, n, k, "last_exact", last, "detail", det)
        assert last[0] > 0, (n, k, last, det)
        assert det[2] >= last[0] * k, (last, det)
    assert h.scan_arith() != 2
    h.close()


# ------------------------------------------------------------------------------------------ b
def layout_case(sizes, d, seed, nq=40):
    """lists of the given sizes around centroids far from each other; the queries lie around the LAST non-empty list's centroid, so
    their neighbours are entries only that list holds"""
    rs = np.random.RandomState(seed)
    nlist = len(sizes)
    cen = (4.0 * rs.randn(nlist, d)).astype(np.float32)
    assign = np.repeat(np.arange(nlist), sizes)
    xb = (cen[assign] + 0.3 * rs.randn(len(assign), d)).astype(np.float32)
    last = max(l for l in range(nlist) if sizes[l])
    xq = (cen[last] + 0.3 * rs.randn(nq, d)).astype(np.float32)
    return cen, assign, xb, xq, last


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("sizes,rem", [((100, 64, 0, 130, 50, 30), 0), ((100, 64, 0, 130, 50), 2), ((0, 0, 40, 0), 2)], ids=["nblk_16", "nblk_14", "nblk_2"])
def test_the_chunk_tail(capi, oracle, sizes, rem, metric):
    d, k = 200, 10
    nblk = sum(2 * -(-s // 64) for s in sizes)
    assert nblk % 4 == rem and nblk == {6: 16, 5: 14, 4: 2}[len(sizes)]
    cen, assign, xb, xq, last_list = layout_case(sizes, d, seed=1300 + len(sizes) + metric)
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)  # (the seed probes every list: the threshold is the true k-th distance)
    last, det = wcheck(oracle, h, lists, xq, k, (sizes, metric))
    eD, eI = expected(oracle, lists, xq, k)
    assert (assign[eI] == last_list).all()  # the neighbours are entries of the last list, whose blocks are the stream's last
    assert last[2] == 0 and last[0] > 0, (last, det)
    assert det[2] == within_count(oracle, lists, xq, k, metric, len(xb)), (last, det)
    h.close()


# ------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [200, 192])
def test_the_last_dimensions_decide(capi, oracle, d, metric):
    """every row of a list equals its centroid in all but the last eight dimensions and differs in those only; so do the queries.
    d = 200: dimensions 192 .. 199, piece 12 of 14, the first piece of the last stage (piece 13 is padding) -- a kernel that skips the
    last stage's real pieces or zero-fills one it should read sees every row of a list at one distance.  d = 192: dimensions
    184 .. 191, the upper half of piece 11 of 12, the LAST piece there is -- a kernel that reads one piece too few sees the same"""
    nlist, nb, n, k = 16, 3000, 64, 10
    rs = np.random.RandomState(77 + metric + d)
    cen = rs.randn(nlist, d).astype(np.float32)
    cen[:, d - 8:] = 0
    assign = rs.randint(0, nlist, size=nb)
    xb = cen[assign].copy()
    xb[:, d - 8:] = rs.randn(nb, 8).astype(np.float32)
    xq = cen[rs.randint(0, nlist, size=n)].copy()
    xq[:, d - 8:] = rs.randn(n, 8).astype(np.float32)
    assert np.array_equal(xb[:, :d - 8], cen[assign][:, :d - 8])
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)  # (16 lists: the seed probes all of them)
    last, det = wcheck(oracle, h, lists, xq, k, "last dimensions")
    print(d, metric, "last_exact", last, "detail", det)
    assert last[2] == 0 and last[0] > 0, (last, det)
    assert det[2] == within_count(oracle, lists, xq, k, metric, nb), (last, det)
    h.close()


# ------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("metric", [L2, IP])
def test_the_wide_pass_serves_exactly_the_queries_without_ties(capi, oracle, metric):
    """integer-valued floats -8 .. 8 at d = 136: every distance is an exact integer in fp32, fp16 holds the operands as they are, and
    numpy's int64 arithmetic says which queries tie.  nlist = 16: the seed probes every list"""
    n, k, nlist, d, nb = 200, 5, 16, 136, 6000
    rs = np.random.RandomState(8)
    assign = ragged_assign(nlist, nb)
    cen = rs.randint(-8, 9, size=(nlist, d)).astype(np.float32)
    xb = rs.randint(-8, 9, size=(nb, d)).astype(np.float32)
    xq = rs.randint(-8, 9, size=(3 * n, d)).astype(np.float32)
    tied, within = exact_ties(metric, xb, xq, k)
    pick = np.nonzero(within <= 512)[0][:n]
    assert len(pick) == n, len(pick)
    xq, ties = xq[pick], int(tied[pick].sum())
    assert 0 < ties < n, ties
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    last, det = wcheck(oracle, h, lists, xq, k, "integer floats")
    print(metric, "numpy ties", ties, "last_exact", last, "detail", det)
    assert last[:3] == (n - ties, ties, 0), (last, ties, det)
    assert det[2] == int(within[pick].sum()), (det, int(within[pick].sum()))
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_copies_one_ulp_apart(capi, oracle, metric):
    d = 160
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
    last, det = wcheck(oracle, h, lists, xq, k, "one ulp")
    print(metric, "oracle ties", int(tied.sum()), "last_exact", last, "detail", det)
    assert last[:3] == (nq - int(tied.sum()), int(tied.sum()), 0), (last, int(tied.sum()))
    h.close()


# ------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("metric", [L2, IP])
def test_zero_query_and_zero_vectors(capi, oracle, metric):
    d, nlist, nb = 136, 16, 2000
    cen, assign, xb, xq = float_case(d, nlist, seed=401, nq=20, nb=nb, ragged=False)
    zero = np.zeros((1, d), np.float32)
    xb1 = xb.copy()
    xb1[77] = 0
    lists = oracle.Lists(metric, cen, xb1, assign)
    h = make_handle(capi, metric, cen, xb1, assign)
    last, det = wcheck(oracle, h, lists, zero, 1, "zero query, one zero vector")
    if metric == L2:  # distance and threshold are both 0 and the bound has no slack: a strict keep test drops the answer
        assert last[:3] == (1, 0, 0) and det[2] == 1, (last, det)
    wcheck(oracle, h, lists, np.concatenate([zero, xq, zero]), 1, "zero queries among others")
    h.close()
    k = 3
    xb2 = xb.copy()
    where = np.array([10, 500, 901, 1502])
    xb2[where] = 0
    assert len(set(assign[where])) > 1
    lists = oracle.Lists(metric, cen, xb2, assign)
    h = make_handle(capi, metric, cen, xb2, assign)
    last, det = wcheck(oracle, h, lists, zero, k, "k + 1 zero vectors")
    if metric == L2:
        assert last[:3] == (0, 1, 0) and det[2] == k + 1, (last, det)
    wcheck(oracle, h, lists, np.concatenate([xq, zero]), k, "k + 1 zero vectors, more queries")
    h.close()


# ------------------------------------------------------------------------------------------ f
WIDE_BOUND_CASES = __import__("exact_wide_cases").BOUND_CASES


@pytest.mark.parametrize("depth", ["tight", "mid"])
@pytest.mark.parametrize("metric,d,W,mid,seed", WIDE_BOUND_CASES)
def test_the_bound_on_coherently_rounded_data(capi, oracle, metric, d, W, mid, seed, depth):
    """test_gpu_filter_bound.py's check of the exact float pass, for the wide pass: the result is the oracle's, the pass answers
    exactly the queries without a tie, and the candidates left after rescoring are the reference's entries at or within the seed's k-th"""
    N, K, NLIST = fb.N, fb.K, fb.NLIST
    c = fb.case(metric, d, W, seed=seed)
    s = fb.TIGHT if depth == "tight" else mid
    lists = oracle.Lists(metric, c.cen, c.xb, c.assign, c.ids)
    keys, zeros = np.tile(np.arange(NLIST, dtype=np.int64), (N, 1)), np.zeros((N, NLIST), np.float32)
    all_D, _, _ = oracle.search_preassigned(lists, c.xq, len(c.xb), keys, zeros)
    eD, eI, _ = oracle.search_preassigned(lists, c.xq, K, keys, zeros)
    b = bits(all_D[:, :K + 1])
    ties = int((b[:, 1:] == b[:, :-1]).any(axis=1).sum())
    cd, ck = oracle.knn(metric, c.xq, c.cen, s)
    sD, sI, _ = oracle.search_preassigned(lists, c.xq, K, ck, cd)
    assert (sI[:, K - 1] >= 0).all()
    valid = int(fb.within(metric, all_D, sD[:, K - 1]).sum())
    h = make_handle(capi, metric, c.cen, c.xb, c.assign)
    h.set_option("exact_seed_nprobe", s)
    D, I = h.search_exact(c.xq, K)
    last, det = h.last_exact(), h.last_exact_detail()
    bad = np.nonzero((I != eI).any(axis=1) | (bits(D) != bits(eD)).any(axis=1))[0]
    print((metric, d, W, depth), "seed depth", s, "last_exact", last, "detail", det, "reference: ties", ties, "valid", valid, "wrong queries", bad.size)
    assert bad.size == 0, ("queries", bad[:8], I[bad[0]], eI[bad[0]])
    assert det[0] == 3, "the call did not take the wide fp16 pass"
    assert last[2] == 0, "queries left the pass for another reason than a tie: candidates were dropped"
    assert last[0] == N - ties and last[1] == ties
    assert det[2] == valid, "the candidates at or within the threshold are not the reference's"
    assert det[1] >= det[2] and det[1] == last[3]
    assert det[3] <= fb.CAP // 4
    h.close()


# ------------------------------------------------------------------------------------------ g
def test_under_a_selector(capi, oracle):
    d, nlist, k, metric = 200, 32, 10, L2
    cen, assign, xb, xq = float_case(d, nlist, seed=1700, nq=150, nb=NB)
    h = make_handle(capi, metric, cen, xb, assign)
    h.set_option("exact_seed_nprobe", 4)  # 32 lists: twice four stays below them
    model = Model(nlist, d, xb, assign)
    nwords = (NB + 63) // 64 + 2
    rs = np.random.RandomState(5)
    half = np.nonzero(rs.rand(NB) < 0.5)[0]
    member = np.zeros(NB, bool)
    member[half] = True
    specs = {
        "mod_2": ((capi.SUBSET_ID_MOD, 2, 0, None), lambda ids, l, seen: np.fmod(ids, 2) == 0),
        "bits_half": ((capi.SUBSET_ID_BITS, 0, 0, id_bits(half, nwords)), lambda ids, l, seen: member[ids]),
        "bits_all": ((capi.SUBSET_ID_BITS, 0, 0, id_bits(np.arange(NB), nwords)), lambda ids, l, seen: np.ones(len(ids), bool)),
    }
    for name, (spec, rule) in specs.items():
        last, det, D, I = sel_check(oracle, capi, h, metric, cen, model, spec, rule, xq, k, name)
        print(name, "last_exact", last, "detail", det)
        assert det[0] == 3 and last[0] > 0, (name, last, det)
        if name == "bits_all":  # every entry is a member: the unfiltered call, bit for bit and candidate for candidate
            uD, uI = h.search_exact(xq, k)
            assert np.array_equal(uI, I) and np.array_equal(bits(uD), bits(D))
            assert h.last_exact() == last and h.last_exact_detail() == det
    h.close()


def test_a_tie_between_a_member_and_a_non_member_is_no_tie(capi, oracle):
    """every second vector is stored twice, the copy under an id beyond nb in another list; the selector keeps the ids below nb"""
    d, nlist, nb, n, k, metric = 200, 64, 3000, 100, 10, L2
    cen, assign, xb, xq = float_case(d, nlist, seed=1800, nq=n, nb=nb, ragged=False)
    twice = np.arange(0, nb, 2)
    xb2 = np.concatenate([xb, xb[twice]])
    assign2 = np.concatenate([assign, (assign[twice] + 5) % nlist])
    lists = oracle.Lists(metric, cen, xb2, assign2)
    tied_all = int(oracle_ties(oracle, lists, xq, k).sum())
    tied_members = int(oracle_ties(oracle, oracle.Lists(metric, cen, xb, assign), xq, k).sum())
    assert tied_all > tied_members
    h = make_handle(capi, metric, cen, xb2, assign2)
    last, det = wcheck(oracle, h, lists, xq, k, "stored twice")
    assert last[1] == tied_all and last[2] == 0, (last, tied_all)
    model = Model(nlist, d, xb2, assign2)
    spec, rule = (capi.SUBSET_ID_RANGE, 0, nb, None), lambda ids, l, seen: ids < nb
    last, det, _, _ = sel_check(oracle, capi, h, metric, cen, model, spec, rule, xq, k, "members only")
    assert det[0] == 3 and last[1] == tied_members and last[2] == 0, (last, det, tied_members)
    h.close()


# ------------------------------------------------------------------------------------------ h
@pytest.mark.parametrize("what", ["exact_wide_unset", "exact_float_0", "filter_1", "d_1028", "list_row_tiny", "query_row_tiny"])
def test_a_call_that_does_not_qualify_goes_the_general_way_whole(capi, oracle, what):
    n, k, metric = 40, 10, L2
    d = 1028 if what == "d_1028" else 200
    cen, assign, xb, xq = float_case(d, 16, seed=501, nq=n, nb=3000)
    if what == "list_row_tiny":
        xb[1234] *= np.float32(2.0 ** -20)
    if what == "query_row_tiny":
        xq[7] *= np.float32(2.0 ** -20)
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    if what == "exact_wide_unset":
        h.set_option("exact_wide", float("nan"))
        assert h.get_option("exact_wide") == 0
    if what == "exact_float_0":
        h.set_option("exact_float", 0)
    if what == "filter_1":
        h.set_option("filter", 1)
    wcheck(oracle, h, lists, xq, k, what, kind=0)
    if what == "query_row_tiny":  # the rule is the call's: the other queries alone take the pass
        wcheck(oracle, h, lists, xq[8:], k, what + ", other queries")
    if what == "exact_wide_unset":
        h.set_option("exact_wide", 1)
        assert wcheck(oracle, h, lists, xq, k, what + ", on")[0][0] > 0
    if what == "exact_float_0":
        h.set_option("exact_float", 1)
        assert wcheck(oracle, h, lists, xq, k, what + ", on")[0][0] > 0
    h.close()


def test_byte_coded_lists_beyond_128_dimensions(capi, oracle):
    metric, cen, assign, xb, xq = make_case("bytes_200")
    n, k = 40, 10
    xq = xq[:n]
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    wcheck(oracle, h, lists, xq, k, "byte codes in use", kind=0)
    h.close()
    h = make_handle(capi, metric, cen, xb, assign)
    h.set_byte_codes(0)
    last, det = wcheck(oracle, h, lists, xq, k, "byte codes off")
    assert last[0] + last[1] == n and last[2] == 0, (last, det)
    h.close()


# ------------------------------------------------------------------------------------------ i
def test_after_changes_on_a_clone_resident_and_reused_buffers(capi, oracle):
    d, nlist, metric, k = 160, 16, L2, 10
    cen, assign, xb, xq = float_case(d, nlist, seed=1900, nq=256, nb=3000, ragged=False)
    rs = np.random.RandomState(5)
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(nlist, d, xb, assign)

    def lists_now():
        fx, fa, fi = model.flat()
        return oracle.Lists(metric, cen, fx, fa, fi)

    def near(to):
        return (cen[to] + 0.3 * rs.randn(len(to), d)).astype(np.float32)

    assert wcheck(oracle, h, lists_now(), xq[:70], k, "before")[0][0] > 0
    to = np.array([2] * 40 + [3, 7, 7], np.int64)
    x = near(to)
    ids = np.arange(50000, 50000 + len(to), dtype=np.int64)
    h.add(x, ids, to)  # the journal is pending when the exact call starts; the fp16 copy follows it
    model.add(x, ids, to)
    last, _ = wcheck(oracle, h, lists_now(), xq[:70], k, "add")
    assert last[0] > 0 and h.last_update()[0] == 1
    sel = [model.ids[3][1], model.ids[3][-1]] + list(model.ids[9][:50])
    assert h.remove_ids(np.array(sel)) == model.remove_ids(sel)
    wcheck(oracle, h, lists_now(), xq[:70], k, "remove")
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
    wcheck(oracle, h, lists, xq[:70], k, "update_lists")
    c = h.clone()
    assert wcheck(oracle, c, lists, xq[:130], k, "clone")[0][0] > 0
    eD, eI = expected(oracle, lists, xq, k)
    for ctx in (h, c):
        ctx.set_queries(xq)
        D, I = ctx.search_exact_resident(37, 150, k)
        assert np.array_equal(I, eI[37:187]) and np.array_equal(bits(D), bits(eD[37:187]))
        assert sum(ctx.last_exact()[:3]) == 150 and ctx.last_exact()[0] > 0 and ctx.last_exact_detail()[0] == 3
    c.close()
    for n, kk in ((20, 10), (256, 64), (7, 10), (200, 1), (64, 100)):  # a larger call, then a smaller one: the workspaces are reused
        wcheck(oracle, h, lists, xq[:n], kk, ("reuse", n, kk))
    h.close()


# ------------------------------------------------------------------------------------------ j
WIDE_ENV = {"AUNCEL_AMD_EXACT_FLOAT": "1", "AUNCEL_AMD_EXACT_WIDE": "1"}


def test_candidate_overflow_in_a_child_process(oracle, tmp_path):
    """AUNCEL_AMD_EXACT_CAP=16: with k = 10 and a threshold from an eighth of the lists of unclustered data, queries overflow their slots"""
    cen, assign, xb, xq = float_case(136, 32, seed=61, clustered=False, nq=200, nb=NB)
    calls = [dict(name=f"m{m}", metric=m, cen="cen", xb="xb", assign="assign", xq="xq", k=10) for m in (L2, IP)]
    out = run_child(tmp_path, dict(WIDE_ENV, AUNCEL_AMD_EXACT_CAP="16", AUNCEL_AMD_EXACT_SEED="4"), calls, dict(cen=cen, xb=xb, assign=assign, xq=xq))
    for m in (L2, IP):
        eD, eI = expected(oracle, oracle.Lists(m, cen, xb, assign), xq, 10)
        last = out[f"m{m}/last"]
        print("cap 16, metric", m, "last_exact", last)
        assert np.array_equal(out[f"m{m}/I"], eI) and np.array_equal(bits(out[f"m{m}/D"]), bits(eD))
        assert last[2] > 0 and last[:3].sum() == len(xq) and last[3] > 0, last  # (candidates were emitted: the pass ran)


def test_a_loose_seed_in_a_child_process(oracle, tmp_path):
    """AUNCEL_AMD_EXACT_SEED=1 on clustered data: the threshold comes from one list, many candidates per query"""
    cen, assign, xb, xq = float_case(136, 32, seed=71, nq=200, nb=NB)
    calls = [dict(name=f"m{m}", metric=m, cen="cen", xb="xb", assign="assign", xq="xq", k=10) for m in (L2, IP)]
    out = run_child(tmp_path, dict(WIDE_ENV, AUNCEL_AMD_EXACT_SEED="1"), calls, dict(cen=cen, xb=xb, assign=assign, xq=xq))
    for m in (L2, IP):
        eD, eI = expected(oracle, oracle.Lists(m, cen, xb, assign), xq, 10)
        last = out[f"m{m}/last"]
        print("seed 1, metric", m, "last_exact", last)
        assert np.array_equal(out[f"m{m}/I"], eI) and np.array_equal(bits(out[f"m{m}/D"]), bits(eD))
        assert last[:3].sum() == len(xq) and last[0] > 0 and last[3] >= last[0] * 10, last


# ------------------------------------------------------------------------------------------ k
def test_a_narrow_call_with_the_option_set_takes_the_narrow_pass(capi, oracle):
    cen, assign, xb, xq = float_case(96, 16, seed=41, nq=130, nb=NB)
    lists = oracle.Lists(IP, cen, xb, assign)
    h = plain_handle(capi, IP, cen, xb, assign)
    h.set_option("exact_float", 1)
    off = fcheck(oracle, h, lists, xq, 10, "exact_wide unset", kind=2)
    h.set_option("exact_wide", 1)
    on = fcheck(oracle, h, lists, xq, 10, "exact_wide 1", kind=2)
    assert on == off, (on, off)
    h.close()
