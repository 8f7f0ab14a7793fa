"""Exact k-NN and exact range search over byte-coded lists beyond 128 dimensions (option "exact_wide_bytes": scan_all_wide_i8_kernel,
DESIGN.md 13.5).  (D, I) are, bit for bit, the pinned CPU oracle's search_preassigned over every list in list-number order -- and what
amd_ivf_search_preassigned returns for those keys on the same handle -- and every served call reports pass 4:
  a. the piece counts and stage edges of the tile (d = 132, 192, 200, 384, 960, 1024 at d m^2 = 2^24), ragged lists, batches around the
     query block and the 128-query tile; at least half of every batch is answered by the pass
  b. the chunk tail: block streams of 16, 14 and 2 blocks
  c. rows that differ in the last eight dimensions only
  d. the pass serves exactly the queries without equal distances in their window (values 0 .. 8)
  e. a zero query against stored zero vectors; k beyond a selector's members
  f. under a selector (the KEEP form)
  g. the exact range search, its resident and selected forms
  h. calls that do not qualify are decided as they were
  i. after changes of the lists, on a clone, resident queries, reused buffers
  j. candidate overflow and a loose seed in child processes
The data is exact_wide_bytes_cases.py's; test_exact_wide_bytes_cpu.py asserts what these tests lean on (the byte rule, the tie counts,
the candidate counts) with exact integers."""
import numpy as np
import pytest

import exact_wide_bytes_cases as wb
from test_gpu_exact import IP, L2, bits, byte_case, check, expected, identity_keys, run_child
from test_gpu_exact import make_handle as plain_handle
from test_gpu_exact_float import fcheck, oracle_ties
from test_gpu_exact_range import check as range_check
from test_gpu_exact_range import emitted, inside, int_dis, same, want
from test_gpu_exact_selected import check as sel_check
from test_gpu_subset import filtered, id_bits, oracle_lists
from test_gpu_update import Model, make_case
from test_gpu_wide_bytes import limit_m, make_lists

pytestmark = pytest.mark.gpu

KIND = 4


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
    h.set_option("exact_wide_bytes", 1)
    return h


def bcheck(oracle, h, lists, xq, k, what="", kind=KIND):
    return fcheck(oracle, h, lists, xq, k, what, kind=kind)


# ------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", wb.STAGE_D)
def test_exact_equals_oracle_at_every_stage_edge(capi, oracle, d, metric):
    cen, assign, xb, xq = wb.stage_case(d, metric)
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    for n, k in wb.BATCHES:
        last, det = bcheck(oracle, h, lists, xq[:n], k, (d, metric, n, k))
        print(d, metric, n, k, "last_exact", last, "detail", det)
        assert 2 * last[0] >= n and last[2] == 0, (n, k, last, det)
        assert det[2] == det[1] >= last[0] * k, (last, det)  # (the byte pass emits nothing beyond the threshold)
    assert h.scan_arith() == 2
    h.close()


# ------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("sizes,nblk", wb.TAIL_SIZES, ids=["nblk_16", "nblk_14", "nblk_2"])
def test_the_chunk_tail(capi, oracle, sizes, nblk, metric):
    k = 10
    cen, assign, xb, xq, last_list = wb.tail_case(sizes, metric)
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)  # (the seed probes every list: the threshold is the true k-th distance)
    last, det = bcheck(oracle, h, lists, xq, k, (sizes, metric))
    eD, eI = expected(oracle, lists, xq, k)
    assert (assign[eI] == last_list).all()  # the neighbours are entries of the last list, whose blocks are the stream's last
    tied, within = wb.ties_within(metric, xb, xq, k)
    assert last[:3] == (len(xq) - int(tied.sum()), int(tied.sum()), 0) and 2 * last[0] >= len(xq), (last, det)
    assert det[2] == int(within.sum()), (last, det, int(within.sum()))
    h.close()


# ------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [200, 192])
def test_the_last_dimensions_decide(capi, oracle, d, metric):
    """d = 200: dimensions 192 .. 199, the only real ones of piece 6 of 7 -- the first piece of the second stage; a kernel that skips
    the last stage's real piece sees every row of a list at one distance.  d = 192: dimensions 184 .. 191 in piece 5 of 6, the LAST
    piece of the only stage, which is full"""
    k = 10
    cen, assign, xb, xq = wb.last_dims_case(d, metric)
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    last, det = bcheck(oracle, h, lists, xq, k, "last dimensions")
    tied, within = wb.ties_within(metric, xb, xq, k)
    print(d, metric, "ties", int(tied.sum()), "last_exact", last, "detail", det)
    assert last[:3] == (len(xq) - int(tied.sum()), int(tied.sum()), 0) and 2 * last[0] >= len(xq), (last, det)
    assert det[2] == int(within.sum()), (last, det)
    h.close()


# ------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("metric", [L2, IP])
def test_the_pass_serves_exactly_the_queries_without_ties(capi, oracle, metric):
    n, k = 200, 5
    cen, assign, xb, xq, tied, within = wb.small_range_case(metric, n, k)
    ties = int(tied.sum())
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    last, det = bcheck(oracle, h, lists, xq, k, "values 0 .. 8")
    print(metric, "numpy ties", ties, "last_exact", last, "detail", det)
    assert last[:3] == (n - ties, ties, 0) and 2 * last[0] >= n, (last, ties, det)
    assert det[2] == int(within.sum()), (det, int(within.sum()))
    h.close()


# ------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("metric", [L2, IP])
def test_zero_query_and_zero_vectors(capi, oracle, metric):
    d = 136
    cen, assign, xb, xq = byte_case(d, 16, seed=401, nq=20, nb=2000)
    zero = np.zeros((1, d), np.float32)
    xb[77] = 0
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    last, det = bcheck(oracle, h, lists, zero, 1, "zero query, one zero vector")
    if metric == L2:  # distance and threshold are both 0: a strict keep test drops the answer
        assert last[:3] == (1, 0, 0) and det[2] == 1, (last, det)
    bcheck(oracle, h, lists, np.concatenate([zero, xq, zero]), 1, "zero queries among others")
    h.close()


def test_k_beyond_the_members_of_a_selector(capi, oracle):
    d, nlist, k, metric = 200, 16, 10, L2
    cen, assign, xb, xq = byte_case(d, nlist, seed=402, nq=40, nb=2000)
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(nlist, d, xb, assign)
    spec, rule = (capi.SUBSET_ID_RANGE, 100, 106, None), lambda ids, l, seen: (ids >= 100) & (ids < 106)
    last, det, D, I = sel_check(oracle, capi, h, metric, cen, model, spec, rule, xq, k, "six members", subset=False)
    assert (I[:, 6:] == -1).all() and (I[:, :6] >= 100).all() and last == (0, 0, len(xq), 0) and det[0] == 0, (last, det)
    h.close()


# ------------------------------------------------------------------------------------------ f
def test_under_a_selector(capi, oracle):
    d, nlist, k, metric, nb = 200, 32, 10, L2, 4000
    cen, assign, xb, xq = byte_case(d, nlist, seed=1700, nq=150, nb=nb)
    h = make_handle(capi, metric, cen, xb, assign)
    h.set_option("exact_seed_nprobe", 4)  # 32 lists: twice four stays below them
    model = Model(nlist, d, xb, assign)
    nwords = (nb + 63) // 64 + 2
    rs = np.random.RandomState(5)
    half = np.nonzero(rs.rand(nb) < 0.5)[0]
    member = np.zeros(nb, bool)
    member[half] = True
    specs = {
        "mod_2": ((capi.SUBSET_ID_MOD, 2, 0, None), lambda ids, l, seen: np.fmod(ids, 2) == 0),
        "bits_half": ((capi.SUBSET_ID_BITS, 0, 0, id_bits(half, nwords)), lambda ids, l, seen: member[ids]),
        "bits_all": ((capi.SUBSET_ID_BITS, 0, 0, id_bits(np.arange(nb), nwords)), lambda ids, l, seen: np.ones(len(ids), bool)),
    }
    for name, (spec, rule) in specs.items():
        last, det, D, I = sel_check(oracle, capi, h, metric, cen, model, spec, rule, xq, k, name)
        print(name, "last_exact", last, "detail", det)
        assert det[0] == KIND and 2 * last[0] >= len(xq), (name, last, det)
        if name == "bits_all":  # every entry is a member: the unfiltered call, bit for bit and candidate for candidate
            uD, uI = h.search_exact(xq, k)
            assert np.array_equal(uI, I) and np.array_equal(bits(uD), bits(D))
            assert h.last_exact() == last and h.last_exact_detail() == det
    h.close()


def test_a_tie_between_a_member_and_a_non_member_is_no_tie(capi, oracle):
    """every second vector is stored twice, the copy under an id beyond nb in another list; the selector keeps the ids below nb"""
    d, nlist, nb, n, k, metric = 200, 64, 3000, 100, 10, L2
    rs = np.random.RandomState(1800)
    cen = rs.randint(0, 256, size=(nlist, d)).astype(np.float32)
    assign = rs.randint(0, nlist, size=nb)
    xb = np.clip(cen[assign] + rs.randint(-31, 32, size=(nb, d)), 0, 255).astype(np.float32)
    xq = np.clip(cen[rs.randint(0, nlist, size=n)] + rs.randint(-31, 32, size=(n, d)), 0, 255).astype(np.float32)
    twice = np.arange(0, nb, 2)
    xb2 = np.concatenate([xb, xb[twice]])
    assign2 = np.concatenate([assign, (assign[twice] + 5) % nlist])
    lists = oracle.Lists(metric, cen, xb2, assign2)
    tied_all = int(oracle_ties(oracle, lists, xq, k).sum())
    tied_members = int(oracle_ties(oracle, oracle.Lists(metric, cen, xb, assign), xq, k).sum())
    assert tied_all > tied_members and 2 * tied_members <= n
    h = make_handle(capi, metric, cen, xb2, assign2)
    last, det = bcheck(oracle, h, lists, xq, k, "stored twice")
    assert last[1] == tied_all and last[2] == 0, (last, tied_all)
    model = Model(nlist, d, xb2, assign2)
    spec, rule = (capi.SUBSET_ID_RANGE, 0, nb, None), lambda ids, l, seen: ids < nb
    last, det, _, _ = sel_check(oracle, capi, h, metric, cen, model, spec, rule, xq, k, "members only")
    assert det[0] == KIND and last[1] == tied_members and last[2] == 0 and 2 * last[0] >= n, (last, det, tied_members)
    h.close()


# ------------------------------------------------------------------------------------------ g
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [200, 960])
def test_the_exact_range_search(capi, oracle, d, metric):
    cen, assign, xb, xq = wb.range_case(d, metric)
    n = len(xq)
    dis = int_dis(metric, xb, xq)
    v = float(np.sort(dis[0])[15] if metric == L2 else -np.sort(-dis[0])[15])  # a stored integer distance of query 0
    at = int((dis[0] == v).sum())
    below = float(dis.min() if metric == L2 else dis.max())  # no entry is strictly within it
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    last, exp = range_check(oracle, h, lists, xq, below, ("below every distance", d, metric))
    assert exp[0][-1] == 0 and last[:3] == (KIND, n, 0), last
    last, exp = range_check(oracle, h, lists, xq, v, ("at a stored distance", d, metric))
    assert np.array_equal(np.diff(exp[0]), inside(metric, dis, v).sum(1))
    assert int(emitted(metric, dis[0], v).sum() - inside(metric, dis[0], v).sum()) == at >= 1
    assert last[:3] == (KIND, n, 0) and last[3] == int(emitted(metric, dis, v).sum(1).max()), last
    last, exp = range_check(oracle, h, lists, xq[:5], float("inf"), ("+inf", d, metric))
    assert last[0] == KIND and exp[0][-1] == (5 * len(xb) if metric == L2 else 0), last
    # the resident form over a slice that does not start at 0
    exp = want(oracle, lists, xq[7:30], v)
    h.set_queries(xq)
    assert same(h.range_search_exact_resident(7, 23, v), exp)
    assert h.last_range_exact()[:3] == (KIND, 23, 0)
    # the selected form: the members alone
    model = Model(cen.shape[0], d, xb, assign)
    rule = lambda ids, l, seen: np.fmod(ids, 2) == 0
    exp = want(oracle, oracle_lists(oracle, metric, cen, filtered(model, rule)), xq, v)
    with h.selector(capi.SUBSET_ID_MOD, 2, 0, None) as s:
        assert same(h.range_search_exact_selected(s, xq, v), exp)
        assert h.last_range_exact()[:3] == (KIND, n, 0)
        assert same(h.range_search_selected(s, xq, v, cen.shape[0], keys=identity_keys(n, cen.shape[0])), exp)
    h.close()


# ------------------------------------------------------------------------------------------ h
@pytest.mark.parametrize("what", ["unset", "zero", "byte_codes_off", "query_256", "query_beyond_the_rule"])
def test_a_call_that_does_not_qualify_is_decided_as_before(capi, oracle, what):
    n, k, metric = 40, 10, L2
    d = 960 if what == "query_beyond_the_rule" else 200
    cen, assign, xb, xq = byte_case(d, 16, seed=501, top=limit_m(d), nq=n, nb=3000)
    if what == "query_256":
        xq[5, 3] = 256.0
    if what == "query_beyond_the_rule":
        assert limit_m(d) == 132
        xq[5, 3] = 133.0  # a byte, but 960 x 133^2 > 2^24
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    if what == "unset":
        h.set_option("exact_wide_bytes", float("nan"))
        assert h.get_option("exact_wide_bytes") == 0
    if what == "zero":
        h.set_option("exact_wide_bytes", 0)
    if what == "byte_codes_off":
        h.set_byte_codes(0)
    bcheck(oracle, h, lists, xq, k, what, kind=0)
    if what in ("query_256", "query_beyond_the_rule"):  # the rule is the call's: the other queries alone take the pass
        assert bcheck(oracle, h, lists, xq[6:], k, what + ", other queries")[0][0] > 0
    if what in ("unset", "zero"):
        h.set_option("exact_wide_bytes", 1)
        assert bcheck(oracle, h, lists, xq, k, what + ", on")[0][0] > 0
    if what == "byte_codes_off":  # ... and as a call over float lists is: the wide fp16 pass, if its options ask for it
        h.set_option("exact_float", 1)
        h.set_option("exact_wide", 1)
        assert bcheck(oracle, h, lists, xq, k, what + ", the fp16 options", kind=3)[0][0] > 0
    h.close()


def test_the_wide_bytes_helpers_of_the_byte_scan_tests(capi, oracle):
    """test_gpu_wide_bytes.py's lists at the edge of the rule (d = 384, m = 209: clustered and uniform rows, duplicated rows, rows one
    step away from them, the row of all m), lengths 0 .. 1300"""
    d, metric = 384, L2
    t = make_lists(d, limit_m(d), metric, seed=91)
    rs = np.random.RandomState(92)
    xq = t.xb[rs.choice(len(t.xb), 100, replace=False)].copy()
    xq[:, :7] = np.clip(xq[:, :7] + rs.randint(-3, 4, size=(100, 7)), 0, t.m)
    lists = oracle.Lists(metric, t.cen, t.xb, t.assign)
    h = make_handle(capi, metric, t.cen, t.xb, t.assign)
    last, det = bcheck(oracle, h, lists, xq, 10, "edge of the rule")
    tied, within = wb.ties_within(metric, t.xb, xq, 10)
    assert last[:3] == (100 - int(tied.sum()), int(tied.sum()), 0) and det[2] == int(within.sum()), (last, det)
    h.close()


def test_a_narrow_call_with_the_option_set_takes_the_narrow_pass(capi, oracle):
    cen, assign, xb, xq = byte_case(128, 16, seed=41, nq=130, nb=4000)
    lists = oracle.Lists(IP, cen, xb, assign)
    h = plain_handle(capi, IP, cen, xb, assign)
    off = fcheck(oracle, h, lists, xq, 10, "exact_wide_bytes unset", kind=1)
    h.set_option("exact_wide_bytes", 1)
    on = fcheck(oracle, h, lists, xq, 10, "exact_wide_bytes 1", kind=1)
    assert on == off, (on, off)
    h.close()


# ------------------------------------------------------------------------------------------ i
def test_after_changes_on_a_clone_resident_and_reused_buffers(capi, oracle):
    metric, cen, assign, xb, xq = make_case("bytes_200")
    nlist, d = cen.shape
    k = 10
    rs = np.random.RandomState(5)
    top = int(max(xb.max(), xq.max()))
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(nlist, d, xb, assign)

    def lists_now():
        fx, fa, fi = model.flat()
        return oracle.Lists(metric, cen, fx, fa, fi)

    def near(to):
        return np.clip(cen[to] + rs.randint(-20, 21, size=(len(to), d)), 0, top).astype(np.float32)

    assert bcheck(oracle, h, lists_now(), xq[:70], k, "before")[0][0] > 0
    to = np.array([2] * 40 + [3, 7, 7], np.int64)
    x = near(to)
    ids = np.arange(50000, 50000 + len(to), dtype=np.int64)
    h.add(x, ids, to)  # the journal is pending when the exact call starts
    model.add(x, ids, to)
    last, _ = bcheck(oracle, h, lists_now(), xq[:70], k, "add")
    assert last[0] > 0 and h.last_update()[0] == 1
    sel = [model.ids[3][1], model.ids[3][-1]] + list(model.ids[9][:50])
    assert h.remove_ids(np.array(sel)) == model.remove_ids(sel)
    bcheck(oracle, h, lists_now(), xq[:70], k, "remove")
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
    bcheck(oracle, h, lists, xq[:70], k, "update_lists")
    c = h.clone()
    assert bcheck(oracle, c, lists, xq[:130], k, "clone")[0][0] > 0
    eD, eI = expected(oracle, lists, xq, k)
    lo, cnt = 37, min(150, len(xq) - 37)
    for ctx in (h, c):
        ctx.set_queries(xq)
        D, I = ctx.search_exact_resident(lo, cnt, k)
        assert np.array_equal(I, eI[lo:lo + cnt]) and np.array_equal(bits(D), bits(eD[lo:lo + cnt]))
        assert sum(ctx.last_exact()[:3]) == cnt and ctx.last_exact()[0] > 0 and ctx.last_exact_detail()[0] == KIND
    c.close()
    nq = len(xq)
    for n, kk in ((20, 10), (nq, 64), (7, 10), (min(200, nq), 1), (64, 100)):  # a larger call, then a smaller one: the workspaces are reused
        bcheck(oracle, h, lists, xq[:n], kk, ("reuse", n, kk))
    h.close()


# ------------------------------------------------------------------------------------------ j
WIDE_ENV = {"AUNCEL_AMD_EXACT_WIDE_BYTES": "1"}


def test_candidate_overflow_in_a_child_process(oracle, tmp_path):
    """AUNCEL_AMD_EXACT_CAP=16: with k = 10 and a threshold from an eighth of the lists of unclustered data, queries overflow their slots"""
    cen, assign, xb, xq = byte_case(136, 32, seed=61, clustered=False, nq=200, nb=4000)
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
    cen, assign, xb, xq = byte_case(136, 32, seed=71, nq=200, nb=4000)
    calls = [dict(name=f"m{m}", metric=m, cen="cen", xb="xb", assign="assign", xq="xq", k=10) for m in (L2, IP)]
    out = run_child(tmp_path, dict(WIDE_ENV, AUNCEL_AMD_EXACT_SEED="1"), calls, dict(cen=cen, xb=xb, assign=assign, xq=xq))
    for m in (L2, IP):
        eD, eI = expected(oracle, oracle.Lists(m, cen, xb, assign), xq, 10)
        last = out[f"m{m}/last"]
        print("seed 1, metric", m, "last_exact", last)
        assert np.array_equal(out[f"m{m}/I"], eI) and np.array_equal(bits(out[f"m{m}/D"]), bits(eD))
        assert last[:3].sum() == len(xq) and last[0] > 0 and last[3] >= last[0] * 10, last
