"""The byte-code scan over its whole domain: d > 128 (the "any d" form scan_mfma_kernel<METRIC, MASKED, 0>, which is the only byte
kernel once a row needs more than four K-steps) and the edge of the eligibility rule d * m^2 <= 2^24, m the largest value over
lists and queries.

Two references, independent of each other and of the engine:
  * the pinned CPU oracle (the reference's fp32 rounding sequence): (D, I), range results, my_nprobe and the statistics, bit for bit;
  * exact integer arithmetic (|x|^2 + |y|^2 - 2 x.y, or x.y, as int64): every returned (query, id) carries float32 of that integer,
    and every row's distances are the brute-force top-k over the probed lists.  On eligible data no partial sum of the reference
    passes 2^24, so this is the same number; it would catch an oracle and a kernel that were wrong together.
Every comparison is of bit patterns or of integers.  The first test holds the premise (the two references agree) without a GPU.

List and query geometry follows test_gpu_pair_scan.py, where work items change shape: list lengths around 32 / 64 / 512 and one
list of several chunks, lists probed by 1 .. ~200 queries, calls of 1, 19, 70 and 513 queries."""
import math
import os

import numpy as np
import pytest

# AUNCEL_TEST_SEED_OFFSET=<n>: the sweep's 60 shapes drawn from other seeds (one-off fuzzing after kernel changes)
SEED_OFFSET = int(os.environ.get("AUNCEL_TEST_SEED_OFFSET", "0"))

gpu = pytest.mark.gpu

LIMIT = 1 << 24
# (d, m): m the largest value on either side; d m^2 <= 2^24 < d (m + 1)^2, except where m = 255 is the type's limit
SHAPES = [(129, 255), (136, 255), (160, 255), (161, 255), (200, 255), (256, 255), (257, 255), (258, 255), (259, 254), (384, 209),
          (960, 132), (1024, 128), (4096, 64)]
METRICS = [1, 0]  # L2, IP
LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1300]  # the last one: several chunks of a dense and of a threshold round
PROBED_BY = [3, 2, 32, 33, 64, 65, 200, 1, 33, 65, 64, 200]    # queries that probe each list (as far as the call has that many)
BIG = np.iinfo(np.int64).max


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def limit_m(d):
    """the largest byte value m with d m^2 <= 2^24"""
    return min(255, math.isqrt(LIMIT // d))


def exact_table(metric, xq, xb):
    """int64 distances of every query to every row.  The products are summed by a float64 matrix product: every partial sum is an
    integer below 2^53, so each is exact in any order; the result is checked to be integral and the rest is int64."""
    g = xq.astype(np.float64) @ xb.astype(np.float64).T
    gi = g.astype(np.int64)
    assert np.array_equal(gi, g)
    if metric == 0:
        return gi
    qi, yi = xq.astype(np.int64), xb.astype(np.int64)
    return (qi * qi).sum(1)[:, None] + (yi * yi).sum(1)[None, :] - 2 * gi


def probed_mask(keys, assign, nlist, max_codes=0):
    """(nq, nb) bool: the rows a query scans -- its keys >= 0, and with max_codes the lists that start before the budget is used
    (IndexIVF::search_preassigned: nscan += list size; stop once nscan >= max_codes)"""
    live = keys >= 0
    if max_codes:
        sizes = np.bincount(assign, minlength=nlist)
        sz = np.where(live, sizes[np.clip(keys, 0, None)], 0)
        live = live & (np.cumsum(sz, axis=1) - sz < max_codes)
    hit = np.zeros((keys.shape[0], nlist), bool)
    q, p = np.nonzero(live)
    hit[q, keys[q, p]] = True
    return hit[:, assign]


def rows_of_pairs(I, assign, nlist):
    """store_pairs labels (list << 32 | offset) -> database rows (-1 stays)"""
    order = np.argsort(assign, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nlist))])
    out = np.full(I.shape, -1, np.int64)
    ok = I >= 0
    out[ok] = order[off[I[ok] >> 32] + (I[ok] & 0xffffffff)]
    return out


def topk_table(metric, E, probed, k):
    """the brute-force top-k of every query over its probed rows: (values, how many there are)"""
    v = np.where(probed, E, BIG if metric == 1 else -BIG)
    top = np.sort(v, axis=1)[:, :k] if metric == 1 else -np.sort(-v, axis=1)[:, :k]
    if top.shape[1] < k:
        top = np.concatenate([top, np.zeros((top.shape[0], k - top.shape[1]), np.int64)], axis=1)
    return top, np.minimum(probed.sum(1), k)


def check_exact(metric, D, rows, E, probed, k, tag, skip_above=None, top=None):
    """(D, rows) of a search against the int64 table: float32 of the integer for every pair, a probed row each, no row twice, the
    brute-force top-k as the row's distances, -1 beyond the candidates.  skip_above: pairs whose exact value passes it are left to
    the oracle alone (there the reference's value depends on its summation order)"""
    ok = rows >= 0
    q = np.nonzero(ok)[0]
    val = E[q, rows[ok]]
    assert probed[q, rows[ok]].all(), tag
    cmp = np.ones(val.shape, bool) if skip_above is None else val <= skip_above
    assert np.array_equal(bits(D[ok])[cmp], bits(val.astype(np.float32))[cmp]), tag
    top, ncand = topk_table(metric, E, probed, k) if top is None else top
    there = np.arange(k)[None, :] < ncand[:, None]
    assert np.array_equal(ok, there), tag
    distinct = np.sort(np.where(there, rows, -1 - np.arange(k)[None, :]), axis=1)
    assert (np.diff(distinct, axis=1) != 0).all(), tag
    got = np.where(there, E[np.arange(D.shape[0])[:, None], np.clip(rows, 0, None)], 0)
    want = np.where(there, top, 0)
    if skip_above is not None:
        low = (want <= skip_above).all(1)
        got, want = got[low], want[low]
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (tag, "first query whose distances are not the brute-force top-k", int(bad[0]))


class Data:
    pass


def make_lists(d, m, metric, seed, lengths=LENGTHS):
    """clustered and uniform rows 0 .. m, a block of duplicated rows, rows one step away from them in one coordinate, and the row of
    all m (the single row of list 1, and one row of the long list)"""
    rs = np.random.RandomState(seed)
    t = Data()
    t.d, t.m, t.metric, t.nlist = d, m, metric, len(lengths)
    t.assign = rs.permutation(np.repeat(np.arange(t.nlist), lengths)).astype(np.int64)
    nb = len(t.assign)
    centre = rs.randint(0, m + 1, size=(t.nlist, d))
    t.cen = (centre + rs.uniform(-0.3, 0.3, size=centre.shape)).astype(np.float32)  # (non-integer: no exact coarse ties)
    spread = max(1, m // 8)
    xb = np.clip(centre[t.assign] + rs.randint(-spread, spread + 1, size=(nb, d)), 0, m)
    uni = np.nonzero(rs.rand(nb) < 0.3)[0]
    xb[uni] = rs.randint(0, m + 1, size=(len(uni), d))
    t.base = xb[rs.choice(nb, 6, replace=False)].copy()
    pick = rs.choice(nb, 80, replace=False)
    xb[pick[:40]] = t.base[rs.randint(0, 6, size=40)]
    for r in pick[40:]:
        row = t.base[rs.randint(0, 6)].copy()
        c = rs.randint(0, d)
        row[c] += 1 if row[c] < m else -1
        xb[r] = row
    for l in (1, t.nlist - 1):
        xb[np.nonzero(t.assign == l)[0][0]] = m
    t.xb = xb.astype(np.float32)
    t.centre = centre
    assert t.xb.min() >= 0 and t.xb.max() == m
    return t


def make_queries(t, nq, seed, probed_by=PROBED_BY):
    """queries near the list centres, copies of the duplicated rows and their neighbours; query 0 is the other end of the extreme
    pair (all 0 for L2, all m for IP) and probes list 1, whose single row is all m.  Keys: list l is probed by probed_by[l] queries."""
    rs = np.random.RandomState(seed)
    m, d, nlist = t.m, t.d, t.nlist
    spread = max(1, m // 8)
    xq = np.clip(t.centre[rs.randint(0, nlist, size=nq)] + rs.randint(-spread, spread + 1, size=(nq, d)), 0, m)
    for i in range(1, nq, 5):
        row = t.base[rs.randint(0, 6)].copy()
        if i % 2:
            c = rs.randint(0, d)
            row[c] += 1 if row[c] < m else -1
        xq[i] = row
    xq[0] = 0 if t.metric == 1 else m
    per_q = [[] for _ in range(nq)]
    for l in range(nlist):
        c = min(probed_by[l], nq)
        if nq == 1:
            qs = [0]
        elif l <= 2:  # (the empty list, the one-row list and a 31-row list: what query 0 probes)
            qs = [0] + list(1 + rs.choice(nq - 1, c - 1, replace=False))
        else:
            qs = list(1 + rs.choice(nq - 1, min(c, nq - 1), replace=False))
        for q in qs:
            per_q[int(q)].append(l)
    for p in per_q:
        if not p:
            p.append(nlist - 1)
    nprobe = max(len(p) for p in per_q)
    keys = np.full((nq, nprobe), -1, np.int64)
    for q, p in enumerate(per_q):
        keys[q, :len(p)] = rs.permutation(p)
    return xq.astype(np.float32), keys


def new_handle(capi, t, xb=None):
    h = capi.Handle(t.d, t.nlist, t.metric, 0)
    h.set_centroids(t.cen)
    h.set_lists_from_assign(t.xb if xb is None else xb, t.assign)
    return h


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the premise, on the CPU: on eligible data the oracle's fp32 result is float32 of the exact integer, and its rows are the
#    brute-force top-k (store_pairs and max_codes included, which also pins this file's model of them)
# ------------------------------------------------------------------------------------------------------------------------------
def test_references_agree_on_eligible_data(oracle):
    for d, m in SHAPES:
        assert d * m * m <= LIMIT and (m == 255 or d * (m + 1) * (m + 1) > LIMIT), (d, m)
        assert limit_m(d) == m or (m == 255 and d <= 258)
        for metric in METRICS:
            t = make_lists(d, m, metric, 100 + d)
            lists = oracle.Lists(metric, t.cen, t.xb, t.assign)
            xq, keys = make_queries(t, 70, 200 + d)
            E = exact_table(metric, xq, t.xb)
            assert E.max() == d * m * m and E.min() >= 0  # the extreme pair is there
            zero = np.zeros(keys.shape, np.float32)
            for k, pairs, mc in ((10, False, 0), (200, False, 0), (10, True, 0), (100, False, len(t.xb) // 7)):
                eD, eI, _ = oracle.search_preassigned(lists, xq, k, keys, zero, store_pairs=pairs, max_codes=mc)
                rows = rows_of_pairs(eI, t.assign, t.nlist) if pairs else eI
                check_exact(metric, eD, rows, E, probed_mask(keys, t.assign, t.nlist, mc), k, (d, m, metric, k, pairs, mc))
            # the extreme pair itself: query 0 against the row of list 1
            row = int(np.nonzero(t.assign == 1)[0][0])
            eD, eI, _ = oracle.search_preassigned(lists, xq[:1], 200, keys[:1], zero[:1])
            at = np.nonzero(eI[0] == row)[0]
            assert len(at) == 1 and bits(eD[0, at[0]]) == bits(np.float32(d * m * m)), (d, m, metric)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. fixed-nprobe search
# ------------------------------------------------------------------------------------------------------------------------------
def run_search(h, t, xq, k, keys, pairs=False, mc=0):
    h.stats(reset=True)
    D, I = h.search_preassigned(xq, k, keys, store_pairs=pairs, max_codes=mc)
    st = h.stats()
    return D, I, [st["nlist"], st["ndis"], st["nheap_updates"]]


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,m", SHAPES)
def test_fixed_nprobe_search(capi, oracle, monkeypatch, d, m, metric):
    t = make_lists(d, m, metric, 300 + d)
    lists = oracle.Lists(metric, t.cen, t.xb, t.assign)
    h = new_handle(capi, t)
    nb, turn = len(t.xb), 0
    for nq in (1, 19, 70, 513):
        xq, keys = make_queries(t, nq, 400 + d + nq)
        E = exact_table(metric, xq, t.xb)
        zero = np.zeros(keys.shape, np.float32)
        for k in (1, 10, 100, 200):
            variants = [(False, 0)] + ([(True, 0)] if k == 10 else []) + ([(False, max(1, nb // 7))] if k == 100 else [])
            for pairs, mc in variants:
                eD, eI, est = oracle.search_preassigned(lists, xq, k, keys, zero, store_pairs=pairs, max_codes=mc)
                probed = probed_mask(keys, t.assign, t.nlist, mc)
                top = topk_table(metric, E, probed, k)
                for rounds in (1, 2):  # dense only; dense + one threshold round
                    for pipe in ((7, 3, 0) if k == 10 else ((7, 3, 0)[turn % 3],)):  # ks >= 5: one kernel whatever is asked
                        turn += 1
                        monkeypatch.setenv("AUNCEL_AMD_SELECT", "heap" if turn % 2 else "sorted")
                        h.set_option("fixed_rounds", rounds)
                        h.set_option("scan_pipelined", pipe)
                        D, I, st = run_search(h, t, xq, k, keys, pairs, mc)
                        tag = f"d={d} m={m} metric={metric} nq={nq} k={k} pairs={pairs} mc={mc} rounds={rounds} pipe={pipe} turn={turn}"
                        assert h.scan_arith() == 2, tag
                        assert np.array_equal(I, eI), tag
                        assert np.array_equal(bits(D), bits(eD)), tag
                        assert st == list(est), tag
                        check_exact(metric, D, rows_of_pairs(I, t.assign, t.nlist) if pairs else I, E, probed, k, tag, top=top)
        # search(): the engine's own coarse ranking in front
        nprobe = 5
        cd, ck = oracle.knn(metric, xq, t.cen, nprobe)
        eD, eI, est = oracle.search_preassigned(lists, xq, 10, ck, cd)
        h.set_option("fixed_rounds", None)
        h.set_option("scan_pipelined", None)
        D, I = h.search(xq, 10, nprobe)
        assert h.scan_arith() == 2
        assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD)), (d, m, metric, nq, "search")
        check_exact(metric, D, I, E, probed_mask(ck, t.assign, t.nlist), 10, (d, m, metric, nq, "search"))
        # the same handle in fp32 arithmetic
        h.set_byte_codes(0)
        for k, rounds in ((10, 1), (200, 2)):
            eD, eI, est = oracle.search_preassigned(lists, xq, k, keys, zero)
            h.set_option("fixed_rounds", rounds)
            D, I, st = run_search(h, t, xq, k, keys)
            assert h.scan_arith() == 1
            assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD)) and st == list(est), (d, m, metric, nq, k, "fp32")
        h.set_byte_codes(1)
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the eligibility rule where magnitude decides it, on the lists' side and on the queries' side
# ------------------------------------------------------------------------------------------------------------------------------
def check_against_oracle(oracle, h, t, lists, xb, xq, keys, want_bytes, tag):
    E = exact_table(t.metric, xq, xb)
    zero = np.zeros(keys.shape, np.float32)
    probed = probed_mask(keys, t.assign, t.nlist)
    for k, rounds in ((10, 1), (200, 2)):
        eD, eI, est = oracle.search_preassigned(lists, xq, k, keys, zero)
        h.set_option("fixed_rounds", rounds)
        D, I, st = run_search(h, t, xq, k, keys)
        assert (h.scan_arith() == 2) == want_bytes, (tag, h.scan_arith())
        assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD)) and st == list(est), (tag, k)
        # beyond 2^24 the reference's value depends on its summation order: the oracle alone is the reference for those pairs
        check_exact(t.metric, D, I, E, probed, k, (tag, k), skip_above=LIMIT)
    h.set_option("fixed_rounds", None)
    return E


BOUNDARY = [(d, m) for d, m in SHAPES if m < 255] + [(258, 255)]  # (258, 255): m + 1 = 256 leaves the type, not the magnitude


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,m", BOUNDARY)
def test_eligibility_boundary(capi, oracle, d, m, metric):
    """(a) lists <= m, one query element m + 1; (b) one list element m + 1, queries <= m; (c) both <= m.  Byte codes in (c) only; the
    oracle's result in all three.  In (a) and (b) the extreme pair is all m + 1 against all 0 (L2) / all m (IP): d (m + 1)^2 for L2
    passes 2^24 (at d = 259: 16 841 475, which fp32 does not hold)."""
    t = make_lists(d, m, metric, 500 + d)
    nq = 70
    xq, keys = make_queries(t, nq, 600 + d)
    lists = oracle.Lists(metric, t.cen, t.xb, t.assign)
    row1 = int(np.nonzero(t.assign == 1)[0][0])  # the row query 0 probes
    # (c)
    h = new_handle(capi, t)
    check_against_oracle(oracle, h, t, lists, t.xb, xq, keys, True, (d, m, metric, "c"))
    # (a) one element of one query, then a whole query of m + 1 (L2: against a list row of all 0)
    xa = xq.copy()
    xa[7, d // 2] = m + 1
    check_against_oracle(oracle, h, t, lists, t.xb, xa, keys, False, (d, m, metric, "a1"))
    check_against_oracle(oracle, h, t, lists, t.xb, xq, keys, True, (d, m, metric, "c again"))  # ... and back on the same handle
    h.close()
    xb0 = t.xb.copy()
    xb0[row1] = 0 if metric == 1 else m
    xa = xq.copy()
    xa[0] = m + 1
    h = new_handle(capi, t, xb0)
    E = check_against_oracle(oracle, h, t, oracle.Lists(metric, t.cen, xb0, t.assign), xb0, xa, keys, False, (d, m, metric, "a2"))
    assert E[0, row1] == (d * (m + 1) * (m + 1) if metric == 1 else d * m * (m + 1))
    h.close()
    # (b) one element of one row, then a whole row of m + 1
    xb1 = t.xb.copy()
    xb1[np.nonzero(t.assign == t.nlist - 1)[0][5], d - 1] = m + 1
    h = new_handle(capi, t, xb1)
    check_against_oracle(oracle, h, t, oracle.Lists(metric, t.cen, xb1, t.assign), xb1, xq, keys, False, (d, m, metric, "b1"))
    h.close()
    xb2 = t.xb.copy()
    xb2[row1] = m + 1
    h = new_handle(capi, t, xb2)
    E = check_against_oracle(oracle, h, t, oracle.Lists(metric, t.cen, xb2, t.assign), xb2, xq, keys, False, (d, m, metric, "b2"))
    assert E[0, row1] == (d * (m + 1) * (m + 1) if metric == 1 else d * m * (m + 1))
    h.close()


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_full_byte_range_at_d_259_is_not_eligible(capi, oracle, metric):
    """d = 259, both sides 0 .. 255: every value fits the type, the magnitude does not (259 * 255^2 = 16 841 475 > 2^24, and no fp32
    number), so the search runs in fp32 and equals the oracle -- the extreme pair included, for which only the oracle speaks"""
    t = make_lists(259, 255, metric, 777)
    xq, keys = make_queries(t, 70, 778)
    lists = oracle.Lists(metric, t.cen, t.xb, t.assign)
    h = new_handle(capi, t)
    E = check_against_oracle(oracle, h, t, lists, t.xb, xq, keys, False, (259, 255, metric))
    assert E.max() == 16841475
    zero = np.zeros((1, keys.shape[1]), np.float32)
    eD, eI, _ = oracle.search_preassigned(lists, xq[:1], 200, keys[:1], zero)
    D, I = h.search_preassigned(xq[:1], 200, keys[:1])
    row1 = int(np.nonzero(t.assign == 1)[0][0])
    assert row1 in I[0] and np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    h.close()


@gpu
@pytest.mark.parametrize("d,m", [(259, 254), (960, 132)])
def test_eligible_and_ineligible_queries_on_one_handle(capi, oracle, d, m):
    """eligible, ineligible, eligible queries through one handle -- as caller's queries and as resident ones, whose signed-byte copy
    is cached between calls and must not serve a query set it was not made from"""
    metric = 1
    t = make_lists(d, m, metric, 900 + d)
    lists = oracle.Lists(metric, t.cen, t.xb, t.assign)
    h = new_handle(capi, t)
    nq, nprobe, k = 70, 6, 10
    good, _ = make_queries(t, nq, 901 + d)
    other, _ = make_queries(t, nq, 902 + d)  # (eligible too, other values: a stale byte copy would show)
    bad = good.copy()
    bad[3, 1] = m + 1
    for step, (xq, want) in enumerate(((good, True), (bad, False), (good, True), (other, True), (bad, False), (other, True))):
        cd, ck = oracle.knn(metric, xq, t.cen, nprobe)
        eD, eI, _ = oracle.search_preassigned(lists, xq, k, ck, cd)
        D, I = h.search(xq, k, nprobe)
        assert (h.scan_arith() == 2) == want, step
        assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD)), step
        h.set_queries(xq)
        for start, n in ((0, nq), (0, nq), (5, 40), (5, 40), (0, nq)):
            D, I = h.search_resident(start, n, k, nprobe)
            assert (h.scan_arith() == 2) == want, (step, start, n)
            assert np.array_equal(I, eI[start:start + n]) and np.array_equal(bits(D), bits(eD[start:start + n])), (step, start, n)
            D, I = h.search_resident_preassigned(start, n, k, ck[start:start + n])
            assert (h.scan_arith() == 2) == want, (step, start, n)
            assert np.array_equal(I, eI[start:start + n]) and np.array_equal(bits(D), bits(eD[start:start + n])), (step, start, n)
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. range search: the MASKED kernel with the exact mask
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,m", SHAPES)
def test_range_search(capi, oracle, d, m, metric):
    t = make_lists(d, m, metric, 1100 + d)
    lists = oracle.Lists(metric, t.cen, t.xb, t.assign)
    h = new_handle(capi, t)
    for nq in (19, 513):
        xq, keys = make_queries(t, nq, 1200 + d + nq)
        E = exact_table(metric, xq, t.xb)
        probed = probed_mask(keys, t.assign, t.nlist)
        vals = E[probed]
        r0 = int(np.median(vals[vals < (1 << 23)]))  # an integer that is a distance of some probed pair (r0 +- 0.5 are fp32 numbers)
        r0 = int(vals[np.argmin(np.abs(vals - r0))])
        assert (vals == r0).any() and r0 + 0.5 == float(np.float32(r0 + 0.5))
        radii = [float(r0), r0 - 0.5, r0 + 0.5, 0.0, -1.0, -float(d * m * m) - 0.5, float(d * m * m), float(1 << 25), float("inf")]
        for radius in radii:
            radius = float(np.float32(radius))
            elims, elab, edis, est = oracle.range_search_preassigned(lists, xq, radius, keys)
            h.stats(reset=True)
            lims, lab, dis = h.range_search(xq, radius, keys.shape[1], keys=keys)
            tag = (d, m, metric, nq, radius)
            assert h.scan_arith() == 2, tag
            assert np.array_equal(lims, elims) and np.array_equal(lab, elab) and np.array_equal(bits(dis), bits(edis)), tag
            st = h.stats()
            assert [st["nlist"], st["ndis"]] == list(est), tag
            # counts and values against the integers (the comparison is strict, as the reference's)
            inside = probed & ((E < radius) if metric == 1 else (E > radius))
            assert np.array_equal(np.diff(lims), inside.sum(1)), tag
            q = np.repeat(np.arange(nq), np.diff(lims))
            assert inside[q, lab].all(), tag
            assert np.array_equal(bits(dis), bits(E[q, lab].astype(np.float32))), tag
        # the radii above must have met all three outcomes
        assert (probed & (E == r0)).any()
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 5. adaptive (Auncel) search: the flow of test_gpu_random_adaptive.py on wide byte data
# ------------------------------------------------------------------------------------------------------------------------------
def adaptive_case(d, m, metric, seed):
    rs = np.random.RandomState(7000 + SEED_OFFSET + 97 * seed + d + metric)
    nlist = int(rs.choice([64, 128]))
    K = int(rs.choice([10, 20, 100, 130])) if metric == 1 else int(rs.choice([5, 10]))
    nb, nq = 6000, int(rs.choice([7, 40, 150]))
    nblobs = nlist // 2
    centres = rs.rand(nblobs, d) * (m * 0.63)

    def draw(n):
        return np.floor(np.clip(centres[rs.randint(0, nblobs, n)] + rs.randn(n, d) * (m * 0.12), 0, m)).astype(np.float32)
    if metric == 1:
        xb, xq = draw(nb), draw(nq)
        xb[0] = m  # the largest value is there on both sides
        xq[0, 0] = m
        cen = (xb[rs.choice(nb, nlist, replace=False)] + rs.randn(nlist, d) * 1e-3).astype(np.float32)  # no exact coarse ties
    else:
        # The reference's inner-product rule reads every product as a cosine (error_pro::arcos, domain [-1, 1], and its table
        # ends before 1): among byte values only products of 0 are inside it.  So rows and queries keep to disjoint coordinates:
        # every distance is 0 exactly where the kernel's acc + cx + cy cancels (terms up to 128 * 255 * d), and equal distances
        # everywhere leave the ids to the reference's heap order.
        cut = 3 * d // 4
        xb, xq = np.zeros((nb, d), np.float32), np.zeros((nq, d), np.float32)
        xb[:, :cut] = rs.randint(0, m + 1, size=(nb, cut))
        xq[:, cut:] = rs.randint(0, m + 1, size=(nq, d - cut))
        xb[0, :cut] = m
        xq[0, cut:] = m
        cen = (xb[rs.choice(nb, nlist, replace=False)] / (4.0 * m * d) + rs.randn(nlist, d) * 1e-6).astype(np.float32)
    ntr = 1
    while (1 << ntr) <= nlist // 8:
        ntr += 1
    traces = []
    for _ in range(ntr):
        n = int(rs.randint(3, 60))
        x = np.sort(rs.rand(n) * 25.0).astype(np.float32)
        x += np.arange(n, dtype=np.float32) * 1e-3  # strictly ascending
        traces.append((x, (0.5 + rs.rand(n) * 2.5).astype(np.float32), (rs.rand(n) * 0.5).astype(np.float32)))
    qk = min(int(rs.choice([1, 3, 10, min(K, 40)])), K)
    return dict(nlist=nlist, d=d, metric=metric, K=K, xb=xb, xq=xq, cen=cen, traces=traces, query_topk=qk,
                req=rs.choice([0.5, 0.8, 0.9, 0.95, 0.99], size=nq).astype(np.float32),
                multipler=float(rs.choice([1.0, 1.3, 2.0, 3.7])), std_m=float(rs.choice([0.0, 1.0, 2.0])), profile=bool(seed % 2))


@gpu
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("d,m,metric", [(160, 255, 1), (960, 132, 1), (160, 255, 0)])
def test_adaptive_search(capi, oracle, monkeypatch, d, m, metric, seed):
    c = adaptive_case(d, m, metric, seed)
    monkeypatch.setenv("AUNCEL_AMD_REPLAY_NLD", "16" if seed % 2 else "32")
    monkeypatch.setenv("AUNCEL_AMD_SELECT", "heap" if seed % 3 == 0 else "sorted")
    nq, K, nlist = c["xq"].shape[0], c["K"], c["nlist"]
    _, a = oracle.knn(metric, c["xb"], c["cen"], 1, nthreads=8)
    assign = a[:, 0].copy()
    if metric == 0:
        # the reference's inner-product rule needs lists of at least max_topk vectors: the first rows are dealt round the lists
        assign[:nlist * K] = np.arange(nlist * K) % nlist
    lists = oracle.Lists(metric, c["cen"], c["xb"], assign)
    assert metric == 1 or lists.sizes.min() >= K
    cd, ck = oracle.knn(metric, c["xq"], c["cen"], nlist, nthreads=8)
    gtD, _ = oracle.knn(metric, c["xq"], c["xb"], K, nthreads=8)
    arcos = capi.arcos_table()
    tun = oracle.Tuner(oracle.interdis(metric, c["cen"]), c["traces"], K, nq, arcos=arcos)
    stt = tun.struct(c["query_topk"], c["req"], c["multipler"], c["std_m"], gt_D=gtD, profile=c["profile"])
    tag = {k: v for k, v in c.items() if k in ("nlist", "d", "metric", "K", "query_topk", "multipler", "std_m", "profile")}
    eD, eI, est = oracle.search_preassigned(lists, c["xq"], K, ck, cd, tuner=stt, offset=0, nthreads=1)
    h = capi.Handle(d, nlist, metric, 0)
    h.set_centroids(c["cen"])
    h.set_lists_from_assign(c["xb"], assign)
    h.set_interdis(None)
    h.set_tuner(K, c["traces"], arcos)
    h.set_queries(c["xq"])
    my_np = np.zeros(nq, dtype=np.uint64)
    t_rec = np.zeros(nq, dtype=np.float32)
    h.stats(reset=True)
    D, I = h.search_adaptive(0, nq, c["query_topk"], c["multipler"], c["std_m"], c["req"], my_np, t_rec, gt_D=gtD, profile=c["profile"])
    assert h.scan_arith() == 2, tag
    assert np.array_equal(my_np.astype(np.int64), tun.my_nprobe.astype(np.int64)), tag
    assert np.array_equal(I, eI), tag
    assert np.array_equal(bits(D), bits(eD)), tag
    assert np.array_equal(bits(t_rec), bits(tun.t_recalls)), tag
    st = h.stats()
    assert [st["nlist"], st["ndis"], st["nheap_updates"]] == list(est), tag
    # the integers: every returned pair, and the probed prefix of the coarse ranking as the candidate set
    E = exact_table(metric, c["xq"], c["xb"])
    keys = np.where(np.arange(nlist)[None, :] < tun.my_nprobe.astype(np.int64)[:, None], ck, -1)
    ok = I >= 0
    q = np.nonzero(ok)[0]
    assert np.array_equal(bits(D[ok]), bits(E[q, I[ok]].astype(np.float32))), tag
    assert probed_mask(keys, assign, nlist)[q, I[ok]].all(), tag
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 6. random sweep
# ------------------------------------------------------------------------------------------------------------------------------
def sweep_case(seed):
    rs = np.random.RandomState(9000 + SEED_OFFSET + seed)
    d = int(rs.randint(129, 1101))
    if rs.rand() < 0.6:
        d |= 1  # odd dimensions over-represented
    kind = str(rs.choice(["bytes", "dups", "binary"]))
    top = limit_m(d)
    m = 1 if kind == "binary" else int(rs.choice([top, top, rs.randint(1, top + 1)]))
    nlist = int(rs.choice([1, 2, 7, 16, 33, 64]))
    nb = int(rs.choice([50, 300, 2000, 5000]))
    nq = int(rs.choice([1, 3, 19, 64, 130]))
    metric = int(rs.choice([0, 1]))
    if kind == "dups":
        base = rs.randint(max(0, m - 4), m + 1, size=(max(nb // 20, 2), d)).astype(np.float32)
        xb = base[rs.randint(0, len(base), size=nb)]
        xq = base[rs.randint(0, len(base), size=nq)]
    else:
        xb = rs.randint(0, m + 1, size=(nb, d)).astype(np.float32)
        xq = rs.randint(0, m + 1, size=(nq, d)).astype(np.float32)
    xb[rs.randint(0, nb)] = m  # the limit is met: a row of all m, and a query at the other end
    xq[rs.randint(0, nq)] = 0 if metric == 1 else m
    cen = xb[rs.choice(nb, size=nlist, replace=nb < nlist)].copy()
    # ragged on purpose: some lists empty, one list large
    assign = rs.randint(0, nlist, size=nb)
    if nlist > 2:
        assign[assign == 1] = 0
    k = int(rs.choice([1, 5, 10, 64, 100, 127, 128, 200]))
    nprobe = int(rs.choice([1, 2, 5, 16, 24, nlist, nlist + 3]))
    return dict(d=d, m=m, nlist=nlist, metric=metric, xb=xb, xq=xq, cen=cen, assign=assign, k=k, nprobe=nprobe, kind=kind)


@gpu
@pytest.mark.parametrize("seed", range(60))
def test_sweep_search_and_range(capi, oracle, monkeypatch, seed):
    c = sweep_case(seed)
    d, m, metric, nlist = c["d"], c["m"], c["metric"], c["nlist"]
    assert d * m * m <= LIMIT
    lists = oracle.Lists(metric, c["cen"], c["xb"], c["assign"])
    npq = min(c["nprobe"], nlist)
    cd, ck = oracle.knn(metric, c["xq"], c["cen"], npq)
    keys = np.full((c["xq"].shape[0], c["nprobe"]), -1, dtype=np.int64)  # (-1 beyond nlist, as the reference's heap leaves it)
    keys[:, :npq] = ck
    zero = np.zeros(keys.shape, np.float32)
    E = exact_table(metric, c["xq"], c["xb"])
    h = capi.Handle(d, nlist, metric, 0)
    h.set_centroids(c["cen"])
    h.set_lists_from_assign(c["xb"], c["assign"])
    for pairs, mc in ((False, 0), (True, 0), (False, max(1, len(c["xb"]) // 7))):
        eD, eI, est = oracle.search_preassigned(lists, c["xq"], c["k"], keys, zero, store_pairs=pairs, max_codes=mc)
        probed = probed_mask(keys, c["assign"], nlist, mc)
        for rounds in ("1", "2"):
            monkeypatch.setenv("AUNCEL_AMD_FIXED_ROUNDS", rounds)
            monkeypatch.setenv("AUNCEL_AMD_SELECT", "heap" if (seed + int(rounds)) % 3 == 0 else "sorted")
            h.stats(reset=True)
            D, I = h.search_preassigned(c["xq"], c["k"], keys, store_pairs=pairs, max_codes=mc)
            tag = f"{c['kind']} d={d} m={m} nlist={nlist} k={c['k']} nprobe={c['nprobe']} pairs={pairs} mc={mc} rounds={rounds}"
            assert h.scan_arith() == 2, tag
            assert np.array_equal(I, eI), tag
            assert np.array_equal(bits(D), bits(eD)), tag
            st = h.stats()
            assert [st["nlist"], st["ndis"], st["nheap_updates"]] == list(est), tag
            check_exact(metric, D, rows_of_pairs(I, c["assign"], nlist) if pairs else I, E, probed, c["k"], tag)
    monkeypatch.delenv("AUNCEL_AMD_FIXED_ROUNDS")
    monkeypatch.delenv("AUNCEL_AMD_SELECT")
    # range search at a distance that occurs among the probed pairs
    probed = probed_mask(keys, c["assign"], nlist)
    vals = E[probed]
    radius = float(np.float32(np.median(vals))) if vals.size else 1.0
    elims, elab, edis, est = oracle.range_search_preassigned(lists, c["xq"], radius, keys)
    h.stats(reset=True)
    lims, lab, dis = h.range_search(c["xq"], radius, c["nprobe"], keys=keys)
    assert h.scan_arith() == 2
    assert np.array_equal(lims, elims) and np.array_equal(lab, elab) and np.array_equal(bits(dis), bits(edis))
    st = h.stats()
    assert [st["nlist"], st["ndis"]] == list(est)
    inside = probed & ((E < radius) if metric == 1 else (E > radius))
    assert np.array_equal(np.diff(lims), inside.sum(1))
    h.close()
