"""Id selectors combined on the device, range search under a selector, selected searches in flight (amd_ivf_selector_combine,
amd_ivf_range_search_selected / _preassigned_selected, amd_ivf_submit_search_resident_selected; ivf_selector.hip).  The expected
value is the pinned CPU oracle over the lists with the non-members removed -- membership by the numpy list model under the same
boolean expression -- and, for range search, the same call on amd_ivf_subset of the same selector.  Every comparison is of bits or
of integers."""
import functools

import numpy as np
import pytest

from test_gpu_subset import filtered, oracle_lists, selector
from test_gpu_update import BYTE_CASES, K, NPROBE, NQ, Model, bits, handle, make_case

pytestmark = pytest.mark.gpu

PAIRS = [("range_third", "mod_3_1"), ("bits_half", "bits_1pct"), ("bits_all", "bits_lists"), ("bits_none", "slice_mid")]


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


@functools.lru_cache(maxsize=None)
def case(name):
    metric, cen, assign, xb, xq = make_case(name)
    return metric, cen, assign, xb, xq, Model(cen.shape[0], cen.shape[1], xb, assign)


@functools.lru_cache(maxsize=None)
def coarse(oracle, name):
    metric, cen, assign, xb, xq, model = case(name)
    return oracle.knn(metric, xq, cen, NPROBE)


# ---- boolean expressions over named selectors: a name, or (op, e) / (op, e1, e2) with op in "not", "and", "or", "andnot"
def rule_of(capi, expr, model):
    """the membership rule of an expression, as test_gpu_subset.selector's rules: (ids of a list, list number, entries before) -> bools"""
    if isinstance(expr, str):
        return selector(capi, expr, model)[1]
    rules = [rule_of(capi, e, model) for e in expr[1:]]
    op = expr[0]
    if op == "not":
        return lambda ids, l, seen: ~np.asarray(rules[0](ids, l, seen), bool)
    f = {"and": lambda a, b: a & b, "or": lambda a, b: a | b, "andnot": lambda a, b: a & ~b}[op]
    return lambda ids, l, seen: f(np.asarray(rules[0](ids, l, seen), bool), np.asarray(rules[1](ids, l, seen), bool))


class Made:
    """the Selector of an expression on `parent`, made with Selector.combine from base selectors; closes everything it made"""

    def __init__(self, capi, parent, model, expr):
        self.capi, self.parent, self.model, self.all = capi, parent, model, []
        self.s = self.make(expr)

    def make(self, expr):
        capi = self.capi
        if isinstance(expr, str):
            s = self.parent.selector(*selector(capi, expr, self.model)[0])
        else:
            ops = [self.make(e) for e in expr[1:]]
            code = {"not": capi.SELECTOR_NOT, "and": capi.SELECTOR_AND, "or": capi.SELECTOR_OR, "andnot": capi.SELECTOR_ANDNOT}[expr[0]]
            s = ops[0].combine(code, ops[1] if len(ops) > 1 else None)
        self.all.append(s)
        return s

    def __enter__(self):
        return self.s

    def __exit__(self, *exc):
        for s in self.all:
            s.close()


def same(got, eD, eI, what=None):
    D, I = got
    assert np.array_equal(I, eI), what
    assert np.array_equal(bits(D), bits(eD)), what


def byte_settings(name):
    return (1, 0) if name in BYTE_CASES else (0,)


def knn_expected(oracle, capi, name, expr):
    """the filtered lists of an expression and the oracle's (D, I, stats) over them at (K, NPROBE)"""
    metric, cen, assign, xb, xq, model = case(name)
    want = filtered(model, rule_of(capi, expr, model))
    cd, ck = coarse(oracle, name)
    eD, eI, est = oracle.search_preassigned(oracle_lists(oracle, metric, cen, want), xq, K, ck, cd)
    return want, eD, eI, est


# ------------------------------------------------------------------------------------------------ 1. combine against the model
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "+".join(p))
@pytest.mark.parametrize("name", ["ragged", "odd_30", "sift_l2", "bytes_200"])
def test_combine_equals_the_model(capi, oracle, name, pair):
    """AND, OR, ANDNOT both ways, NOT of each operand and (a | b) - (a & b): the kept count is the model's under the same expression,
    and search_preassigned_selected under the result is the oracle over the filtered lists (nheap_updates the filtered lists')"""
    metric, cen, assign, xb, xq, model = case(name)
    if name == "ragged":  # (otherwise selector_valid_word is not exercised: an empty list, a ragged last word, an odd 32-block count)
        lens = [len(i) for i in model.ids]
        assert any(n == 0 for n in lens) and any(n % 64 != 0 for n in lens) and any(((n + 31) // 32) % 2 == 1 for n in lens), lens
    a, b = pair
    exprs = [("and", a, b), ("or", a, b), ("andnot", a, b), ("andnot", b, a), ("not", a), ("not", b), ("andnot", ("or", a, b), ("and", a, b))]
    cd, ck = coarse(oracle, name)
    parent = handle(capi, metric, cen, xb, assign, 1)
    D0, I0 = parent.search(xq, K, NPROBE)
    for expr in exprs:
        want, eD, eI, est = knn_expected(oracle, capi, name, expr)
        with Made(capi, parent, model, expr) as s:
            looked, kept, h2d, held = s.info()
            nwords = sum((len(i) + 63) // 64 for i in model.ids)
            assert (looked, kept, h2d) == (len(xb), sum(len(i) for i in want.ids), 0), (expr, s.info())
            assert 0 < held <= 8 * nwords + 4 * nwords + 4 * cen.shape[0], (held, nwords)
            for byte in byte_settings(name):
                parent.set_byte_codes(byte)
                parent.stats(reset=True)
                same(parent.search_preassigned_selected(s, xq, K, ck, cd), eD, eI, (expr, byte))
                assert parent.stats()["nheap_updates"] == est[2], (expr, byte)
            parent.set_byte_codes(1)
            if expr == ("not", "bits_none"):
                same(parent.search_selected(s, xq, K, NPROBE), D0, I0, "NOT(bits_none) is the unfiltered search")
                same((eD, eI), D0, I0)
            if expr == ("not", "bits_all"):  # (a bit that survives past a list's end would be a candidate here)
                assert kept == 0
                for byte in byte_settings(name):
                    parent.set_byte_codes(byte)
                    assert (parent.search_preassigned_selected(s, xq, K, ck, cd)[1] == -1).all(), byte
                    assert (parent.search_selected(s, xq, K, NPROBE)[1] == -1).all(), byte
                parent.set_byte_codes(1)
    same(parent.search(xq, K, NPROBE), D0, I0, "unfiltered, after")
    parent.close()


# ------------------------------------------------------------------------------------------------ 2. a dense round's mask
@pytest.mark.parametrize("row_lists", [0, 1])
@pytest.mark.parametrize("name", ["sift_l2", "l2_96"])
def test_dense_round_writes_combined_keep_words_as_its_mask(capi, oracle, name, row_lists):
    """fixed_rounds 2 under NOT(bits_half): the dense round's mask is the combined selector's keep words themselves -- a set bit past
    a list's end would admit a candidate that does not exist"""
    metric, cen, assign, xb, xq, model = case(name)
    expr = ("not", "bits_half")
    want, eD, eI, est = knn_expected(oracle, capi, name, expr)
    cd, ck = coarse(oracle, name)
    parent = handle(capi, metric, cen, xb, assign, 1)
    parent.set_option("fixed_rounds", 2)
    parent.set_option("row_lists", row_lists)
    with Made(capi, parent, model, expr) as s:
        for byte in byte_settings(name):
            parent.set_byte_codes(byte)
            parent.stats(reset=True)
            same(parent.search_preassigned_selected(s, xq, K, ck, cd), eD, eI, byte)
            assert parent.stats()["nheap_updates"] == est[2]
            assert parent.last_timing_detail()["min_bytes_thr"] > 0, "no threshold round ran"
            same(parent.search_selected(s, xq, K, NPROBE), eD, eI, byte)
    parent.close()


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_combine_refusals_and_lifetime(capi, oracle):
    metric, cen, assign, xb, xq, _ = case("l2_96")
    nlist, d = cen.shape
    model = Model(nlist, d, xb, assign)
    parent = handle(capi, metric, cen, xb, assign, 1)
    other = handle(capi, metric, cen, xb, assign, 1)
    L = capi.lib()

    def refused(f, word):
        with pytest.raises(capi.EngineError) as e:
            f()
        assert e.value.code == -2, e.value
        assert word in L.amd_ivf_last_error().decode(), L.amd_ivf_last_error()

    a = parent.selector(capi.SUBSET_ID_MOD, 3, 1)
    b = parent.selector(capi.SUBSET_ID_RANGE, 0, 1500)
    foreign = other.selector(capi.SUBSET_ID_MOD, 3, 1)
    for op in (capi.SELECTOR_AND, capi.SELECTOR_OR, capi.SELECTOR_ANDNOT):
        refused(lambda: a.combine(op, foreign), "different indexes")
        refused(lambda: foreign.combine(op, a), "different indexes")
        refused(lambda: a.combine(op, None), "two operands")
    refused(lambda: a.combine(capi.SELECTOR_NOT, b), "one operand")
    for op in (-1, 4, 17):
        refused(lambda: a.combine(op, b), "unknown op")
        refused(lambda: a.combine(op, None), "unknown op")
    foreign.close()
    other.close()
    # tickets out on the index: the rule of amd_ivf_selector_create
    parent.set_queries(xq)
    t = parent.submit_search_resident(0, NQ, K, NPROBE)
    refused(lambda: a & b, "tickets")
    parent.wait(t)
    parent.set_async_depth(0)
    # the result outlives its operands, and counts among the index's live selectors
    rule = lambda ids, l, seen: (np.fmod(ids, 3) == 1) & (ids < 1500)  # noqa: E731
    want = filtered(model, rule)
    cd, ck = coarse(oracle, "l2_96")
    eD, eI, _ = oracle.search_preassigned(oracle_lists(oracle, metric, cen, want), xq, K, ck, cd)
    both = a & b
    a.close()
    b.close()
    assert both.info()[:3] == (len(xb), sum(len(i) for i in want.ids), 0)
    same(parent.search_preassigned_selected(both, xq, K, ck, cd), eD, eI)
    same(parent.search_selected(both, xq, K, NPROBE), eD, eI)
    refused(parent.close, "1 selector")
    same(parent.search_selected(both, xq, K, NPROBE), eD, eI, "still a valid handle")
    # an operand made stale by amd_ivf_add
    fresh = parent.selector(capi.SUBSET_ID_MOD, 2, 0)
    parent.add(xq[:3].copy(), np.arange(5000, 5003, dtype=np.int64), np.array([0, 1, 2]))
    newer = parent.selector(capi.SUBSET_ID_MOD, 2, 0)
    refused(lambda: ~both, "stale")
    refused(lambda: both | fresh, "stale")
    refused(lambda: newer & fresh, "stale")
    refused(lambda: fresh & newer, "stale")
    with ~newer as n:
        assert n.info()[0] == len(xb) + 3 and n.info()[1] == len(xb) + 3 - newer.info()[1]
    for s in (both, fresh, newer):
        s.close()
    parent.close()


# ------------------------------------------------------------------------------------------------ 4. range search
# The radius of a (case, selector) comes from the oracle alone: the oracle's k-NN distances at (RANGE_K, NPROBE) of all queries over
# the FILTERED lists, the finite ones (a query that probes fewer than RANGE_K members ends in padding), and of those the quantile
# RANGE_Q counted from the near end -- the RANGE_Q quantile for L2 (results are the entries below the radius), the 1 - RANGE_Q
# quantile for inner product (results are the entries above it).  Where the filtered lists hold nothing (bits_none) the same rule
# over the unfiltered lists.  RANGE_K = 128, RANGE_Q = 0.4: two in five of a query's 128 nearest members lie inside on average
# (51), so the queries in dense places get more than 64 results, and results from far down their lists; bits_1pct keeps ~30
# entries of 3000, its table holds every member a query probes (~15), and a radius that takes the nearer two fifths of those
# distances leaves the queries with no member in their own cluster empty-handed.  (The conditions below hold for every case at
# 0.35 and 0.4; at 0.3 no query of sift_l2 / mod_3_1 has more than 64 results, at 0.45 every query of ip_96 / bits_1pct has one.)
RANGE_K, RANGE_Q = 128, 0.4
RANGE_SELECTORS = ["bits_half", "bits_1pct", "mod_3_1", "bits_none", ("not", "bits_half")]


def radius_of(metric, eD):
    fin = eD[np.isfinite(eD) & (np.abs(eD) < 1e37)]
    assert fin.size
    return float(np.quantile(fin, RANGE_Q if metric == 1 else 1.0 - RANGE_Q))


@functools.lru_cache(maxsize=None)
def range_expected(oracle, capi, name, expr):
    metric, cen, assign, xb, xq, model = case(name)
    want = filtered(model, rule_of(capi, expr, model))
    cd, ck = coarse(oracle, name)
    near = want if sum(len(i) for i in want.ids) else model
    radius = radius_of(metric, oracle.search_preassigned(oracle_lists(oracle, metric, cen, near), xq, RANGE_K, ck, cd)[0])
    elims, elab, edis, est = oracle.range_search_preassigned(oracle_lists(oracle, metric, cen, want), xq, radius, ck)
    return want, radius, elims, elab, edis, est


def input_conditions(name, expr, model, elims, elab):
    """what the oracle's output must exercise (asserted before the engine is asked anything)"""
    per_query = np.diff(elims)
    if expr == "bits_none":
        assert elims[-1] == 0
        return
    # a result from a second mask word: its position in the PARENT's list is 64 or more
    pos = {}
    for ids in model.ids:
        for p, i in enumerate(ids):
            pos[int(i)] = p
    assert any(pos[int(i)] >= 64 for i in elab), (name, expr, "no result beyond a list's first mask word")
    if expr == "bits_1pct":  # (it keeps ~30 entries in all: no query can have 64)
        assert (per_query == 0).any() and (per_query > 0).any(), (name, expr, per_query)
    else:
        assert per_query.max() > 64, (name, expr, int(per_query.max()))


@pytest.mark.parametrize("expr", RANGE_SELECTORS, ids=lambda e: e if isinstance(e, str) else "not_" + e[1])
@pytest.mark.parametrize("name", ["sift_l2", "l2_96", "ip_96", "ragged", "bytes_200", "bytes_960"])
def test_range_search_selected_equals_the_oracle_and_the_subset(capi, oracle, name, expr):
    """lims, labels and distances of range_search_preassigned_selected and range_search_selected: the oracle's over the filtered
    lists and the subset's range_search, in order; byte codes on / off, "filter" unset / 0; ndis is the parent's"""
    metric, cen, assign, xb, xq, model = case(name)
    want, radius, elims, elab, edis, est = range_expected(oracle, capi, name, expr)
    input_conditions(name, expr, model, elims, elab)
    cd, ck = coarse(oracle, name)
    pst = oracle.range_search_preassigned(oracle_lists(oracle, metric, cen, model), xq, radius, ck)[3]

    def equal(got, exp, what):
        assert np.array_equal(got[0], exp[0]), (what, "lims")
        assert np.array_equal(got[1], exp[1]), (what, "labels")
        assert np.array_equal(bits(got[2]), bits(exp[2])), (what, "distances")

    parent = handle(capi, metric, cen, xb, assign, 1)
    before = parent.range_search(xq, radius, NPROBE, keys=ck)
    with Made(capi, parent, model, expr) as s:
        # (the subset of an expression: its members as an ID_BATCH -- the ids of a case are unique)
        sub = parent.subset(capi.SUBSET_ID_BATCH, 0, 0, np.concatenate(want.ids).astype(np.int64))
        assert sub.ntotal == s.info()[1] == sum(len(i) for i in want.ids)
        for byte in byte_settings(name):
            for filt in (None, 0):
                for h in (parent, sub):
                    h.set_byte_codes(byte)
                    h.set_option("filter", filt)
                what = (byte, filt)
                from_sub = sub.range_search(xq, radius, NPROBE, keys=ck)
                equal(from_sub, (elims, elab, edis), what + ("subset",))
                parent.stats(reset=True)
                got = parent.range_search_selected(s, xq, radius, NPROBE, keys=ck)
                st = parent.stats()
                equal(got, (elims, elab, edis), what + ("preassigned",))
                equal(got, from_sub, what + ("preassigned / subset",))
                assert st["ndis"] == pst[1], (st, pst)
                got = parent.range_search_selected(s, xq, radius, NPROBE)
                equal(got, (elims, elab, edis), what + ("coarse",))
                equal(got, sub.range_search(xq, radius, NPROBE), what + ("coarse / subset",))
        sub.close()
        parent.set_byte_codes(1)
        parent.set_option("filter", None)
        equal(parent.range_search(xq, radius, NPROBE, keys=ck), before, "unfiltered, with selectors alive")
    equal(parent.range_search(xq, radius, NPROBE, keys=ck), before, "unfiltered, after")
    parent.close()


def test_range_search_selected_refuses_a_foreign_or_stale_selector(capi, oracle):
    metric, cen, assign, xb, xq, model = case("l2_96")
    cd, ck = coarse(oracle, "l2_96")
    parent = handle(capi, metric, cen, xb, assign, 1)
    other = handle(capi, metric, cen, xb, assign, 1)
    L = capi.lib()
    s = parent.selector(capi.SUBSET_ID_MOD, 3, 1)
    for keys in (None, ck):
        with pytest.raises(capi.EngineError) as e:
            other.range_search_selected(s, xq, 1.0, NPROBE, keys=keys)
        assert e.value.code == -2 and "another index" in L.amd_ivf_last_error().decode()
    parent.add(xq[:2].copy(), np.array([7000, 7001], dtype=np.int64), np.array([0, 3]))
    for keys in (None, ck):
        with pytest.raises(capi.EngineError) as e:
            parent.range_search_selected(s, xq, 1.0, NPROBE, keys=keys)
        assert e.value.code == -2 and "stale" in L.amd_ivf_last_error().decode()
    s.close()
    other.close()
    parent.close()


# ------------------------------------------------------------------------------------------------ 5. tickets
@pytest.mark.parametrize("name", ["sift_l2", "l2_96"])
def test_selected_searches_in_flight(capi, oracle, name):
    """six tickets alternating between mod_3_1 and NOT(mod_3_1) over two query ranges at depth 3: every waited result is the
    synchronous call's and the oracle's; a selector is not destroyed under its tickets; a stale or foreign selector gets no ticket"""
    metric, cen, assign, xb, xq, _ = case(name)
    nlist, d = cen.shape
    model = Model(nlist, d, xb, assign)
    L = capi.lib()
    parent = handle(capi, metric, cen, xb, assign, 1)
    other = handle(capi, metric, cen, xb, assign, 1)
    parent.set_queries(xq)
    parent.set_async_depth(3)
    exprs = ["mod_3_1", ("not", "mod_3_1")]
    exp = [knn_expected(oracle, capi, name, e) for e in exprs]
    ranges = [(0, 100), (100, NQ - 100)]

    def refused(f, word):
        with pytest.raises(capi.EngineError) as e:
            f()
        assert e.value.code == -2, e.value
        assert word in L.amd_ivf_last_error().decode(), L.amd_ivf_last_error()

    base = parent.selector(*selector(capi, "mod_3_1", model)[0])
    sels = [base, ~base]
    sync = [[parent.search_resident_selected(s, start, n, K, NPROBE) for start, n in ranges] for s in sels]
    for w in range(2):
        for r, (start, n) in enumerate(ranges):
            same(sync[w][r], exp[w][1][start:start + n], exp[w][2][start:start + n], ("synchronous", w, r))
    tickets = [(parent.submit_search_resident_selected(sels[i % 2], *ranges[(i // 2) % 2], K, NPROBE), i % 2, (i // 2) % 2) for i in range(6)]
    for s in sels:
        refused(s.destroy, "tickets that search under this selector")
    # amd_ivf_add with selected tickets out is refused as for any ticket
    refused(lambda: parent.add(xq[:1].copy(), np.array([9000], dtype=np.int64), np.array([0])), "tickets")
    for t, w, r in tickets:
        D, I, _, _ = parent.wait(t)
        start, n = ranges[r]
        same((D, I), *sync[w][r], ("ticket / synchronous", w, r))
        same((D, I), exp[w][1][start:start + n], exp[w][2][start:start + n], ("ticket / oracle", w, r))
    # a foreign selector, then a stale one: -2 and no ticket
    foreign = other.selector(capi.SUBSET_ID_MOD, 3, 1)
    counts = parent.async_counts()
    assert counts[0] == 6
    refused(lambda: parent.submit_search_resident_selected(foreign, 0, 10, K, NPROBE), "another index")
    foreign.close()
    other.close()
    sels[1].destroy()  # (its tickets have been waited for)
    parent.add(xq[:1].copy(), np.array([9000], dtype=np.int64), np.array([0]))
    refused(lambda: parent.submit_search_resident_selected(base, 0, 10, K, NPROBE), "stale")
    assert parent.async_counts() == counts
    assert not getattr(parent, "_tickets", None)
    base.destroy()
    parent.set_async_depth(0)
    parent.close()
