"""Trace training (the search pass of Error_sys::sys_train: amd_ivf_train_samples, _x, _pre -> train_core -> the training branch of
replay_kernel) against the pinned CPU oracle, bit for bit: D, I and EVERY raw (sum_angle, kscaling) trace as uint32 views, then
Trace::SB over them.  Adaptive-search tests feed the same traces to both sides, so a wrong sample passes them all; here the
samples themselves are held, at the shapes the three small goldens of test_gpu_parity.py do not reach:

  sweep     nlist 24 (the smallest legal) .. 4096 (ranked prefix, many threshold rounds, four enqueued ahead), powers of two or not;
            K 4 .. 130 on both sides of the register heap, multiples of 4 or not (the row stride is K / 4, rounded down); byte,
            small-integer, float and unit-norm (inner product) data; calls of 1 .. 200 queries, both sides of the 20-query coarse
            regime; the three entry points, each held to the same oracle call
  offsets   three uneven slices [0, a), [a, a + 1), [a + 1, T) with the raw arrays carried from call to call, one variant
            prefilled with another negative bit pattern than -1
  gt edge   one entry below K / 4 of every query's ground truth moved by a factor 1 +- 1e-5 (1 + e), e in {+-3e-2, +-1e-3, 0}: the
            match test `(double)(df / kdis) < 1e-5 || (double)df < 1e-5` (float division, double compare) then ends the query's row
            there (no match -> kscaling < 0 -> partial row) or lets it run on; kdis == 0 (queries that are base vectors: df / kdis
            is NaN, the absolute test decides); a gt that matches nothing; lists so small that the heap still holds FLT_MAX at the
            first stages; inner product over lists shorter than K, which the oracle and the engine both refuse
  refusals  start + n > train_num and max_topk < 4 (either would be a device write behind the raw buffers)

No tolerance anywhere.  The oracle restates IndexIVF::search_preassigned's training branch and is held to the compiled reference by
test_oracle_golden.py::test_auncel_offline.  test_inputs_reach_what_they_are_for needs no GPU: it builds every case, runs the oracle
side only and asserts that the inputs do what the list above says (both outcomes of the edge, list sizes, samples at every stage).

Shapes are capped at nb 120 000, d 100, 200 queries; the oracle's side of a case takes 0.05 - 1.5 s (the assignment of the base
vectors to 4096 centroids is most of it), the engine's three calls well under a second."""
import functools

import numpy as np
import pytest

L2, IP = 1, 0
PREFILL_ALT = np.array([0xC0A01234], dtype=np.uint32).view(np.float32)[0]  # -5.00222..: negative, not -1, not a sample's value


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
#        name              nlist    K    d  kind        nb   nq
SWEEP = [("n24_k4",           24,   4,  12, "bytes",   3000,   1),
         ("n24_k20",          24,  20,  30, "float",   3000,  19),
         ("n24_k7_ip",        24,   7,  32, "unit",    6000,  20),
         ("n64_k10",          64,  10,  64, "small",   6000,  70),
         ("n64_k127",         64, 127,  32, "bytes",   8000, 200),
         ("n64_k10_ip",       64,  10, 100, "unit",   40000,  19),
         ("n100_k128",       100, 128,  30, "float",  10000,  20),
         ("n100_k130",       100, 130,  12, "bytes",  10000,  70),
         ("n100_k4_ip",      100,   4,  64, "unit",   40000, 200),
         ("n256_k100",       256, 100,  32, "bytes",  20000, 200),
         ("n256_k7",         256,   7, 100, "float",  20000,   1),
         ("n256_k130",       256, 130,  64, "small",  20000,  19),
         ("n256_k128",       256, 128,  12, "float",  20000,  70),
         ("n1000_k100",     1000, 100,  32, "bytes",  30000, 200),  # sparse: 30 vectors a list, the heap holds FLT_MAX at stage 1
         ("n1000_k20",      1000,  20,  30, "small",  30000,  20),
         ("n1000_k127",     1000, 127,  64, "float",  30000,  70),
         ("n2048_k10",      2048,  10,  12, "bytes",  40000,  19),
         ("n2048_k130",     2048, 130,  32, "float",  60000,  70),
         ("n2048_k100",     2048, 100, 100, "small",  40000, 200),
         ("n4096_k20",      4096,  20,  30, "float",  60000, 200),
         ("n4096_k128",     4096, 128,  64, "bytes", 120000,  70),
         ("n4096_k7",       4096,   7,  32, "small",  60000,   1),
         ("n4096_k127",     4096, 127,  12, "bytes",  60000,  20)]
#        name              nlist    K    d  kind        nb   nq   a (offsets: slices [0, a), [a, a + 1), [a + 1, nq))
OFFSETS = [("off_bytes",     256,  20,  32, "bytes",  20000,  70,  19),
           ("off_float",     100,   7,  30, "float",  10000,  41,  20)]
#        name              nlist    K    d  kind        nb   nq   (zero: a quarter of the queries are copies of base vectors)
EDGES = [("edge_bytes",      256, 100,  32, "bytes",  20000, 200),
         ("edge_float",      256, 128,  32, "float",  20000, 200),
         ("edge_float_k40",  128,  40,  30, "float",  10000, 200)]
EDGE_E = np.array([-3e-2, -1e-3, 0.0, 1e-3, 3e-2])
# inner product over 2048 lists of about 5 vectors, K 10: a heap that is not full yet hands -FLT_MAX to the acos table
IP_SHORT = ("ip_short_lists", 2048, 10, 32, "unit", 10000, 20)
SHAPES = {r[0]: r for r in SWEEP + [o[:7] for o in OFFSETS] + EDGES + [IP_SHORT]}


def READ(nlist):
    """entries of a coarse ranking that a training pass reads: nlist / 8 + 1 probes, nlist / 8 + 20 entries in set_online"""
    return nlist // 8 + 21


def ntraces(nlist):
    n = 0
    while (1 << n) <= nlist // 8:
        n += 1
    return n


def drawer(rs, kind, nblobs, d):
    """the data kinds of test_gpu_random_adaptive.py, and small integers of either sign (fused arithmetic, no byte codes)"""
    centres = rs.rand(nblobs, d) * 160.0

    def draw(n):
        c = centres[rs.randint(0, nblobs, n)]
        if kind == "bytes":
            return np.floor(np.clip(c + rs.randn(n, d) * 30.0, 0, 255)).astype(np.float32)
        if kind == "small":
            return np.clip(np.round(c / 16.0 - 5.0 + rs.randn(n, d) * 2.0), -15, 15).astype(np.float32)
        if kind == "float":
            return (c / 40.0 + rs.randn(n, d) * 0.8).astype(np.float32)
        x = c / 160.0 - 0.5 + rs.randn(n, d) * 0.15
        return (x / np.linalg.norm(x, axis=1, keepdims=True) * 0.9).astype(np.float32)
    return draw


class Case:
    pass


@functools.lru_cache(maxsize=None)
def build_case(name):
    """data, lists and the oracle's rankings of one shape, from seeds: computed once a process and left unchanged"""
    from oracle import pyoracle as orc
    _, nlist, K, d, kind, nb, nq = SHAPES[name]
    rs = np.random.RandomState(9100 + sorted(SHAPES).index(name))
    c = Case()
    c.name, c.nlist, c.K, c.d, c.kind, c.nq = name, nlist, K, d, kind, nq
    c.metric = IP if kind == "unit" else L2
    draw = drawer(rs, kind, max(nlist // 2, 8), d)
    c.xb, c.xq = draw(nb), draw(nq)
    if name == "edge_bytes":
        c.xq[::4] = c.xb[rs.choice(nb, len(c.xq[::4]), replace=False)]  # kdis == 0 at rank 0
    c.cen = (c.xb[rs.choice(nb, nlist, replace=False)] + rs.randn(nlist, d) * 1e-3).astype(np.float32)
    _, a = orc.knn(c.metric, c.xb, c.cen, 1, nthreads=8)
    c.assign = a[:, 0].copy()
    c.lists = orc.Lists(c.metric, c.cen, c.xb, c.assign)
    # The engine ranks the centroids itself in two of the three entry points, and inside a run of exactly equal distances its
    # order is the reference's only for calls of fewer than 20 queries (include/auncel_amd.h).  The noise on the centroids keeps
    # such runs to chance; a query that still has one in the part a training pass reads is drawn again.
    for _ in range(20):
        c.cd, c.ck = orc.knn(c.metric, c.xq, c.cen, nlist, nthreads=8)
        tied = np.nonzero((np.diff(c.cd[:, :READ(nlist)], axis=1) == 0).any(axis=1))[0]
        if len(tied) == 0:
            break
        for q in tied:
            c.xq[q] = c.xb[rs.randint(nb)] if name == "edge_bytes" and q % 4 == 0 else draw(1)[0]
    assert len(tied) == 0, name
    c.gt, _ = orc.knn(c.metric, c.xq, c.xb, K, nthreads=8)
    c.interdis = orc.interdis(c.metric, c.cen)
    c.arcos = orc.arcos_table()
    c.ntr = ntraces(nlist)
    for v in (c.xb, c.xq, c.cen, c.assign, c.cd, c.ck, c.gt, c.interdis, c.arcos):
        v.setflags(write=False)
    return c


def new_raw(c, T, fill=-1.0):
    return [np.full((T * (c.K // 4), 2), fill, dtype=np.float32) for _ in range(c.ntr)]


def oracle_train(c, lo, hi, T, raw, gt=None):
    """the oracle over queries [lo, hi) of the case, as ids lo .. hi - 1 of T; raw is updated in place"""
    from oracle import pyoracle as orc
    return orc.train_samples(c.lists, c.xq[lo:hi], c.K, c.ck[lo:hi], c.cd[lo:hi], c.interdis, c.arcos, c.gt if gt is None else gt, lo, T, raw)


@functools.lru_cache(maxsize=None)
def expected(name):
    """one oracle call over all the case's queries from offset 0: (D, I, raw)"""
    c = build_case(name)
    raw = new_raw(c, c.nq)
    D, I = oracle_train(c, 0, c.nq, c.nq, raw)
    for v in [D, I] + raw:
        v.setflags(write=False)
    return D, I, raw


def written(raw_i, K, fill=-1.0):
    """samples written per query of one raw trace (a written sample's kscaling is positive)"""
    y = bits(raw_i[:, 1]).reshape(-1, K // 4)
    return (y != bits(np.float32(fill))).sum(axis=1)


def edge_gt(c):
    """the exact ground truth with one entry p < K / 4 of every query moved to the edge of the match test -> (gt, p)"""
    rs = np.random.RandomState(77)
    q = np.arange(c.nq)
    p = rs.randint(0, c.K // 4, c.nq)
    sign = rs.choice([-1.0, 1.0], c.nq)
    gt = c.gt.copy()
    gt[q, p] = (c.gt[q, p].astype(np.float64) * (1.0 + sign * 1e-5 * (1.0 + EDGE_E[q % 5]))).astype(np.float32)
    return gt, p


@functools.lru_cache(maxsize=None)
def expected_edge(name):
    """(gt, p, D, I, raw, share of rows that end at p, share that run on) at the last stage, from the oracle alone"""
    c = build_case(name)
    gt, p = edge_gt(c)
    raw = new_raw(c, c.nq)
    D, I = oracle_train(c, 0, c.nq, c.nq, raw, gt=gt)
    cnt = written(raw[-1], c.K)
    for v in [gt, D, I] + raw:
        v.setflags(write=False)
    return gt, p, D, I, raw, float((cnt == p).mean()), float((cnt > p).mean())


def no_match_gt(c):
    return np.full((c.nq, c.K), -5.0, dtype=np.float32)  # L2: every kdis >= 0, so df >= 5 and df / kdis > 1 (or inf / NaN)


# ---- the inputs do what they are for: no GPU ----------------------------------------------------------------------------------------
def test_inputs_reach_what_they_are_for(oracle):
    assert {r[1] for r in SWEEP} == {24, 64, 100, 256, 1000, 2048, 4096}
    assert {r[2] for r in SWEEP} == {4, 7, 10, 20, 100, 127, 128, 130}
    assert {r[3] for r in SWEEP} == {12, 30, 32, 64, 100}
    assert {r[4] for r in SWEEP} == {"bytes", "small", "float", "unit"}
    assert {r[6] for r in SWEEP} == {1, 19, 20, 70, 200}
    assert all(r[5] <= 120000 and r[3] <= 100 and r[6] <= 200 for r in SHAPES.values())
    for row in SWEEP:
        c = build_case(row[0])
        if c.metric == IP:
            assert c.lists.sizes.min() >= c.K, (c.name, int(c.lists.sizes.min()))
        assert (np.diff(c.cd[:, :READ(c.nlist)], axis=1) != 0).all(), c.name
        _, _, raw = expected(c.name)
        for i in range(c.ntr):
            assert written(raw[i], c.K).sum() >= 1, (c.name, "no sample at stage", 1 << i)
    # lists so small that the heap still holds FLT_MAX: partial rows at the first stage, full rows at the last
    c = build_case("n1000_k100")
    _, _, raw = expected(c.name)
    full = [float((written(r, c.K) == c.K // 4).mean()) for r in raw]
    print("n1000_k100: share of full rows per stage", full)
    assert full[0] < 0.9 and full[-1] == 1.0
    for name, *_ in OFFSETS:
        c = build_case(name)
        assert (np.diff(c.cd[:, :READ(c.nlist)], axis=1) != 0).all(), name
    # the edge: both outcomes, a quarter each at least, at the last stage
    for name, *_ in EDGES:
        c = build_case(name)
        _, p, _, _, _, ends, runs_on = expected_edge(name)
        print(f"{name}: row ends at p {ends:.3f}, runs on {runs_on:.3f}")
        assert ends >= 0.25 and runs_on >= 0.25, (name, ends, runs_on)
    c = build_case("edge_bytes")
    assert (c.gt[::4, 0] == 0).all() and (c.gt[1::4, 0] > 0).all()  # kdis == 0 for a quarter of the queries
    raw = new_raw(c, c.nq)
    oracle_train(c, 0, c.nq, c.nq, raw, gt=no_match_gt(c))
    assert all((bits(r) == bits(np.float32(-1))).all() for r in raw)
    # inner product over lists shorter than K: the reference's rule refuses
    c = build_case(IP_SHORT[0])
    assert np.median(c.lists.sizes) < c.K
    with pytest.raises(RuntimeError):
        oracle_train(c, 0, c.nq, c.nq, new_raw(c, c.nq))


# ---- the engine ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def make_handle(capi, c):
    h = capi.Handle(c.d, c.nlist, c.metric, 0)
    h.set_centroids(c.cen)
    h.set_lists_from_assign(c.xb, c.assign)
    h.set_interdis(None)
    h.set_queries(c.xq)
    return h


def train(h, form, c, lo, hi, T, raw, gt=None):
    """one engine call over queries [lo, hi) of the case through one of the three entry points"""
    gt = c.gt if gt is None else gt
    if form == "resident":
        return h.train_samples(lo, hi - lo, c.K, gt, T, raw)
    if form == "x":
        return h.train_samples_x(c.xq[lo:hi], lo, c.K, gt, T, raw)
    return h.train_samples_pre(c.xq[lo:hi], lo, c.ck[lo:hi], c.cd[lo:hi], c.K, gt, T, raw)


FORMS = ("resident", "x", "pre")


def assert_same(tag, D, I, raw, eD, eI, eraw):
    assert np.array_equal(I, eI), tag
    assert np.array_equal(bits(D), bits(eD)), tag
    for i, (r, e) in enumerate(zip(raw, eraw)):
        bad = np.argwhere(bits(r) != bits(e))
        assert len(bad) == 0, (tag, f"raw trace {i}: {len(bad)} of {e.size} differ, first at {bad[0]}: {r[tuple(bad[0])]} for {e[tuple(bad[0])]}")


def assert_same_traces(capi, oracle, tag, raw):
    for i, r in enumerate(raw):
        for got, want in zip(capi.trace_sb(r.copy()), oracle.trace_sb(r)):
            assert np.array_equal(bits(got), bits(want)), (tag, "trace_sb", i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r[0] for r in SWEEP])
def test_sweep_against_oracle(capi, oracle, monkeypatch, name):
    c = build_case(name)
    monkeypatch.setenv("AUNCEL_AMD_REPLAY_NLD", "16" if [r[0] for r in SWEEP].index(name) % 2 else "32")
    eD, eI, eraw = expected(name)
    assert np.array_equal(bits(capi.arcos_table()), bits(c.arcos))
    h = make_handle(capi, c)
    for form in FORMS:
        raw = new_raw(c, c.nq)
        D, I = train(h, form, c, 0, c.nq, c.nq, raw)
        rounds = h.last_timing()["rounds"]
        print(name, form, "rounds", rounds)
        assert_same((name, form), D, I, raw, eD, eI, eraw)
        if c.nlist >= 256:
            assert rounds >= 2, (name, form, rounds)  # the threshold rounds are what was compared
    assert_same_traces(capi, oracle, name, eraw)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", OFFSETS, ids=[o[0] for o in OFFSETS])
def test_slices_carry_the_raw_arrays(capi, oracle, monkeypatch, shape, form):
    """three uneven slices: rows outside a call's slice keep their bits, the end is the oracle's with the same offsets and a single
    call's.  off_float starts from another negative bit pattern than -1: unwritten slots keep it."""
    name, a = shape[0], shape[7]
    c = build_case(name)
    monkeypatch.setenv("AUNCEL_AMD_REPLAY_NLD", "16" if name == "off_float" else "32")
    T, w = c.nq, c.K // 4
    fill = PREFILL_ALT if name == "off_float" else np.float32(-1)
    slices = [(0, a), (a, a + 1), (a + 1, T)]
    h = make_handle(capi, c)
    raw, eraw = new_raw(c, T, fill), new_raw(c, T, fill)
    for lo, hi in slices:
        before = [r.copy() for r in raw]
        D, I = train(h, form, c, lo, hi, T, raw)
        eD, eI = oracle_train(c, lo, hi, T, eraw)
        for i in range(c.ntr):
            outside = np.ones(T * w, dtype=bool)
            outside[lo * w:hi * w] = False
            assert np.array_equal(bits(raw[i])[outside], bits(before[i])[outside]), (name, form, lo, hi, "rows outside the slice", i)
        assert_same((name, form, lo, hi), D, I, raw, eD, eI, eraw)
    one, eone = new_raw(c, T, fill), new_raw(c, T, fill)
    D, I = train(h, form, c, 0, T, T, one)
    eD, eI = oracle_train(c, 0, T, T, eone)
    assert_same((name, form, "one call"), D, I, one, eD, eI, eone)
    assert_same((name, form, "slices against one call"), D, I, raw, eD, eI, one)
    assert any((bits(r) == bits(fill)).any() for r in raw) and any((bits(r) != bits(fill)).any() for r in raw)
    assert_same_traces(capi, oracle, name, raw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [e[0] for e in EDGES])
def test_ground_truth_at_the_edge_of_the_match_test(capi, oracle, monkeypatch, name):
    c = build_case(name)
    monkeypatch.setenv("AUNCEL_AMD_REPLAY_NLD", "16" if name == "edge_float" else "32")
    gt, p, eD, eI, eraw, ends, runs_on = expected_edge(name)
    assert ends >= 0.25 and runs_on >= 0.25, (name, ends, runs_on)  # (the oracle's output alone)
    h = make_handle(capi, c)
    for form in FORMS:
        raw = new_raw(c, c.nq)
        D, I = train(h, form, c, 0, c.nq, c.nq, raw, gt=gt)
        assert_same((name, form), D, I, raw, eD, eI, eraw)
    assert_same_traces(capi, oracle, name, eraw)


@pytest.mark.gpu
def test_ground_truth_that_matches_nothing(capi, oracle):
    """every kscaling is negative: no sample anywhere, D and I as ever"""
    c = build_case("edge_bytes")
    gt = no_match_gt(c)
    eraw = new_raw(c, c.nq)
    eD, eI = oracle_train(c, 0, c.nq, c.nq, eraw, gt=gt)
    h = make_handle(capi, c)
    for form in FORMS:
        raw = new_raw(c, c.nq, PREFILL_ALT)
        D, I = train(h, form, c, 0, c.nq, c.nq, raw, gt=gt)
        assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD)), form
        assert all((bits(r) == bits(PREFILL_ALT)).all() for r in raw), form


@pytest.mark.gpu
def test_inner_product_over_lists_shorter_than_k_is_refused(capi, oracle):
    c = build_case(IP_SHORT[0])
    with pytest.raises(RuntimeError):
        oracle_train(c, 0, c.nq, c.nq, new_raw(c, c.nq))
    h = make_handle(capi, c)
    for form in FORMS:
        with pytest.raises(capi.EngineError):
            train(h, form, c, 0, c.nq, c.nq, new_raw(c, c.nq))


@pytest.mark.gpu
def test_rows_outside_the_raw_arrays_are_refused(capi, oracle):
    """start + n > train_num and max_topk < 4 would be device writes behind the raw buffers: refused on the host, by name, with the
    raw arrays untouched and the handle as good as before"""
    c = build_case("off_float")
    T = c.nq
    h = make_handle(capi, c)
    for form in FORMS:
        for lo, hi, tn in ((0, T, T - 1), (1, T, T - 1), (T - 1, T, 0), (5, 6, 5)):
            raw = new_raw(c, T, PREFILL_ALT)
            with pytest.raises(capi.EngineError, match="train_num"):
                train(h, form, c, lo, hi, tn, raw)
            assert all((bits(r) == bits(PREFILL_ALT)).all() for r in raw), (form, lo, hi, tn)
        for K in (0, 1, 3):
            raw = new_raw(c, T, PREFILL_ALT)  # (sized for the case's K: a row of K / 4 = 0 samples has no array to check)
            gt = np.ascontiguousarray(c.gt[:, :max(K, 1)])
            with pytest.raises(capi.EngineError, match="max_topk"):
                if form == "resident":
                    h.train_samples(0, T, K, gt, T, raw)
                elif form == "x":
                    h.train_samples_x(c.xq, 0, K, gt, T, raw)
                else:
                    h.train_samples_pre(c.xq, 0, c.ck, c.cd, K, gt, T, raw)
            assert all((bits(r) == bits(PREFILL_ALT)).all() for r in raw), (form, K)
        raw, eraw = new_raw(c, T), new_raw(c, T)
        D, I = train(h, form, c, 0, T, T, raw)
        eD, eI = oracle_train(c, 0, T, T, eraw)
        assert_same(("after the refusals", form), D, I, raw, eD, eI, eraw)
