"""The adaptive rule and its training branch under an id selector (amd_ivf_search_adaptive_selected, _x_selected, _selected_each,
amd_ivf_train_samples_selected): every output is, bit for bit, what the unselected call returns on amd_ivf_subset of the same
selector, and what the pinned CPU oracle returns over the lists with the non-members removed.  The worlds, the selectors and the
oracle's answers are adaptive_selected_cases.py's; test_adaptive_selected_cases_cpu.py asserts what these tests lean on (queries that
run past the first round, equal distances inside the kept set, runs of equal coarse distances in reach, probed lists that keep
nothing).  Where the reference throws (a tuned inner-product search whose first probe leaves the heap short of Kmax members) the
subset's call and the call under test are refused alike.

World B's rankings hold runs of equal coarse distances, and a call of 20 queries and more orders them by centroid number unless
"coarse_ties" says otherwise: the comparisons with the oracle run under "redo" (2) -- the regime that searches the queries concerned
again, under their own selectors -- the comparisons with the subset under that and under the default.  Every comparison is of bits
or of integers."""
import numpy as np
import pytest

import adaptive_selected_cases as ac

pytestmark = pytest.mark.gpu

NS = (1, 4, 19, 20, 300)  # fuse_small (<= 4), spec_finish (< 20), the chained rounds, the large-call paths (>= 256)
NRES = 300


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


@pytest.fixture(scope="module")
def arcos(capi):
    return capi.arcos_table()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def resident(w):
    """the world's queries repeated to 300 resident rows, and their bounds: query i is query i % nq"""
    idx = np.arange(NRES) % w.nq
    return idx, np.ascontiguousarray(w.xq[idx]), np.ascontiguousarray(w.req[idx])


def open_parent(capi, arcos, w):
    h = capi.Handle(w.d, w.nlist, w.metric, 0)
    h.set_centroids(w.cen)
    h.set_lists_from_assign(w.xb, w.assign)
    h.set_interdis(None)
    h.set_tuner(w.K, w.traces, arcos)
    h.set_queries(resident(w)[1])
    return h


_parents = {}


@pytest.fixture(scope="module")
def parents(capi, arcos):
    """one parent a world, with interdis, tuner and the resident queries set before any subset is cut"""
    def get(name, metric):
        if (name, metric) not in _parents:
            _parents[(name, metric)] = open_parent(capi, arcos, ac.world(name, metric))
        h = _parents[(name, metric)]
        h.set_byte_codes(1)
        h.set_option("coarse_ties", None)
        h.set_option("selected_skip_empty", None)
        return h
    yield get
    for h in _parents.values():
        h.close()
    _parents.clear()


def cut(h, name, metric, sel):
    (kind, a1, a2, arr), _ = ac.selector(name, metric, sel)
    s = h.selector(kind, a1, a2, arr)
    sub = h.subset(kind, a1, a2, arr)
    sub.set_queries(resident(ac.world(name, metric))[1])
    return s, sub


def gt_rows(gtD, idx):
    return np.ascontiguousarray(gtD[idx])


def call(f, w, start, n, gt=None, profile=0):
    """one adaptive call over resident queries [start, start + n): (D, I, my_nprobe, t_recalls) of those queries"""
    _, _, req = resident(w)
    my_np = np.zeros(NRES, np.uint64)
    t_rec = np.zeros(NRES, np.float32)
    D, I = f(start, n, w.qk, w.mult, w.std_m, req, my_np, t_rec, gt_D=gt, profile=profile)
    return D, I, my_np[start:start + n].astype(np.int64), t_rec[start:start + n].copy()


def same(a, b, what=""):
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(bits(a[0]), bits(b[0])), what
    assert np.array_equal(a[2], b[2]), what
    assert np.array_equal(bits(a[3]), bits(b[3])), what


def refused_alike(capi, f, g):
    msgs = []
    for fn in (f, g):
        with pytest.raises(capi.EngineError) as e:
            fn()
        assert e.value.code == -2
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "arcos" in msgs[0]


@pytest.mark.parametrize("sel", ac.SELECTORS)
@pytest.mark.parametrize("byte_codes", [1, 0])
@pytest.mark.parametrize("name,metric", ac.WORLDS)
def test_selected_equals_subset_and_oracle(capi, oracle, arcos, parents, name, metric, byte_codes, sel):
    w = ac.world(name, metric)
    h = parents(name, metric)
    s, sub = cut(h, name, metric, sel)
    idx = resident(w)[0]
    try:
        for x in (h, sub):
            x.set_byte_codes(byte_codes)
        try:
            ref = ac.reference(oracle, arcos, name, metric, sel)
        except RuntimeError:
            refused_alike(capi, lambda: call(sub.search_adaptive, w, 0, w.nq),
                          lambda: call(lambda *a, **k: h.search_adaptive_selected(s, *a, **k), w, 0, w.nq))
            # ... and the handle serves the next call
            ref_all = ac.reference(oracle, arcos, name, metric, "everything")
            with h.selector(*ac.selector(name, metric, "everything")[0]) as s_all:
                got = call(lambda *a, **k: h.search_adaptive_selected(s_all, *a, **k), w, 0, 4)
            assert np.array_equal(got[1], ref_all.I[:4]) and np.array_equal(got[2], ref_all.my_nprobe[:4])
            return
        gt = gt_rows(ref.gtD, idx)
        selected = lambda *a, **k: h.search_adaptive_selected(s, *a, **k)
        for ties in ((None, 2) if name == "B" else (None,)):
            for x in (h, sub):
                x.set_option("coarse_ties", ties)
            want = call(sub.search_adaptive, w, 0, w.nq, gt)
            got = call(selected, w, 0, w.nq, gt)
            same(got, want, (sel, ties))
            if ties == 2 or name == "A":
                assert np.array_equal(got[1], ref.I) and np.array_equal(bits(got[0]), bits(ref.D)) and np.array_equal(got[2], ref.my_nprobe)
            # the planner's skip changes no output
            h.set_option("selected_skip_empty", 0)
            same(call(selected, w, 0, w.nq, gt), want, (sel, ties, "no skip"))
            h.set_option("selected_skip_empty", None)
            # the caller's rows instead of the resident ones
            my_np = np.zeros(w.nq, np.uint64)
            t_rec = np.zeros(w.nq, np.float32)
            D, I = h.search_adaptive_x_selected(s, w.xq, 0, w.qk, w.mult, w.std_m, w.req, my_np, t_rec, gt_D=ref.gtD)
            same((D, I, my_np.astype(np.int64), t_rec), want, (sel, ties, "x"))
            if sel == "everything":
                same(call(h.search_adaptive, w, 0, w.nq, gt), got, "unselected")
        # profile bit 0: t_recalls against the FILTERED ground truth
        pref = ac.reference(oracle, arcos, name, metric, sel, profile=True)
        want = call(sub.search_adaptive, w, 0, w.nq, gt, profile=1)
        got = call(selected, w, 0, w.nq, gt, profile=1)
        same(got, want, "profile")
        assert np.array_equal(bits(got[3]), bits(pref.t_recalls))
    finally:
        s.close()
        sub.close()


@pytest.mark.parametrize("sel", ["range_10pct", "sparse", "few"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_call_size(capi, oracle, arcos, parents, name, sel):
    """n = 1, 4, 19, 20, 300 (the queries repeated): every path through the first selection, and a start that is not 0"""
    w = ac.world(name, ac.L2)
    h = parents(name, ac.L2)
    s, sub = cut(h, name, ac.L2, sel)
    ref = ac.reference(oracle, arcos, name, ac.L2, sel)
    idx = resident(w)[0]
    gt = gt_rows(ref.gtD, idx)
    try:
        for x in (h, sub):
            x.set_option("coarse_ties", 2)
        for n in NS:
            start = 0 if n == NRES else 7
            rows = idx[start:start + n]
            got = call(lambda *a, **k: h.search_adaptive_selected(s, *a, **k), w, start, n, gt)
            same(got, call(sub.search_adaptive, w, start, n, gt), (sel, n))
            assert np.array_equal(got[1], ref.I[rows]) and np.array_equal(bits(got[0]), bits(ref.D[rows])), (sel, n)
            assert np.array_equal(got[2], ref.my_nprobe[rows]), (sel, n)
            if name == "B" and sel == "range_10pct" and n == NRES:
                # queries read runs of equal coarse distances: the pass is not patched under a selector, they are searched again
                assert h.last_tie_patched() == 0 and h.last_tie_redone() > 0
    finally:
        s.close()
        sub.close()


@pytest.mark.parametrize("ties", [None, 2])
@pytest.mark.parametrize("name,metric", [("A", ac.L2), ("B", ac.L2), ("B", ac.IP)])
def test_a_selector_per_query(capi, oracle, arcos, parents, name, metric, ties):
    """three selectors interleaved over the batch: row i is the single-selector call's row i under sels[sel_of[i]]; nsel == 1 is that
    call"""
    w = ac.world(name, metric)
    h = parents(name, metric)
    names = ["range_10pct", "mod_3_1", "sparse"] if metric == ac.L2 else ["everything", "everything", "everything"]
    sels = [h.selector(*ac.selector(name, metric, nm)[0]) for nm in names]
    try:
        h.set_option("coarse_ties", ties)
        for n, start in ((w.nq, 0), (19, 5), (NRES, 0)):
            singles = [call(lambda *a, **k: h.search_adaptive_selected(s, *a, **k), w, start, n) for s in sels]
            sel_of = (np.arange(n) * 7 + 1) % 3
            got = call(lambda *a, **k: h.search_adaptive_selected_each(sels, sel_of, *a, **k), w, start, n)
            for j in range(3):
                m = sel_of == j
                same(tuple(v[m] for v in got), tuple(v[m] for v in singles[j]), (n, j))
            if ties == 2 and name == "B" and n == NRES:
                assert h.last_tie_patched() == 0 and h.last_tie_redone() > 0  # (the second pass carried the re-indexed sel_of)
            one = call(lambda *a, **k: h.search_adaptive_selected_each(sels[2:], np.zeros(n, np.int64), *a, **k), w, start, n)
            same(one, singles[2], (n, "nsel 1"))
            if ties == 2 and metric == ac.L2:
                idx = resident(w)[0][start:start + n]
                for j, nm in enumerate(names):
                    ref = ac.reference(oracle, arcos, name, metric, nm)
                    m = sel_of == j
                    assert np.array_equal(got[1][m], ref.I[idx[m]]) and np.array_equal(got[2][m], ref.my_nprobe[idx[m]]), (n, nm)
    finally:
        for s in sels:
            s.close()


@pytest.mark.parametrize("sel", ["mod_3_1", "sparse"])
def test_training_under_a_selector(capi, oracle, arcos, parents, sel):
    """raw, D and I of amd_ivf_train_samples_selected equal the subset's amd_ivf_train_samples and the oracle's over the filtered lists"""
    w = ac.world("A", ac.L2)
    h = parents("A", ac.L2)
    s, sub = cut(h, "A", ac.L2, sel)
    ref = ac.reference(oracle, arcos, "A", ac.L2, sel)
    T, K = w.nq, w.K
    ntr = ac.ntraces(w.nlist)
    fresh = lambda: [np.full((T * (K // 4), 2), -1.0, np.float32) for _ in range(ntr)]
    try:
        raw_o = fresh()
        eD, eI = oracle.train_samples(ref.lists, w.xq, K, ref.ck, ref.cd, oracle.interdis(ac.L2, w.cen), arcos, ref.gtD, 0, T, raw_o)
        raw_s, raw_g = fresh(), fresh()
        sD, sI = sub.train_samples(0, T, K, ref.gtD, T, raw_s)
        gD, gI = h.train_samples_selected(s, 0, T, K, ref.gtD, T, raw_g)
        assert np.array_equal(gI, sI) and np.array_equal(bits(gD), bits(sD))
        assert np.array_equal(gI, eI) and np.array_equal(bits(gD), bits(eD))
        for a, b, c in zip(raw_g, raw_s, raw_o):
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
        assert any((a != -1.0).any() for a in raw_g)
    finally:
        s.close()
        sub.close()


def test_a_small_selected_call_after_a_large_unselected_one(capi, oracle, arcos, parents):
    """the stale-workspace case: masks, logs, hints and row space of a 300-query unselected search stay behind in the handle"""
    w = ac.world("B", ac.L2)
    h = parents("B", ac.L2)
    new = open_parent(capi, arcos, w)
    sels = [x.selector(*ac.selector("B", ac.L2, "sparse")[0]) for x in (h, new)]
    try:
        call(h.search_adaptive, w, 0, NRES)
        for n in (4, 19, 40):
            got = call(lambda *a, **k: h.search_adaptive_selected(sels[0], *a, **k), w, 3, n)
            want = call(lambda *a, **k: new.search_adaptive_selected(sels[1], *a, **k), w, 3, n)
            same(got, want, n)
            call(h.search_adaptive, w, 0, NRES)
    finally:
        for s in sels:
            s.close()
        new.close()


def test_skip_saves_scan_bytes_and_changes_nothing(capi, oracle, arcos, parents):
    """under the sparse selector the planner makes no row for a list that keeps nothing: the call's scan bytes (a count, not a time)
    are strictly fewer, its outputs the same"""
    w = ac.world("B", ac.L2)
    h = parents("B", ac.L2)
    with h.selector(*ac.selector("B", ac.L2, "sparse")[0]) as s:
        out, scanned = {}, {}
        for skip in (0, 1):
            h.set_option("selected_skip_empty", skip)
            assert h.get_option("selected_skip_empty") == skip
            out[skip] = call(lambda *a, **k: h.search_adaptive_selected(s, *a, **k), w, 0, w.nq)
            scanned[skip] = h.last_timing()["scan_bytes"]
        h.set_option("selected_skip_empty", None)
        assert h.get_option("selected_skip_empty") == 1
        same(out[0], out[1])
        print(scanned)
        assert 0 < scanned[1] < scanned[0], scanned


def test_refusals(capi, arcos):
    w = ac.world("A", ac.L2)
    h, other = open_parent(capi, arcos, w), open_parent(capi, arcos, w)
    L = capi.lib()
    s = h.selector(*ac.selector("A", ac.L2, "mod_3_1")[0])
    foreign = other.selector(*ac.selector("A", ac.L2, "mod_3_1")[0])

    def refused(f, word):
        with pytest.raises(capi.EngineError) as e:
            f()
        assert e.value.code == -2 and word in L.amd_ivf_last_error().decode(), e.value

    sel1 = lambda x: (lambda *a, **k: h.search_adaptive_selected(x, *a, **k))
    each = lambda xs, so: (lambda *a, **k: h.search_adaptive_selected_each(xs, so, *a, **k))
    raw = [np.full((8 * (w.K // 4), 2), -1.0, np.float32) for _ in range(ac.ntraces(w.nlist))]
    gt = np.zeros((NRES, w.K), np.float32)
    refused(lambda: call(sel1(foreign), w, 0, 8), "another index")
    refused(lambda: call(each([s, foreign], np.zeros(8, np.int64)), w, 0, 8), "another index")
    refused(lambda: call(each([s], np.full(8, 1, np.int64)), w, 0, 8), "not below nsel")
    refused(lambda: call(each([s, None], np.zeros(8, np.int64)), w, 0, 8), "null")
    refused(lambda: call(sel1(s), w, 0, 8, profile=2), "overhead_profile")
    refused(lambda: call(sel1(s), w, NRES - 4, 8), "out of bounds")
    refused(lambda: h.train_samples_selected(foreign, 0, 8, w.K, gt, 8, raw), "another index")
    c = h.clone()
    refused(lambda: call(lambda *a, **k: c.search_adaptive_selected(s, *a, **k), w, 0, 8), "amd_ivf_clone")
    refused(lambda: c.train_samples_selected(s, 0, 8, w.K, gt, 8, raw), "amd_ivf_clone")
    c.close()
    call(sel1(s), w, 0, 8)
    # amd_ivf_add changes the lists: the selector is stale from there on
    h.add(w.xb[:2].copy(), np.array([w.nb + 1, w.nb + 2]), np.array([0, 3]))
    refused(lambda: call(sel1(s), w, 0, 8), "stale")
    refused(lambda: call(each([s], np.zeros(8, np.int64)), w, 0, 8), "stale")
    refused(lambda: h.train_samples_selected(s, 0, 8, w.K, gt, 8, raw), "stale")
    s.close()
    foreign.close()
    h.close()
    other.close()
