"""A subset index cut on the device (amd_ivf_subset, ivf_subset.hip): list l of the subset holds the members of the parent's list l in
the parent's order.  The expected lists are made here with numpy (the loop of IndexIVF::copy_subset_to); the device layout is compared
with a handle that takes those lists through amd_ivf_set_lists (all eight digest words), and every search with the pinned CPU oracle
over them.  Every comparison is of bits or of integers."""
import numpy as np
import pytest

from test_gpu_update import BYTE_CASES, K, NPROBE, NQ, Model, bits, handle, make_case, new_rows, warm

pytestmark = pytest.mark.gpu

CASES = ["sift_l2", "l2_96", "ip_96", "odd_30", "ragged", "bytes_200", "bytes_960"]
SELECTORS = ["range_third", "mod_3_1", "slice_mid", "bits_half", "bits_1pct", "bits_all", "bits_none", "batch_200", "bits_lists"]


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def id_bits(ids, nwords):
    """the ID_BITS selector that holds `ids` (all of them in [0, 64 nwords))"""
    w = np.zeros(nwords, np.uint64)
    ids = np.asarray(ids, np.int64)
    np.bitwise_or.at(w, ids >> 6, np.uint64(1) << (ids & 63).astype(np.uint64))
    return w


def selector(capi, name, model):
    """(kind, a1, a2, sel) and the membership rule as a function of (ids of a list, list number, entries before the list)"""
    all_ids = np.concatenate(model.ids)
    nt, top = len(all_ids), int(all_ids.max()) + 1
    nwords = (top + 63) // 64 + 2
    rs = np.random.RandomState(17)
    if name == "range_third":
        a1, a2 = top // 3, 2 * top // 3
        return (capi.SUBSET_ID_RANGE, a1, a2, None), lambda ids, l, seen: (ids >= a1) & (ids < a2)
    if name == "mod_3_1":
        return (capi.SUBSET_ID_MOD, 3, 1, None), lambda ids, l, seen: np.fmod(ids, 3) == 1  # (C++ %: the sign of the dividend)
    if name == "slice_mid":
        a1, a2 = nt // 4, 3 * nt // 4

        def rule(ids, l, seen):  # IndexIVF::copy_subset_to, type 2
            nxt = seen + len(ids)
            i0 = nxt * a1 // nt - seen * a1 // nt
            i1 = nxt * a2 // nt - seen * a2 // nt
            pos = np.arange(len(ids))
            return (pos >= i0) & (pos < i1)
        return (capi.SUBSET_SLICE, a1, a2, None), rule
    if name.startswith("bits_"):
        if name == "bits_half":
            chosen = all_ids[rs.rand(nt) < 0.5]
        elif name == "bits_1pct":
            chosen = all_ids[rs.rand(nt) < 0.01]
        elif name == "bits_all":
            chosen = all_ids
        elif name == "bits_none":
            chosen = all_ids[:0]
        else:  # whole lists emptied, others cut across a 64-entry boundary, the rest kept whole
            parts = []
            for l, ids in enumerate(model.ids):
                if l in (0, 1, 9):
                    continue
                parts.append(ids[:70] if l == 2 else ids[60:130] if l == 3 else ids[63:65] if l == 4 else ids)
            chosen = np.concatenate(parts)
        held = set(int(v) for v in chosen)
        return (capi.SUBSET_ID_BITS, 0, 0, id_bits(chosen, nwords)), lambda ids, l, seen: np.array([int(v) in held for v in ids], bool)
    assert name == "batch_200"
    picked = rs.choice(all_ids, 150, replace=False)
    batch = np.concatenate([picked, picked[:30], np.array([top + 5, top + 77, -3, 10 ** 12] * 5)]).astype(np.int64)
    rs.shuffle(batch)
    assert len(batch) == 200
    held = set(int(v) for v in batch)
    return (capi.SUBSET_ID_BATCH, 0, 0, batch), lambda ids, l, seen: np.array([int(v) in held for v in ids], bool)


def filtered(model, rule):
    """the loop of copy_subset_to: the members of every list, in order"""
    out = Model.__new__(Model)
    out.d, out.codes, out.ids = model.d, [], []
    seen = 0
    for l in range(len(model.ids)):
        keep = rule(model.ids[l], l, seen) if len(model.ids[l]) else np.zeros(0, bool)
        out.codes.append(model.codes[l][keep].copy())
        out.ids.append(model.ids[l][keep].copy())
        seen += len(model.ids[l])
    return out


def from_lists(capi, metric, cen, model):
    """the same lists through amd_ivf_set_lists"""
    h = capi.Handle(cen.shape[1], cen.shape[0], metric, 0)
    h.set_centroids(cen)
    h.set_lists([len(i) for i in model.ids], model.codes, model.ids)
    return h


def oracle_lists(oracle, metric, cen, model):
    xb, assign, ids = model.flat()
    return oracle.Lists(metric, cen, xb.reshape(-1, cen.shape[1]), assign, ids)


def check_searches(oracle, h, metric, cen, model, xq):
    """search, search_preassigned and range_search of `h` against the oracle over `model`'s lists"""
    lists = oracle_lists(oracle, metric, cen, model)
    cd, ck = oracle.knn(metric, xq, cen, NPROBE)
    eD, eI, _ = oracle.search_preassigned(lists, xq, K, ck, cd)
    D, I = h.search_preassigned(xq, K, ck, cd)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    D, I = h.search(xq, K, NPROBE)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    fin = eD[:, 0][np.isfinite(eD[:, 0]) & (np.abs(eD[:, 0]) < 1e37)]
    radius = float(np.median(fin)) * (1.5 if metric == 1 else 0.7) if fin.size else 1.0
    elims, elab, edis, _ = oracle.range_search_preassigned(lists, xq, radius, ck)
    lims, lab, dis = h.range_search(xq, radius, NPROBE, keys=ck)
    assert np.array_equal(lims, elims) and np.array_equal(lab, elab) and np.array_equal(bits(dis), bits(edis))
    return eD, eI


def check_subset(capi, sub, ref, want, xq, parent_ntotal, sel):
    """layout (all eight digest words after the same warm-up), lists, sizes and the transfer report of a subset"""
    nlist = sub.nlist
    looked, kept, h2d, d2h = sub.last_subset()
    kept_want = sum(len(i) for i in want.ids)
    assert looked == parent_ntotal and kept == kept_want == sub.ntotal == ref.ntotal
    sel_bytes = 0 if sel is None else 8 * len(sel)
    assert h2d <= sel_bytes + 16 * (nlist + 1) + 65536, sub.last_subset()
    assert d2h <= 16 * (nlist + 1) + 65536, sub.last_subset()
    warm(sub, xq)
    warm(ref, xq)
    ds, dr = sub.layout_digest(), ref.layout_digest()
    assert ds == dr, [i for i in range(8) if ds[i] != dr[i]]
    for l in range(nlist):
        assert sub.list_size(l) == len(want.ids[l])
        c, i = sub.get_list(l)
        assert np.array_equal(i, want.ids[l]), l
        assert np.array_equal(bits(c), bits(want.codes[l])), l
    return ds


@pytest.mark.parametrize("sel_name", SELECTORS)
@pytest.mark.parametrize("name", CASES)
def test_subset_equals_set_lists_of_the_filtered_lists(capi, oracle, name, sel_name):
    metric, cen, assign, xb, xq = make_case(name)
    nlist, d = cen.shape
    parent = handle(capi, metric, cen, xb, assign, 1)
    model = Model(nlist, d, xb, assign)
    (kind, a1, a2, sel), rule = selector(capi, sel_name, model)
    want = filtered(model, rule)
    sub = parent.subset(kind, a1, a2, sel)
    ref = from_lists(capi, metric, cen, want)
    dg = check_subset(capi, sub, ref, want, xq, len(xb), sel)
    if sub.ntotal:
        if name in BYTE_CASES:
            assert dg[3], "no byte fragments"
        else:
            assert dg[4] and dg[5] and dg[6], "the warm-up did not build every fp32 copy"
    eD, eI = check_searches(oracle, sub, metric, cen, want, xq)
    if sub.ntotal and name in BYTE_CASES:
        assert sub.scan_arith() == 2
    if sel_name == "mod_3_1":  # one case per metric (and shape) also through a clone and through a ticket
        c = sub.clone()
        D, I = c.search(xq, K, NPROBE)
        assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
        c.close()
        sub.set_queries(xq)
        t = sub.submit_search_resident(0, NQ, K, NPROBE)
        D, I, _, _ = sub.wait(t)
        assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    for h in (sub, ref, parent):
        h.close()


def make_traces(rs, nlist):
    traces, ntr = [], 1
    while (1 << ntr) <= nlist // 8:
        ntr += 1
    for _ in range(ntr):
        n = int(rs.randint(5, 40))
        tx = np.sort(rs.rand(n) * 25.0).astype(np.float32) + np.arange(n, dtype=np.float32) * 1e-3
        traces.append((tx, (0.5 + rs.rand(n) * 2.5).astype(np.float32), (rs.rand(n) * 0.5).astype(np.float32)))
    return traces


@pytest.mark.parametrize("sel_name", ["mod_3_1", "range_third"])
def test_adaptive_search_of_a_subset(capi, oracle, sel_name):
    """interdis and the tuner are set on the parent BEFORE the cut: (D, I, my_nprobe) of the subset's adaptive search equal the
    oracle's over the filtered lists, which also shows that the Auncel state was copied"""
    metric, cen, assign, xb, xq = make_case("ragged", seed=8, nlist=32)  # (the tuner wants nlist > nlist / 8 + 20)
    nlist, d = cen.shape
    Kmax, qk = 20, 10
    rs = np.random.RandomState(21)
    parent = handle(capi, metric, cen, xb, assign, 1)
    model = Model(nlist, d, xb, assign)
    traces = make_traces(rs, nlist)
    arcos = capi.arcos_table()
    req = rs.choice([0.8, 0.9, 0.95], size=NQ).astype(np.float32)
    parent.set_interdis(None)
    parent.set_tuner(Kmax, traces, arcos)
    (kind, a1, a2, sel), rule = selector(capi, sel_name, model)
    want = filtered(model, rule)
    sub = parent.subset(kind, a1, a2, sel)
    parent.close()
    fb, fa, fi = want.flat()
    olists = oracle.Lists(metric, cen, fb, fa, fi)
    cd, ck = oracle.knn(metric, xq, cen, nlist)
    gtD, _ = oracle.knn(metric, xq, fb, Kmax)
    tun = oracle.Tuner(oracle.interdis(metric, cen), traces, Kmax, NQ, arcos=arcos)
    stt = tun.struct(qk, req, 2.0, 1.0, gt_D=gtD)
    eD, eI, _ = oracle.search_preassigned(olists, xq, Kmax, ck, cd, tuner=stt, offset=0, nthreads=1)
    sub.set_queries(xq)
    my_np = np.zeros(NQ, dtype=np.uint64)
    t_rec = np.zeros(NQ, dtype=np.float32)
    D, I = sub.search_adaptive(0, NQ, qk, 2.0, 1.0, req, my_np, t_rec, gt_D=gtD)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    assert np.array_equal(my_np.astype(np.int64), tun.my_nprobe.astype(np.int64))
    sub.close()


def test_byte_eligibility_is_taken_over_the_kept_values(capi, oracle):
    """20 rows of non-integer values keep the parent off the byte path; the selector leaves them out, and the subset is on it"""
    metric, cen, assign, xb, xq = make_case("sift_l2")
    nlist, d = cen.shape
    rs = np.random.RandomState(9)
    parent = handle(capi, metric, cen, xb, assign, 1)
    model = Model(nlist, d, xb, assign)
    lists = rs.randint(0, nlist, size=20)
    x = (new_rows(rs, "sift_l2", cen, lists) + 0.5).astype(np.float32)
    ids = np.arange(100000, 100020, dtype=np.int64)
    parent.add(x, ids, lists)
    model.add(x, ids, lists)
    parent.search(xq, K, NPROBE)
    assert parent.scan_arith() in (0, 1) and parent.layout_digest()[3] == 0
    want = filtered(model, lambda i, l, seen: (i >= 0) & (i < len(xb)))
    sub = parent.subset(capi.SUBSET_ID_RANGE, 0, len(xb))
    ref = from_lists(capi, metric, cen, want)
    dg = check_subset(capi, sub, ref, want, xq, len(xb) + 20, None)
    assert dg[3] != 0 and dg[3] == ref.layout_digest()[3]
    sub.search(xq, K, NPROBE)
    assert sub.scan_arith() == 2
    check_searches(oracle, sub, metric, cen, want, xq)
    assert sub.scan_arith() == 2
    # ... and the other way: a subset of the non-integer rows alone is not byte-eligible
    odd = parent.subset(capi.SUBSET_ID_RANGE, 100000, 100020)
    assert odd.ntotal == 20 and odd.layout_digest()[3] == 0
    for h in (odd, sub, ref, parent):
        h.close()
    # the same by magnitude at d = 960 (960 * 132^2 <= 2^24 < 960 * 133^2): three rows holding 133 keep the parent's searches in fp32;
    # a subset without them searches its byte codes, one with them does not -- each as a handle that uploaded the kept lists in full
    metric, cen, assign, xb, xq = make_case("bytes_960")
    nlist, d = cen.shape
    parent = handle(capi, metric, cen, xb, assign, 1)
    model = Model(nlist, d, xb, assign)
    x = xb[20:23].copy()
    x[:, 0] = 133.0
    lists, ids = np.array([2, 2, 11]), np.arange(100000, 100003, dtype=np.int64)
    parent.add(x, ids, lists)
    model.add(x, ids, lists)
    check_searches(oracle, parent, metric, cen, model, xq)
    assert parent.scan_arith() == 1
    for a1, a2, arith in ((0, len(xb), 2), (len(xb) // 2, 100003, 1), (100000, 100003, 1)):
        want = filtered(model, lambda i, l, seen: (i >= a1) & (i < a2))
        sub = parent.subset(capi.SUBSET_ID_RANGE, a1, a2)
        ref = from_lists(capi, metric, cen, want)
        dg = check_subset(capi, sub, ref, want, xq, len(xb) + 3, None)
        assert dg[3] != 0
        for h in (sub, ref):
            check_searches(oracle, h, metric, cen, want, xq)
            assert h.scan_arith() == arith, (a1, a2, h.scan_arith())
            h.close()
    parent.close()


@pytest.mark.parametrize("name", ["sift_l2", "ip_96"])
def test_parent_is_untouched_and_the_subset_stands_alone(capi, oracle, name):
    metric, cen, assign, xb, xq = make_case(name)
    nlist, d = cen.shape
    rs = np.random.RandomState(4)
    parent = handle(capi, metric, cen, xb, assign, 1)
    model = Model(nlist, d, xb, assign)
    warm(parent, xq)
    # a pending add, made without a search in between, is in the subset
    lists = rs.randint(0, nlist, size=90)
    x = new_rows(rs, name, cen, lists)
    ids = np.arange(3001, 3001 + 3 * len(lists), 3, dtype=np.int64)  # (3001 % 3 == 1: the selector keeps them)
    parent.add(x, ids, lists)
    model.add(x, ids, lists)
    (kind, a1, a2, sel), rule = selector(capi, "mod_3_1", model)
    want = filtered(model, rule)
    assert sum(int(np.isin(ids, i).sum()) for i in want.ids) == len(ids)
    sub = parent.subset(kind, a1, a2, sel)
    before = parent.layout_digest()
    D0, I0 = parent.search(xq, K, NPROBE)
    ref = from_lists(capi, metric, cen, want)
    check_subset(capi, sub, ref, want, xq, len(xb) + len(lists), sel)
    # a subset of the subset equals the subset by the intersection
    (kind2, b1, b2, sel2), rule2 = selector(capi, "range_third", model)
    both = filtered(model, lambda i, l, seen: rule(i, l, seen) & rule2(i, l, seen))
    subsub = sub.subset(kind2, b1, b2, sel2)
    direct = parent.subset(capi.SUBSET_ID_BITS, 0, 0, id_bits(np.concatenate(both.ids), (int(np.concatenate(model.ids).max()) >> 6) + 2))
    ref2 = from_lists(capi, metric, cen, both)
    check_subset(capi, subsub, ref2, both, xq, sub.ntotal, sel2)
    warm(direct, xq)
    assert direct.layout_digest() == subsub.layout_digest()
    # the parent: same layout, same results
    assert parent.layout_digest() == before
    D1, I1 = parent.search(xq, K, NPROBE)
    assert np.array_equal(I0, I1) and np.array_equal(bits(D0), bits(D1))
    check_searches(oracle, parent, metric, cen, model, xq)
    # the subset borrows nothing: it searches after the parent is gone
    parent.close()
    sub.close()
    check_searches(oracle, subsub, metric, cen, both, xq)
    for h in (subsub, direct, ref, ref2):
        h.close()


def test_refusals(capi, oracle):
    metric, cen, assign, xb, xq = make_case("l2_96")
    nlist, d = cen.shape
    parent = handle(capi, metric, cen, xb, assign, 1)
    model = Model(nlist, d, xb, assign)
    sub = parent.subset(capi.SUBSET_ID_MOD, 2, 0)
    L = capi.lib()

    def refused(f, word=None):
        with pytest.raises(capi.EngineError) as e:
            f()
        assert e.value.code == -2, e.value
        if word:
            assert word in L.amd_ivf_last_error().decode()

    # every mutator on a subset
    sizes = [sub.list_size(l) for l in range(nlist)]
    refused(lambda: sub.add(xb[:2], np.array([7, 8]), np.array([0, 1])), "read-only")
    refused(lambda: sub.set_lists_from_assign(xb, assign), "read-only")
    refused(lambda: sub.update_lists(sizes, np.array([(3 << 32) | 0], np.uint64), np.array([5]), xb[:1]), "read-only")
    refused(lambda: sub.remove_ids(np.array([0, 2, 4])), "read-only")
    refused(lambda: sub.set_centroids(cen), "read-only")
    assert sub.ntotal == sum(sizes)
    # bad arguments
    refused(lambda: parent.subset(3, 2, 0))
    refused(lambda: parent.subset(4, 2, 0))
    refused(lambda: parent.subset(7, 0, 0))
    refused(lambda: parent.subset(-1, 0, 0))
    refused(lambda: parent.subset(capi.SUBSET_ID_MOD, 0, 0))
    refused(lambda: parent.subset(capi.SUBSET_ID_MOD, -3, 0))
    refused(lambda: parent.subset(capi.SUBSET_SLICE, 10, 5))
    refused(lambda: parent.subset(capi.SUBSET_SLICE, 0, len(xb) + 1))
    out = capi.C.c_void_p()
    for kind in (capi.SUBSET_ID_BITS, capi.SUBSET_ID_BATCH):
        assert L.amd_ivf_subset(parent._h, kind, capi.C.c_int64(0), capi.C.c_int64(0), None, capi.C.c_size_t(4), capi.C.byref(out)) == -2
    assert L.amd_ivf_subset(parent._h, 0, capi.C.c_int64(0), capi.C.c_int64(5), None, capi.C.c_size_t(0), None) == -2
    # a clone; a ticket out on the parent (whose later wait still returns the right result)
    c = parent.clone()
    refused(lambda: c.subset(capi.SUBSET_ID_MOD, 2, 0))
    c.close()
    lists = oracle_lists(oracle, metric, cen, model)
    cd, ck = oracle.knn(metric, xq, cen, NPROBE)
    eD, eI, _ = oracle.search_preassigned(lists, xq, K, ck, cd)
    parent.set_queries(xq)
    t = parent.submit_search_resident(0, NQ, K, NPROBE)
    refused(lambda: parent.subset(capi.SUBSET_ID_MOD, 2, 0), "tickets")
    D, I, _, _ = parent.wait(t)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    again = parent.subset(capi.SUBSET_ID_MOD, 2, 0)
    assert again.ntotal == sub.ntotal
    # an empty SLICE and an empty parent are valid
    assert parent.subset(capi.SUBSET_SLICE, 5, 5).ntotal == 0
    empty = capi.Handle(d, nlist, metric, 0)
    empty.set_centroids(cen)
    assert empty.subset(capi.SUBSET_ID_RANGE, 0, 100).ntotal == 0


def test_subset_at_scale(capi, oracle):
    """the index of tests/test_gpu_scale.py (1M x 128, byte-valued, IVF1024), ID_MOD 10 / 3: 64 queries at nprobe 16 against the
    oracle over the filtered lists, and the layout against amd_ivf_set_lists of them"""
    from auncel_amd import synth
    nb, nq, d, nlist = 1_000_000, 64, 128, 1024
    xb, xq = synth.sift_like(nb, nq, d=d, nblobs=2000, sigma=35.0, seed=1234)
    rs = np.random.RandomState(3)
    cen = xb[rs.choice(nb, nlist, replace=False)] + rs.uniform(-0.4, 0.4, size=(nlist, d)).astype(np.float32)  # non-integer
    h = capi.Handle(d, nlist, capi.METRIC_L2, 0)
    h.set_centroids(cen)
    h.add(xb)
    model = Model.__new__(Model)
    model.d, model.codes, model.ids = d, [], []
    for l in range(nlist):
        c, i = h.get_list(l)
        model.codes.append(c)
        model.ids.append(i)
    want = filtered(model, lambda i, l, seen: np.fmod(i, 10) == 3)
    sub = h.subset(capi.SUBSET_ID_MOD, 10, 3)
    looked, kept, h2d, d2h = sub.last_subset()
    assert looked == nb and kept == sub.ntotal == nb // 10
    assert h2d <= 16 * (nlist + 1) + 65536 and d2h <= 16 * (nlist + 1) + 65536
    ref = from_lists(capi, 1, cen, want)
    sub.search(xq, 10, 16)
    ref.search(xq, 10, 16)
    assert sub.scan_arith() == 2
    assert sub.layout_digest() == ref.layout_digest()
    fb, fa, fi = want.flat()
    lists = oracle.Lists(1, cen, fb, fa, fi)
    cd, ck = oracle.knn(1, xq, cen, 16, nthreads=8)
    eD, eI, _ = oracle.search_preassigned(lists, xq, 10, ck, cd, nthreads=8)
    D, I = sub.search(xq, 10, 16)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    for x in (sub, ref, h):
        x.close()
