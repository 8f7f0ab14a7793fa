"""Changes of a device-resident index in place (amd_ivf_add / amd_ivf_update_lists / amd_ivf_remove_ids, ivf_update.hip): after every
step of a scripted sequence, the handle that applies its journal in HBM ("incremental" 1) holds bit for bit the device layout of a
handle that sends every list again ("incremental" 0) -- offsets, rows, ids and every derived copy -- and searches of it equal the
CPU oracle over the final lists."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, NPROBE, NQ = 10, 8, 256
# byte-valued cases: name -> (d, metric, largest value m, half-width of the noise around a centre).  The wide ones sit at the edge of
# the byte-code rule d m^2 <= 2^24 and are scanned by the any-d form of the MFMA kernel (more than four K-steps)
BYTE_CASES = {"sift_l2": (128, 1, 255, 25), "bytes_200": (200, 1, 255, 25), "bytes_960": (960, 0, 132, 12)}


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_case(name, seed=3, nlist=16):
    rs = np.random.RandomState(seed)
    nb = 3000
    if name == "sift_l2":
        d, metric = 128, 1
        cen = rs.randint(10, 200, size=(nlist, d)).astype(np.float32)
        assign = rs.randint(0, nlist, size=nb)
        xb = np.clip(cen[assign] + rs.randint(-25, 26, size=(nb, d)), 0, 255).astype(np.float32)
        xq = np.clip(cen[rs.randint(0, nlist, size=NQ)] + rs.randint(-25, 26, size=(NQ, d)), 0, 255).astype(np.float32)
        return metric, cen, assign, xb, xq
    if name in BYTE_CASES:
        d, metric, m, w = BYTE_CASES[name]
        cen = rs.randint(m // 25, m - m // 5, size=(nlist, d)).astype(np.float32)
        assign = rs.randint(0, nlist, size=nb)
        xb = np.clip(cen[assign] + rs.randint(-w, w + 1, size=(nb, d)), 0, m).astype(np.float32)
        xq = np.clip(cen[rs.randint(0, nlist, size=NQ)] + rs.randint(-w, w + 1, size=(NQ, d)), 0, m).astype(np.float32)
        xb[0], xq[0] = m, m  # the largest value is met on both sides
        return metric, cen, assign, xb, xq
    d, metric = {"l2_96": (96, 1), "ip_96": (96, 0), "odd_30": (30, 1), "ragged": (64, 1)}[name]
    cen = rs.randn(nlist, d).astype(np.float32)
    assign = rs.randint(0, nlist, size=nb)
    if name == "ragged":
        assign[assign == 1] = 0
        assign[assign == 5] = 4
        assign[assign == 6] = 4
    xb = (cen[assign] + 0.3 * rs.randn(nb, d)).astype(np.float32)
    xq = (cen[rs.randint(0, nlist, size=NQ)] + 0.3 * rs.randn(NQ, d)).astype(np.float32)
    return metric, cen, assign, xb, xq


class Model:
    """the lists as a Python restatement of the reference keeps them"""

    def __init__(self, nlist, d, xb, assign):
        self.codes = [xb[assign == l].copy() for l in range(nlist)]
        self.ids = [np.nonzero(assign == l)[0].astype(np.int64) for l in range(nlist)]
        self.d = d

    def add(self, x, ids, lists):
        for v, i, l in zip(x, ids, lists):
            self.codes[l] = np.vstack([self.codes[l], v[None]])
            self.ids[l] = np.append(self.ids[l], i)

    def remove_ids(self, sel):
        """IndexIVF::remove_ids (IndexIVF.cpp:955-987)"""
        sel, total = set(int(v) for v in sel), 0
        for l in range(len(self.ids)):
            c, ids = self.codes[l].copy(), self.ids[l].copy()
            n = len(ids)
            j = 0
            while j < n:
                if int(ids[j]) in sel:
                    n -= 1
                    ids[j], c[j] = ids[n], c[n]
                else:
                    j += 1
            total += len(ids) - n
            self.codes[l], self.ids[l] = c[:n], ids[:n]
        return total

    def update(self, sizes, where, ids, codes):
        for l, s in enumerate(sizes):
            n = len(self.ids[l])
            if s < n:
                self.codes[l], self.ids[l] = self.codes[l][:s].copy(), self.ids[l][:s].copy()
            elif s > n:
                self.codes[l] = np.vstack([self.codes[l], np.zeros((s - n, self.d), np.float32)])
                self.ids[l] = np.append(self.ids[l], -np.ones(s - n, np.int64))
        for w, i, c in zip(where, ids, codes):
            l, p = int(w) >> 32, int(w) & 0xffffffff
            self.codes[l][p], self.ids[l][p] = c, i

    def flat(self):
        nl = len(self.ids)
        xb = np.vstack([self.codes[l] for l in range(nl)]).astype(np.float32)
        assign = np.concatenate([np.full(len(self.ids[l]), l, np.int64) for l in range(nl)])
        return xb, assign, np.concatenate(self.ids)


def handle(capi, metric, cen, xb, assign, incremental):
    h = capi.Handle(cen.shape[1], cen.shape[0], metric, 0)
    h.set_option("incremental", incremental)
    h.set_centroids(cen)
    h.set_lists_from_assign(xb, assign)
    return h


def warm(h, xq):
    """searches that build every derived copy: the byte path (where the lists qualify), fp32 through the fp16 and the fp32 filter,
    the lane-ordered copy of the dense rounds"""
    h.search(xq, K, NPROBE)
    h.set_byte_codes(0)
    for f in (2, 1):
        h.set_option("filter", f)
        h.search(xq, K, NPROBE)
    h.set_option("filter", float("nan"))
    h.set_byte_codes(1)


def check_step(A, B, model, xq, what):
    warm(A, xq)
    warm(B, xq)
    da, db = A.layout_digest(), B.layout_digest()
    assert da == db, (what, [i for i in range(8) if da[i] != db[i]])
    mode, h2d, written, _ = A.last_update()
    assert mode == 1, (what, A.last_update())
    assert h2d <= written * (4 * ((A.d + 3) // 4 * 4) + 16) + 16 * (A.nlist + 1) + 65536, (what, A.last_update())
    for l in range(A.nlist):
        c, i = A.get_list(l)
        assert np.array_equal(i, model.ids[l]), (what, l)
        assert np.array_equal(bits(c), bits(model.codes[l])), (what, l)


def oracle_check(oracle, h, metric, cen, model, xq):
    xb, assign, ids = model.flat()
    lists = oracle.Lists(metric, cen, xb, assign, ids)
    cd, ck = oracle.knn(metric, xq, cen, NPROBE)
    eD, eI, _ = oracle.search_preassigned(lists, xq, K, ck, cd)
    D, I = h.search_preassigned(xq, K, ck, cd)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    D, I = h.search(xq, K, NPROBE)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    return eD, eI


def new_rows(rs, name, cen, lists):
    if name == "sift_l2":
        return np.clip(cen[lists] + rs.randint(-25, 26, size=(len(lists), cen.shape[1])), 0, 255).astype(np.float32)
    if name in BYTE_CASES:
        _, _, m, w = BYTE_CASES[name]
        return np.clip(cen[lists] + rs.randint(-w, w + 1, size=(len(lists), cen.shape[1])), 0, m).astype(np.float32)
    return (cen[lists] + 0.3 * rs.randn(len(lists), cen.shape[1])).astype(np.float32)


@pytest.mark.parametrize("name", ["sift_l2", "l2_96", "ip_96", "odd_30", "ragged", "bytes_200", "bytes_960"])
def test_layout_equals_full_upload(capi, oracle, name):
    metric, cen, assign, xb, xq = make_case(name)
    nlist, d = cen.shape
    rs = np.random.RandomState(11)
    A = handle(capi, metric, cen, xb, assign, 1)
    B = handle(capi, metric, cen, xb, assign, 0)
    model = Model(nlist, d, xb, assign)
    warm(A, xq)
    warm(B, xq)
    assert A.layout_digest() == B.layout_digest()
    if name not in BYTE_CASES:
        dg = A.layout_digest()
        assert dg[4] and dg[5] and dg[6], "the warm-up did not build every fp32 copy"
    else:
        assert A.layout_digest()[3], "no byte fragments"
        A.search(xq, K, NPROBE)
        assert A.scan_arith() == 2
    next_id = [len(xb) + 1000]

    def add(lists):
        lists = np.asarray(lists, np.int64)
        x = new_rows(rs, name, cen, lists)
        ids = np.arange(next_id[0], next_id[0] + len(lists), dtype=np.int64)
        next_id[0] += len(lists)
        for h in (A, B):
            h.add(x, ids, lists)
        model.add(x, ids, lists)

    sizes = [len(i) for i in model.ids]
    # adds that cross 64-vector boundaries upwards, several lists at once, one list that was empty (ragged: 1, 5, 6)
    grow = (64 - sizes[2] % 64) + 3
    add([2] * grow + [3, 7, 7] + [1] * 5)
    check_step(A, B, model, xq, "add")
    # removals: the middle and the end of a list, a whole list, and enough of list 2 to cross a boundary downwards
    sel = [model.ids[3][len(model.ids[3]) // 2], model.ids[3][-1], model.ids[8][0]] + list(model.ids[9]) + list(model.ids[2][:grow + 5])
    want = model.remove_ids(sel)
    assert A.remove_ids(np.array(sel)) == want and B.remove_ids(np.array(sel)) == want
    check_step(A, B, model, xq, "remove")
    # update_lists: overwrite entries, grow one list, shrink another, refill the emptied list
    sizes = [len(i) for i in model.ids]
    new_sizes = list(sizes)
    new_sizes[4] += 3
    new_sizes[10] = max(0, new_sizes[10] - 2)
    new_sizes[9] = 2
    where = [(4 << 32) | p for p in range(sizes[4], sizes[4] + 3)] + [(9 << 32) | 0, (9 << 32) | 1] + [(11 << 32) | 0, (12 << 32) | 1]
    lists = [w >> 32 for w in where]
    x = new_rows(rs, name, cen, np.array(lists))
    ids = np.arange(next_id[0], next_id[0] + len(where), dtype=np.int64)
    next_id[0] += len(where)
    for h in (A, B):
        h.update_lists(new_sizes, np.array(where, np.uint64), ids, x)
    model.update(new_sizes, where, ids, x)
    check_step(A, B, model, xq, "update_lists")
    add(list(range(nlist)))
    check_step(A, B, model, xq, "add again")
    eD, eI = oracle_check(oracle, A, metric, cen, model, xq)
    if name in BYTE_CASES:
        assert A.scan_arith() == 2
    D, I = B.search(xq, K, NPROBE)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    c = A.clone()
    D, I = c.search(xq, K, NPROBE)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    c.close()
    A.close()
    B.close()


def test_byte_eligibility_flips_as_the_full_path(capi, oracle):
    metric, cen, assign, xb, xq = make_case("sift_l2")
    nlist, d = cen.shape
    A = handle(capi, metric, cen, xb, assign, 1)
    B = handle(capi, metric, cen, xb, assign, 0)
    model = Model(nlist, d, xb, assign)
    A.search(xq, K, NPROBE)
    assert A.scan_arith() == 2
    v = (cen[5] + 0.5).astype(np.float32)[None]
    for h in (A, B):
        h.add(v, np.array([99999]), np.array([5]))
    model.add(v, [99999], [5])
    check_step(A, B, model, xq, "non-integer add")
    A.search(xq, K, NPROBE)
    B.search(xq, K, NPROBE)
    assert A.scan_arith() == B.scan_arith() != 2
    assert A.layout_digest()[3] == 0
    oracle_check(oracle, A, metric, cen, model, xq)
    for h in (A, B):
        assert h.remove_ids(np.array([99999])) == 1
    model.remove_ids([99999])
    check_step(A, B, model, xq, "its removal")
    A.search(xq, K, NPROBE)
    assert A.scan_arith() == 2 and A.layout_digest()[3] != 0
    oracle_check(oracle, A, metric, cen, model, xq)
    for h in (A, B):
        h.close()
    # the same by magnitude at d = 960 (960 * 132^2 <= 2^24 < 960 * 133^2): a row holding 133 still has byte codes, but no search may
    # use them; without it they are used again.  After each step: scan_arith, the layout and the results of a full upload.
    metric, cen, assign, xb, xq = make_case("bytes_960")
    nlist, d = cen.shape
    A = handle(capi, metric, cen, xb, assign, 1)
    B = handle(capi, metric, cen, xb, assign, 0)
    model = Model(nlist, d, xb, assign)

    def fresh():
        fb, fa, fi = model.flat()
        h = capi.Handle(d, nlist, metric, 0)
        h.set_centroids(cen)
        h.set_lists_from_assign(fb, fa, fi)
        return h

    def same_as_full_upload(what, want):
        C = fresh()
        check_step(A, B, model, xq, what)
        warm(C, xq)
        assert A.layout_digest() == C.layout_digest(), what
        for h in (A, B, C):
            oracle_check(oracle, h, metric, cen, model, xq)
            assert h.scan_arith() == want, (what, h.scan_arith())
        C.close()

    A.search(xq, K, NPROBE)
    assert A.scan_arith() == 2
    v = xb[7:8].copy()
    v[0, d - 1] = 133.0
    for h in (A, B):
        h.add(v, np.array([99999]), np.array([5]))
    model.add(v, [99999], [5])
    same_as_full_upload("a row holding 133", 1)
    assert A.layout_digest()[3] != 0  # (byte codes are kept while every value fits the type; the search decides by magnitude)
    for h in (A, B):
        assert h.remove_ids(np.array([99999])) == 1
    model.remove_ids([99999])
    same_as_full_upload("its removal", 2)
    # ... and through update_lists: the value written over an entry, then overwritten again
    sizes = [len(i) for i in model.ids]
    w = np.array([(6 << 32) | 2], np.uint64)
    for h in (A, B):
        h.update_lists(sizes, w, np.array([88888]), v)
    model.update(sizes, w, [88888], v)
    same_as_full_upload("133 written over an entry", 1)
    for h in (A, B):
        h.update_lists(sizes, w, np.array([88889]), xb[9:10])
    model.update(sizes, w, [88889], xb[9:10])
    same_as_full_upload("overwritten again", 2)


def test_fp16_scale_change(capi, oracle):
    metric, cen, assign, xb, xq = make_case("l2_96")
    nlist, d = cen.shape
    A = handle(capi, metric, cen, xb, assign, 1)
    B = handle(capi, metric, cen, xb, assign, 0)
    model = Model(nlist, d, xb, assign)
    warm(A, xq)
    before = A.layout_digest()[4]
    v = (cen[3] * 9.0).astype(np.float32)[None]  # (a larger amax: another power-of-two scale)
    for h in (A, B):
        h.add(v, np.array([77777]), np.array([3]))
    model.add(v, [77777], [3])
    check_step(A, B, model, xq, "larger amax")
    assert A.layout_digest()[4] not in (0, before)
    oracle_check(oracle, A, metric, cen, model, xq)


def test_remove_ids_order(capi):
    metric, cen, assign, xb, xq = make_case("odd_30")
    nlist, d = cen.shape
    A = handle(capi, metric, cen, xb, assign, 1)
    model = Model(nlist, d, xb, assign)
    rs = np.random.RandomState(5)
    sel = rs.choice(len(xb), 400, replace=False).astype(np.int64)
    sel = np.concatenate([sel, [10 ** 9]])  # (an id that is not there)
    assert A.remove_ids(sel) == model.remove_ids(sel) == 400
    assert A.ntotal == len(xb) - 400
    for l in range(nlist):
        c, i = A.get_list(l)
        assert np.array_equal(i, model.ids[l]) and np.array_equal(bits(c), bits(model.codes[l]))
    assert A.last_update()[0] == 1


def test_tickets_out_refuse_and_large_journal_falls_back(capi, oracle):
    metric, cen, assign, xb, xq = make_case("l2_96")
    nlist, d = cen.shape
    A = handle(capi, metric, cen, xb, assign, 1)
    model = Model(nlist, d, xb, assign)
    eD, eI = oracle_check(oracle, A, metric, cen, model, xq)
    A.set_queries(xq)
    t = A.submit_search_resident(0, NQ, K, NPROBE)
    with pytest.raises(capi.EngineError) as e:
        A.remove_ids(np.array([0, 1, 2]))
    assert e.value.code == -2
    with pytest.raises(capi.EngineError):
        A.add(xb[:3], np.array([1, 2, 3]) + 10 ** 6, np.array([0, 0, 0]))
    D, I, _, _ = A.wait(t)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    assert A.ntotal == len(xb)
    # after the wait, the same change goes through
    assert A.remove_ids(np.array([0, 1, 2])) == model.remove_ids([0, 1, 2])
    assert A.last_update()[0] == 1
    # a journal that writes more than a quarter of the entries takes the full path
    rs = np.random.RandomState(2)
    lists = rs.randint(0, nlist, size=len(xb) // 2)
    x = new_rows(rs, "l2_96", cen, lists)
    ids = np.arange(10 ** 6, 10 ** 6 + len(lists), dtype=np.int64)
    A.add(x, ids, lists)
    model.add(x, ids, lists)
    oracle_check(oracle, A, metric, cen, model, xq)
    assert A.last_update()[0] == 2


def test_adaptive_and_tickets_after_updates(capi, oracle):
    """search_adaptive (D, I, my_nprobe) and submit_adaptive / wait tickets over an index changed in place equal the full-upload
    handle and the oracle; update_lists and remove_ids are refused while a ticket is out, and the ticket's results stay right"""
    metric, cen, assign, xb, xq = make_case("ragged", seed=8, nlist=32)  # (the tuner wants nlist > nlist / 8 + 20)
    nlist, d = cen.shape
    Kmax, qk = 20, 10
    rs = np.random.RandomState(21)
    A = handle(capi, metric, cen, xb, assign, 1)
    B = handle(capi, metric, cen, xb, assign, 0)
    model = Model(nlist, d, xb, assign)
    A.search(xq, K, NPROBE)
    B.search(xq, K, NPROBE)
    lists = rs.randint(0, nlist, size=120)
    x = new_rows(rs, "ragged", cen, lists)
    ids = np.arange(50000, 50000 + len(lists), dtype=np.int64)
    sel = np.concatenate([model.ids[2][:40], model.ids[7][-5:]])
    for h in (A, B):
        h.add(x, ids, lists)
        h.remove_ids(sel)
    model.add(x, ids, lists)
    model.remove_ids(sel)
    traces, ntr = [], 1
    while (1 << ntr) <= nlist // 8:
        ntr += 1
    for _ in range(ntr):
        n = int(rs.randint(5, 40))
        tx = np.sort(rs.rand(n) * 25.0).astype(np.float32) + np.arange(n, dtype=np.float32) * 1e-3
        traces.append((tx, (0.5 + rs.rand(n) * 2.5).astype(np.float32), (rs.rand(n) * 0.5).astype(np.float32)))
    arcos = capi.arcos_table()
    req = rs.choice([0.8, 0.9, 0.95], size=NQ).astype(np.float32)
    fb, fa, fi = model.flat()
    olists = oracle.Lists(metric, cen, fb, fa, fi)
    cd, ck = oracle.knn(metric, xq, cen, nlist)
    gtD, _ = oracle.knn(metric, xq, fb, Kmax)
    tun = oracle.Tuner(oracle.interdis(metric, cen), traces, Kmax, NQ, arcos=arcos)
    stt = tun.struct(qk, req, 2.0, 1.0, gt_D=gtD)
    eD, eI, _ = oracle.search_preassigned(olists, xq, Kmax, ck, cd, tuner=stt, offset=0, nthreads=1)
    for h in (A, B):
        h.set_interdis(None)
        h.set_tuner(Kmax, traces, arcos)
        h.set_queries(xq)
        my_np = np.zeros(NQ, dtype=np.uint64)
        t_rec = np.zeros(NQ, dtype=np.float32)
        D, I = h.search_adaptive(0, NQ, qk, 2.0, 1.0, req, my_np, t_rec, gt_D=gtD)
        assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
        assert np.array_equal(my_np.astype(np.int64), tun.my_nprobe.astype(np.int64))
    assert A.last_update()[0] == 1 and B.last_update()[0] == 2
    assert A.layout_digest()[:4] == B.layout_digest()[:4]
    # tickets of the asynchronous pool (its contexts were made before the next change: they must see its buffers)
    tickets = []
    for _ in range(2):
        my_np, t_rec = np.zeros(NQ, dtype=np.uint64), np.zeros(NQ, dtype=np.float32)
        tickets.append(A.submit_adaptive(0, NQ, qk, 2.0, 1.0, req, my_np, t_rec, gt_D=gtD))
    sizes = [len(i) for i in model.ids]
    with pytest.raises(capi.EngineError) as e:
        A.update_lists(sizes, np.array([(3 << 32) | 0], np.uint64), np.array([123456]), x[:1])
    assert e.value.code == -2
    with pytest.raises(capi.EngineError) as e:
        A.remove_ids(np.array([int(model.ids[3][0])]))
    assert e.value.code == -2
    for t in tickets:
        D, I, _, _ = A.wait(t)
        assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    # a further change after the wait, then tickets again on the same pool
    w = np.array([(3 << 32) | 0, (3 << 32) | 1], np.uint64)
    nx = new_rows(rs, "ragged", cen, np.array([3, 3]))
    nid = np.array([70001, 70002], np.int64)
    for h in (A, B):
        h.update_lists(sizes, w, nid, nx)
    model.update(sizes, w, nid, nx)
    assert A.last_update()[0] == 1
    fb, fa, fi = model.flat()
    olists = oracle.Lists(metric, cen, fb, fa, fi)
    gtD, _ = oracle.knn(metric, xq, fb, Kmax)
    tun = oracle.Tuner(oracle.interdis(metric, cen), traces, Kmax, NQ, arcos=arcos)
    stt = tun.struct(qk, req, 2.0, 1.0, gt_D=gtD)
    eD, eI, _ = oracle.search_preassigned(olists, xq, Kmax, ck, cd, tuner=stt, offset=0, nthreads=1)
    my_np, t_rec = np.zeros(NQ, dtype=np.uint64), np.zeros(NQ, dtype=np.float32)
    t = A.submit_adaptive(0, NQ, qk, 2.0, 1.0, req, my_np, t_rec, gt_D=gtD)
    D, I, _, _ = A.wait(t)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    assert np.array_equal(my_np.astype(np.int64), tun.my_nprobe.astype(np.int64))
    assert A.layout_digest()[:4] == B.layout_digest()[:4]
