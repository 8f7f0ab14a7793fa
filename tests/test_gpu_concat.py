"""Device-resident indexes joined on the device (amd_ivf_concat, ivf_concat.hip): list l of the result is, over the parts in order, a
run of each part's list l.  The expected lists are made here with numpy slicing and concatenation; the device layout is compared with
a handle that takes those lists through amd_ivf_set_lists (all eight digest words after the same warm-up), every list is read back,
and every search is compared with the pinned CPU oracle over them.  Every comparison is of bits or of integers."""
import numpy as np
import pytest

from test_gpu_subset import check_searches, from_lists, id_bits, make_traces
from test_gpu_update import BYTE_CASES, K, NPROBE, NQ, Model, bits, make_case, new_rows, warm

pytestmark = pytest.mark.gpu

CASES = ["sift_l2", "l2_96", "ip_96", "odd_30", "ragged", "bytes_200", "bytes_960"]
KINDS = ["own", "cuts"]  # parts as handles of their own (amd_ivf_set_lists), or as amd_ivf_subset cuts of one parent: no host rows


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def model_of(d, codes, ids):
    m = Model.__new__(Model)
    m.d, m.codes, m.ids = d, codes, ids
    return m


def split(model, part_of, nparts):
    """the rows whose id i has part_of[i] == j, list by list in the model's order, for every j"""
    return [model_of(model.d, [c[part_of[i] == j].copy() for c, i in zip(model.codes, model.ids)],
                     [i[part_of[i] == j].copy() for i in model.ids]) for j in range(nparts)]


def joined_model(parts):
    """what the join holds: parts = [(model, begin or None, end or None, id_add)]"""
    m0 = parts[0][0]
    codes, ids = [], []
    for l in range(len(m0.ids)):
        cs, js = [], []
        for m, b, e, add in parts:
            lo = 0 if b is None else int(b[l])
            hi = len(m.ids[l]) if e is None else int(e[l])
            cs.append(m.codes[l][lo:hi])
            js.append(m.ids[l][lo:hi] + np.int64(add))
        codes.append(np.concatenate(cs).reshape(-1, m0.d).astype(np.float32))
        ids.append(np.concatenate(js).astype(np.int64))
    return model_of(m0.d, codes, ids)


def make_parts(capi, kind, metric, cen, models):
    """a handle per model: from its lists, or cut from one parent that holds them all (the parent is closed: a cut borrows nothing)"""
    if kind == "own":
        return [from_lists(capi, metric, cen, m) for m in models]
    parent = from_lists(capi, metric, cen, joined_model([(m, None, None, 0) for m in models]))
    top = max(int(i.max()) for m in models for i in m.ids if len(i)) + 1
    cuts = [parent.subset(capi.SUBSET_ID_BITS, 0, 0, id_bits(np.concatenate(m.ids), (top >> 6) + 2)) for m in models]
    parent.close()
    return cuts


def check_joined(capi, oracle, joined, metric, cen, want, xq, nparts, searches=True):
    """transfer report, layout (all eight digest words after the same warm-up), sizes, lists and searches of a joined index"""
    nlist = joined.nlist
    taken, parts, h2d, d2h = joined.last_concat()
    total = sum(len(i) for i in want.ids)
    assert taken == total == joined.ntotal and parts == nparts, joined.last_concat()
    assert h2d <= (2 * nparts + 2) * 8 * (nlist + 1) + 65536, joined.last_concat()
    assert d2h <= 65536, joined.last_concat()
    ref = from_lists(capi, metric, cen, want)
    warm(joined, xq)
    warm(ref, xq)
    dj, dr = joined.layout_digest(), ref.layout_digest()
    assert dj == dr, [i for i in range(8) if dj[i] != dr[i]]
    for l in range(nlist):
        assert joined.list_size(l) == len(want.ids[l]), l
        c, i = joined.get_list(l)
        assert np.array_equal(i, want.ids[l]), l
        assert np.array_equal(bits(c), bits(want.codes[l])), l
    ref.close()
    if searches:
        check_searches(oracle, joined, metric, cen, want, xq)
    return dj


def copies_built(name, dg, ntotal):
    if ntotal:
        if name in BYTE_CASES:
            assert dg[3], "no byte fragments"
        else:
            assert dg[4] and dg[5] and dg[6], "the warm-up did not build every fp32 copy"


def case(name):
    metric, cen, assign, xb, xq = make_case(name)
    return metric, cen, xb, xq, Model(cen.shape[0], cen.shape[1], xb, assign)


# ------------------------------------------------------------------------------------------------ 1. merge
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", CASES)
def test_merge_of_whole_parts(capi, oracle, name, kind):
    metric, cen, xb, xq, model = case(name)
    rs = np.random.RandomState(5)
    two = split(model, rs.randint(0, 2, size=len(xb)), 2)
    three = split(model, rs.randint(0, 3, size=len(xb)), 3)
    h2, h3 = make_parts(capi, kind, metric, cen, two), make_parts(capi, kind, metric, cen, three)
    # two parts, ids as they are (a bare handle is a whole part)
    j = capi.Handle.concat(h2)
    dg = check_joined(capi, oracle, j, metric, cen, joined_model([(m, None, None, 0) for m in two]), xq, 2)
    copies_built(name, dg, j.ntotal)
    if name in BYTE_CASES:
        assert j.scan_arith() == 2
    j.close()
    # three parts, shifted ids: merge_from's add_id, one of them negative
    adds = [0, 100000, -(1 << 40)]
    j = capi.Handle.concat([(h, None, None, a) for h, a in zip(h3, adds)])
    check_joined(capi, oracle, j, metric, cen, joined_model([(m, None, None, a) for m, a in zip(three, adds)]), xq, 3)
    j.close()
    # the same handle twice, between two others
    order, adds = [0, 1, 0, 2], [0, 7, 50000, 0]
    j = capi.Handle.concat([(h3[p], None, None, a) for p, a in zip(order, adds)])
    check_joined(capi, oracle, j, metric, cen, joined_model([(three[p], None, None, a) for p, a in zip(order, adds)]), xq, 4)
    j.close()
    for h in h2 + h3:
        h.close()


# ------------------------------------------------------------------------------------------------ 2. runs at the layout's edges
EDGE_LEN = [0, 1, 31, 32, 33, 63, 64, 65]
EDGE_BEGIN = [0, 3, 3, 33, 1, 2, 5, 3]  # (not multiples of 4 or of 32)


def edge_runs(models):
    """three parts (the third is the first one's handle again).  Lists 0..7: part 0 gives EDGE_LEN[l] entries from EDGE_BEGIN[l], part 1
    the same lengths in reverse from entry 5; list 8 is empty in every part, list 9 comes from the last part alone, the other lists are
    whole, all but their ends, and the last two entries.  Runs are clamped to the list (ragged has empty lists)."""
    nlist = len(models[0].ids)
    size = [np.array([len(i) for i in m.ids], np.int64) for m in models]
    b0, b1, b2 = np.zeros(nlist, np.int64), np.ones(nlist, np.int64), np.maximum(size[0] - 2, 0)
    e0, e1, e2 = size[0].copy(), np.maximum(size[1] - 1, 1), size[0].copy()
    for l in range(8):
        b0[l], e0[l] = EDGE_BEGIN[l], EDGE_BEGIN[l] + EDGE_LEN[l]
        b1[l], e1[l] = 5, 5 + EDGE_LEN[7 - l]
    b0[8], e0[8], b1[8], e1[8], b2[8], e2[8] = 7, 7, 10, 10, 0, 0
    b0[9], e0[9], b1[9], e1[9] = 4, 4, 0, 0
    runs = []
    for b, e, s in ((b0, e0, size[0]), (b1, e1, size[1]), (b2, e2, size[0])):
        b = np.minimum(b, s)
        runs.append((b.astype(np.uint64), np.maximum(np.minimum(e, s), b).astype(np.uint64)))
    return runs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", CASES)
def test_runs_at_the_layouts_edges(capi, oracle, name, kind):
    metric, cen, xb, xq, model = case(name)
    nlist = cen.shape[0]
    two = split(model, np.arange(len(xb)) % 2, 2)
    hs = make_parts(capi, kind, metric, cen, two)
    runs = edge_runs(two)
    if name != "ragged":  # every list is long enough: the lengths are the intended ones
        assert [int(e - b) for b, e in zip(*runs[0])][:8] == EDGE_LEN
        assert [int(e - b) for b, e in zip(*runs[1])][:8] == EDGE_LEN[::-1]
    order, adds = [0, 1, 0], [0, 0, 1 << 33]
    j = capi.Handle.concat([(hs[p], b, e, a) for p, (b, e), a in zip(order, runs, adds)])
    want = joined_model([(two[p], b, e, a) for p, (b, e), a in zip(order, runs, adds)])
    assert len(want.ids[8]) == 0 and len(want.ids[9]) == min(2, len(two[0].ids[9]))
    dg = check_joined(capi, oracle, j, metric, cen, want, xq, 3)
    copies_built(name, dg, j.ntotal)
    j.close()
    # begin == end everywhere: a valid index of ntotal 0, whose searches return the reference's empty result
    same = (np.arange(nlist) % 5).astype(np.uint64)
    same = np.minimum(same, np.array([len(i) for i in two[1].ids], np.uint64))
    j = capi.Handle.concat([(hs[0], None, np.zeros(nlist, np.uint64), 0), (hs[1], same, same, 3)])
    empty = joined_model([(two[0], None, np.zeros(nlist, np.int64), 0), (two[1], same, same, 3)])
    assert j.ntotal == 0
    check_joined(capi, oracle, j, metric, cen, empty, xq, 2)
    D, I = j.search(xq, K, NPROBE)
    assert (I == -1).all()
    j.close()
    for h in hs:
        h.close()


# ------------------------------------------------------------------------------------------------ 3. split and rejoin
@pytest.mark.parametrize("name", CASES)
def test_split_by_subset_and_rejoin(capi, oracle, name):
    metric, cen, xb, xq, model = case(name)
    nb = len(xb)
    perm = np.random.RandomState(12).permutation(nb).astype(np.int64)
    model.ids = [perm[i] for i in model.ids]  # (ids in no order inside a list: grouping them by range moves entries)
    parent = from_lists(capi, metric, cen, model)
    # ID_RANGE thirds: every list comes back grouped by third
    edges = [0, nb // 3, 2 * nb // 3, nb]
    cuts = [parent.subset(capi.SUBSET_ID_RANGE, edges[t], edges[t + 1]) for t in range(3)]
    j = capi.Handle.concat(cuts)
    third = np.searchsorted(np.array(edges[1:]), np.arange(nb), side="right")
    want = joined_model([(m, None, None, 0) for m in split(model, third, 3)])
    assert any(not np.array_equal(a, b) for a, b in zip(want.ids, model.ids)), "the grouping changed no list"
    check_joined(capi, oracle, j, metric, cen, want, xq, 3)
    j.close()
    for c in cuts:
        c.close()
    # SLICE thirds: the rejoined lists are the parent's own
    cuts = [parent.subset(capi.SUBSET_SLICE, edges[t], edges[t + 1]) for t in range(3)]
    assert sum(c.ntotal for c in cuts) == nb
    j = capi.Handle.concat(cuts)
    dg = check_joined(capi, oracle, j, metric, cen, model, xq, 3)
    warm(parent, xq)
    assert dg == parent.layout_digest()
    for h in cuts + [j, parent]:
        h.close()


# ------------------------------------------------------------------------------------------------ 4. a sliding window
class Window:
    """SlidingIndexWindow::step (IVFlib.cpp:190-243) restated: `sizes` is the reference's table, [list][slice] the list's entries up to
    and including that slice; the entries move by amd_ivf_concat instead of memmove"""

    def __init__(self, capi, slices):
        self.capi = capi
        self.index = capi.Handle.concat(slices)
        self.sizes = np.cumsum([[s.list_size(l) for s in slices] for l in range(slices[0].nlist)], axis=1).astype(np.int64)
        self.n_slice = len(slices)

    def step(self, sub, remove_oldest):
        assert not remove_oldest or self.n_slice > 0, "cannot remove slice: there is none"
        assert sub is not None or remove_oldest, "nothing to do???"
        amount = self.sizes[:, 0].copy() if remove_oldest else None
        parts = [(self.index, None if amount is None else amount.astype(np.uint64), None, 0)] + ([sub] if sub is not None else [])
        new = self.capi.Handle.concat(parts)
        now = np.array([new.list_size(l) for l in range(new.nlist)], np.int64)
        if remove_oldest and sub is not None:
            self.sizes[:, :-1] = self.sizes[:, 1:] - amount[:, None]
            self.sizes[:, -1] = now
        elif sub is not None:
            self.sizes = np.hstack([self.sizes, now[:, None]])
            self.n_slice += 1
        else:
            self.sizes = self.sizes[:, 1:] - amount[:, None]
            self.n_slice -= 1
        old, self.index = self.index, new
        old.close()  # (the previous window goes once the new one exists; the new one borrows nothing from it)
        return len(parts)


@pytest.mark.parametrize("name,kind", [(n, "own") for n in CASES] + [("sift_l2", "cuts"), ("ip_96", "cuts")])
def test_sliding_window(capi, oracle, name, kind):
    metric, cen, xb, xq, model = case(name)
    slices = split(model, np.random.RandomState(2).randint(0, 8, size=len(xb)), 8)
    hs = make_parts(capi, kind, metric, cen, slices)
    win = Window(capi, hs[:4])
    held = [0, 1, 2, 3]
    check_joined(capi, oracle, win.index, metric, cen, joined_model([(slices[t], None, None, 0) for t in held]), xq, 4, searches=False)
    # (slice to add or None, remove the oldest): the three branches of step, each twice
    for add, rm in ((4, True), (5, True), (None, True), (6, False), (7, True), (None, True)):
        nparts = win.step(hs[add] if add is not None else None, rm)
        held = held[1 if rm else 0:] + ([add] if add is not None else [])
        want = joined_model([(slices[t], None, None, 0) for t in held])
        assert win.n_slice == len(held) and win.sizes.shape[1] == len(held)
        assert np.array_equal(win.sizes, np.cumsum([[len(slices[t].ids[l]) for t in held] for l in range(cen.shape[0])], axis=1))
        dg = check_joined(capi, oracle, win.index, metric, cen, want, xq, nparts)
        copies_built(name, dg, win.index.ntotal)
    for h in hs + [win.index]:
        h.close()


# ------------------------------------------------------------------------------------------------ 5. byte eligibility
def byte_coded(h, xq):
    h.search(xq, K, NPROBE)
    return h.scan_arith() == 2 and h.layout_digest()[3] != 0


def test_byte_eligibility_follows_the_values_taken(capi, oracle):
    metric, cen, xb, xq, model = case("sift_l2")
    part_of = np.arange(len(xb)) % 6
    odd = 6 * 100  # (a row of slice 0)
    slices = split(model, part_of, 6)
    l_odd = [l for l in range(len(model.ids)) if odd in slices[0].ids[l]][0]
    p_odd = int(np.nonzero(slices[0].ids[l_odd] == odd)[0][0])
    slices[0].codes[l_odd][p_odd, 3] += 0.5  # the only row with a 0.5
    hs = make_parts(capi, "own", metric, cen, slices)
    assert not byte_coded(hs[0], xq) and all(byte_coded(h, xq) for h in hs[1:])
    win = Window(capi, hs[:4])
    assert not byte_coded(win.index, xq) and win.index.scan_arith() in (0, 1)
    check_joined(capi, oracle, win.index, metric, cen, joined_model([(slices[t], None, None, 0) for t in (0, 1, 2, 3)]), xq, 4)
    # the step that drops slice 0: byte-coded, as amd_ivf_set_lists of those lists
    win.step(hs[4], True)
    want = joined_model([(slices[t], None, None, 0) for t in (1, 2, 3, 4)])
    dg = check_joined(capi, oracle, win.index, metric, cen, want, xq, 2)
    assert dg[3] != 0 and byte_coded(win.index, xq)
    # ... and the reverse: a byte-coded window that takes the slice with that row stops being byte-coded
    win.step(hs[0], True)
    want = joined_model([(slices[t], None, None, 0) for t in (2, 3, 4, 0)])
    dg = check_joined(capi, oracle, win.index, metric, cen, want, xq, 2)
    assert dg[3] == 0 and not byte_coded(win.index, xq) and win.index.scan_arith() in (0, 1)
    win.index.close()
    # a run that cuts the row out of the middle part flips it as well
    nlist = cen.shape[0]
    begin = np.zeros(nlist, np.uint64)
    begin[l_odd] = p_odd + 1
    for b, coded in ((None, False), (begin, True)):
        j = capi.Handle.concat([hs[1], (hs[0], b, None, 0), hs[2]])
        want = joined_model([(slices[1], None, None, 0), (slices[0], b, None, 0), (slices[2], None, None, 0)])
        dg = check_joined(capi, oracle, j, metric, cen, want, xq, 3)
        assert (dg[3] != 0) == coded and byte_coded(j, xq) == coded
        j.close()
    end = np.array([len(i) for i in slices[0].ids], np.uint64)
    end[l_odd] = p_odd
    j = capi.Handle.concat([hs[1], (hs[0], None, end, 0), hs[2]])
    assert byte_coded(j, xq)
    j.close()
    for h in hs:
        h.close()


# ------------------------------------------------------------------------------------------------ 6. everything a subset can do
def test_a_joined_index_does_what_a_subset_does(capi, oracle):
    metric, cen, assign, xb, xq = make_case("ragged", seed=8, nlist=32)  # (the tuner wants nlist > nlist / 8 + 20)
    nlist, d = cen.shape
    model = Model(nlist, d, xb, assign)
    Kmax, qk = 20, 10
    rs = np.random.RandomState(21)
    traces, arcos = make_traces(rs, nlist), capi.arcos_table()
    req = rs.choice([0.8, 0.9, 0.95], size=NQ).astype(np.float32)
    nb = len(xb)
    three = split(model, np.arange(nb) * 3 // nb, 3)  # (thirds by id: the ids of the join are 0 .. nb - 1)
    hs = make_parts(capi, "own", metric, cen, three)
    hs[0].set_interdis(None)  # part 0's Auncel state is inherited
    hs[0].set_tuner(Kmax, traces, arcos)
    j = capi.Handle.concat(hs)
    want = joined_model([(m, None, None, 0) for m in three])
    twin = from_lists(capi, metric, cen, want)
    twin.set_interdis(None)
    twin.set_tuner(Kmax, traces, arcos)
    eD, eI = check_searches(oracle, j, metric, cen, want, xq)
    # a clone, a ticket
    c = j.clone()
    D, I = c.search(xq, K, NPROBE)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    c.close()
    j.set_queries(xq)
    twin.set_queries(xq)
    D, I, _, _ = j.wait(j.submit_search_resident(0, NQ, K, NPROBE))
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    # the adaptive search with the inherited tuner and interdis, against the twin given the same state
    gtD, _ = twin.search_exact(xq, Kmax)
    got = []
    for h in (j, twin):
        my_np, t_rec = np.zeros(NQ, np.uint64), np.zeros(NQ, np.float32)
        D, I = h.search_adaptive(0, NQ, qk, 2.0, 1.0, req, my_np, t_rec, gt_D=gtD)
        got.append((D, I, my_np, t_rec))
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(bits(got[0][0]), bits(got[1][0]))
    assert np.array_equal(got[0][2], got[1][2]) and np.array_equal(bits(got[0][3]), bits(got[1][3]))
    assert got[0][2].max() > 0 and (got[0][1] >= 0).any()
    # a selector search, the exact search
    with j.selector(capi.SUBSET_ID_MOD, 3, 1) as sj, twin.selector(capi.SUBSET_ID_MOD, 3, 1) as st:
        D, I = j.search_selected(sj, xq, K, NPROBE)
        tD, tI = twin.search_selected(st, xq, K, NPROBE)
        assert np.array_equal(I, tI) and np.array_equal(bits(D), bits(tD)) and (np.fmod(I[I >= 0], 3) == 1).all()
    D, I = j.search_exact(xq, K)
    tD, tI = twin.search_exact(xq, K)
    assert np.array_equal(I, tI) and np.array_equal(bits(D), bits(tD))
    # stored vectors back: the ids are 0 .. nb - 1
    j.make_direct_map(True)
    rec, found = j.reconstruct_n(0, nb)
    assert found.all() and np.array_equal(bits(rec), bits(xb))
    # a subset of it, a join of it with another part
    sub, tsub = j.subset(capi.SUBSET_ID_MOD, 2, 0), twin.subset(capi.SUBSET_ID_MOD, 2, 0)
    assert sub.ntotal == tsub.ntotal == (nb + 1) // 2
    warm(sub, xq)
    warm(tsub, xq)
    assert sub.layout_digest() == tsub.layout_digest()
    jj = capi.Handle.concat([j, (hs[1], None, None, 5000), sub])
    both = joined_model([(want, None, None, 0), (three[1], None, None, 5000),
                         (model_of(d, [c[i % 2 == 0] for c, i in zip(want.codes, want.ids)], [i[i % 2 == 0] for i in want.ids]), None, None, 0)])
    check_joined(capi, oracle, jj, metric, cen, both, xq, 3)
    # the mutators
    L = capi.lib()

    def refused(f, word):
        with pytest.raises(capi.EngineError) as e:
            f()
        assert e.value.code == -2 and word in L.amd_ivf_last_error().decode(), e.value

    sizes = [j.list_size(l) for l in range(nlist)]
    refused(lambda: j.add(xb[:2], np.array([7, 8]), np.array([0, 1])), "read-only")
    refused(lambda: j.set_lists_from_assign(xb, assign), "read-only")
    refused(lambda: j.update_lists(sizes, np.array([(3 << 32) | 0], np.uint64), np.array([5]), xb[:1]), "read-only")
    refused(lambda: j.remove_ids(np.array([0, 2, 4])), "read-only")
    refused(lambda: j.set_centroids(cen), "read-only")
    assert j.ntotal == nb
    for h in [sub, tsub, jj, j, twin] + hs:
        h.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(capi, oracle):
    metric, cen, xb, xq, model = case("l2_96")
    nlist, d = cen.shape
    two = split(model, np.arange(len(xb)) % 2, 2)
    a, b = make_parts(capi, "own", metric, cen, two)
    L = capi.lib()

    def refused(parts, word):
        with pytest.raises(capi.EngineError) as e:
            capi.Handle.concat(parts)
        assert e.value.code == -2, e.value
        assert word in L.amd_ivf_last_error().decode(), (word, L.amd_ivf_last_error().decode())

    refused([], "null")
    refused([a] * 65, "1 .. 64")
    refused([a, (None,)], "part 1 is null")
    c = b.clone()
    refused([a, c], "amd_ivf_clone")
    c.close()
    # parts of another shape (another device needs a second GPU: not reached here)
    for other_name, kw in (("odd_30", {}), ("l2_96", {"nlist": 8}), ("ip_96", {})):
        m2, cen2, as2, xb2, _ = make_case(other_name, **kw)
        o = from_lists(capi, m2, cen2, Model(cen2.shape[0], cen2.shape[1], xb2, as2))
        refused([a, o], "differs from part 0")
        o.close()
    # centroids: missing in a later part, or of other bits
    bare = capi.Handle(d, nlist, metric, 0)
    bare.set_lists([len(i) for i in two[1].ids], two[1].codes, two[1].ids)
    refused([a, bare], "no centroids")
    bare.close()
    cen2 = cen.copy()
    cen2.view(np.uint32)[nlist - 1, d - 1] ^= 1
    o = from_lists(capi, metric, cen2, two[1])
    refused([a, o], "centroids are not those of part 0")
    o.close()
    # runs outside their list
    size = np.array([len(i) for i in two[1].ids], np.uint64)
    bad = size.copy()
    bad[3] += 1
    refused([a, (b, None, bad, 0)], "list 3")
    begin = np.zeros(nlist, np.uint64)
    begin[5] = 9
    end = size.copy()
    end[5] = 8
    refused([a, (b, begin, end, 0)], "list 5")
    # tickets out on a part (whose later wait still returns the right result)
    b.set_queries(xq)
    t = b.submit_search_resident(0, NQ, K, NPROBE)
    refused([a, b], "tickets")
    D, I, _, _ = b.wait(t)
    D1, I1 = b.search(xq, K, NPROBE)
    assert np.array_equal(I, I1) and np.array_equal(bits(D), bits(D1))
    # a joined list of 2^32 entries: one list of 2^26 rows, 64 times -- refused from the sizes alone
    big = capi.Handle(1, 1, metric, 0)
    big.set_byte_codes(0)
    n = 1 << 26
    big.set_lists([n], [np.zeros((n, 1), np.float32)], [np.arange(n, dtype=np.int64)])
    refused([big] * 64, "2^32")
    big.close()
    # nothing was changed: the parts still search and still join
    for h, m in ((a, two[0]), (b, two[1])):
        check_searches(oracle, h, metric, cen, m, xq)
    j = capi.Handle.concat([a, b])
    taken, nparts, h2d, d2h = j.last_concat()
    assert (taken, nparts) == (len(xb), 2) and h2d <= (2 * 2 + 2) * 8 * (nlist + 1) + 65536 and d2h <= 65536
    check_joined(capi, oracle, j, metric, cen, joined_model([(m, None, None, 0) for m in two]), xq, 2)
    for h in (j, a, b):
        h.close()


# ------------------------------------------------------------------------------------------------ 8. pending work of a part
@pytest.mark.parametrize("name", ["sift_l2", "ip_96"])
def test_a_pending_add_of_a_part_is_in_the_join(capi, oracle, name):
    metric, cen, xb, xq, model = case(name)
    nlist = cen.shape[0]
    rs = np.random.RandomState(4)
    two = split(model, np.arange(len(xb)) % 2, 2)
    a, b = make_parts(capi, "own", metric, cen, two)
    for h in (a, b):
        warm(h, xq)  # (the adds below are journal entries of a layout that exists)
    for h, m, first in ((a, two[0], 10000), (b, two[1], 20000)):
        lists = rs.randint(0, nlist, size=70)
        x = new_rows(rs, name, cen, lists)
        ids = np.arange(first, first + len(lists), dtype=np.int64)
        h.add(x, ids, lists)  # not searched before the join
        m.add(x, ids, lists)
    j = capi.Handle.concat([a, b])
    want = joined_model([(m, None, None, 0) for m in two])
    assert j.ntotal == len(xb) + 140
    check_joined(capi, oracle, j, metric, cen, want, xq, 2)
    # no part was changed by the join
    for h, m in ((a, two[0]), (b, two[1])):
        check_searches(oracle, h, metric, cen, m, xq)
    for h in (j, a, b):
        h.close()
