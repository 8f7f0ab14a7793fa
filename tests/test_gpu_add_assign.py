"""amd_ivf_add without precomputed_idx: the engine ranks the vectors itself (a k = 1 coarse ranking on the device, in blocks of 2^18,
through the matrix-core pick path where its gate opens) and appends to the list that ranking names.  Every case of
add_assign_cases.py is held to the CPU oracle's assignment and to the numpy list model: host state, device layout, a search over
the result -- with the changes sent whole ("incremental" 0), as a first upload, and through the journal in HBM.  A refused add
(a list number that cannot be) must leave the index exactly as it was."""
import subprocess

import numpy as np
import pytest

import add_assign_cases as ac
import mirror_driver

pytestmark = pytest.mark.gpu

K = 10
# "rebuild": every list is sent again; "dirty": never searched before the adds, one first upload; "journal": an index four times as
# long as the adds, searched before every add, so that each add reaches the device through the journal (apply_journal)
VARIANTS = ("rebuild", "dirty", "journal")
CASES = ac.small_cases()
bits = ac.bits


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def new_handle(capi, case, incremental):
    nlist, d = case.cen.shape
    h = capi.Handle(d, nlist, case.metric, 0)
    h.set_option("incremental", incremental)
    h.set_centroids(case.cen)
    return h


def check_lists(h, model, what):
    """host state: ntotal, every list_size, every get_list (codes by bits, ids)"""
    assert h.ntotal == model.ntotal, (what, h.ntotal, model.ntotal)
    sizes = model.sizes()
    got = np.array([h.list_size(l) for l in range(model.nlist)])
    assert np.array_equal(got, sizes), (what, np.nonzero(got != sizes)[0][:10])
    for l in range(model.nlist):
        c, i = h.get_list(l)
        assert np.array_equal(i, model.ids(l)), (what, l)
        assert np.array_equal(bits(c), bits(model.codes(l))), (what, l)


def expected_search(oracle, case, model, xq):
    nprobe = min(len(case.cen), 64)
    xb, assign, ids = model.flat()
    lists = oracle.Lists(case.metric, case.cen, xb, assign, ids)
    cd, ck = oracle.knn(case.metric, xq, case.cen, nprobe)
    eD, eI, _ = oracle.search_preassigned(lists, xq, K, ck, cd)
    return cd, ck, eD, eI


def check_search_and_layout(capi, oracle, h, case, model, what):
    """search_preassigned over the result == the oracle over the model; the device layout == a fresh handle's that was given the
    model's lists whole.  Where vectors were skipped ntotal counts them and set_lists cannot know of them: the last digest (the
    flags, ntotal among them) is left out there -- every buffer of the layout is still compared."""
    xq = ac.finite_queries(case)
    cd, ck, eD, eI = expected_search(oracle, case, model, xq)
    D, I = h.search_preassigned(xq, K, ck, cd)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD)), what
    F = new_handle(capi, case, 1)
    F.set_lists(model.sizes(), [model.codes(l) for l in range(model.nlist)], [model.ids(l) for l in range(model.nlist)])
    D, I = F.search_preassigned(xq, K, ck, cd)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD)), what
    dh, df = h.layout_digest(), F.layout_digest()
    upto = 8 if model.ntotal == model.sizes().sum() else 7
    assert dh[:upto] == df[:upto], (what, [i for i in range(upto) if dh[i] != df[i]])
    F.close()
    return dh, df


def check_pick(h, case, n, first, what):
    """the path the ranking of the last add took"""
    p = h.last_coarse_pick()
    if not ac.takes_pick(n, len(case.cen)):
        assert p == 0, (what, p)
    elif case.picks:
        assert 0 < p <= n, (what, p)
        if first and case.tied is not None:
            assert n - p >= case.tied, (what, p)  # (a ranking that ties for the first place is never the picked path's)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_add_assigns_as_the_oracle(capi, oracle, name, variant):
    case = CASES[name]
    h = new_handle(capi, case, 0 if variant == "rebuild" else 1)
    model = ac.Model(*case.cen.shape)
    xq = ac.finite_queries(case)
    if variant == "journal":
        seed = ac.seed_rows(case)
        keys = ac.expected_keys(case.metric, seed, case.cen)
        h.add(seed, precomputed_idx=keys)
        model.add(seed, None, keys)
    for j, (x, xids) in enumerate(case.adds):
        if variant == "journal":
            h.search(xq, K, 4)  # (the lists are in HBM: the next add is journalled)
        h.add(x, xids)
        check_pick(h, case, len(x), j == 0, (name, variant, j))
        model.add(x, xids, ac.expected_keys(case.metric, x, case.cen))
        assert h.ntotal == model.ntotal
    check_lists(h, model, (name, variant))
    assert h.last_update()[0] == (1 if variant == "journal" else 2), h.last_update()
    dh, df = check_search_and_layout(capi, oracle, h, case, model, (name, variant))
    if name.startswith("nonfinite-bytes"):
        # the stored vectors are bytes: the skipped ones (a NaN, an infinity) must not cost the lists their byte codes
        assert df[3] != 0 and dh[3] == df[3], (name, variant, dh[3], df[3])
    h.close()


@pytest.mark.parametrize("metric", [1, 0])
def test_nonfinite_rankings_are_flagged_one_by_one(capi, metric):
    """"coarse_pick" 1: approximate distances from fp32 operands, which need no scale for the whole matrix -- the non-finite rankings
    are flagged each on its own by coarse_pick_kernel and go the exact way, the others stay with the picked path"""
    case = ac.nonfinite_case(metric, 300)
    (x, _), = case.adds
    h = new_handle(capi, case, 1)
    h.set_option("coarse_pick", 1)
    h.add(x)
    p = h.last_coarse_pick()
    assert 0 < p <= len(x) - int((~np.isfinite(x).all(axis=1)).sum()), p
    check_lists(h, ac.model_of(case), case.name)
    h.close()


@pytest.mark.parametrize("metric,nlist", ac.BLOCK_CASES)
def test_block_edge(capi, oracle, metric, nlist):
    """2^18 + 3 vectors in one call, as 2^18 and 3, and as 3 and 2^18: the oracle's lists each time, and one device layout"""
    case = ac.block_case(metric, nlist)
    x = case.adds[0][0]
    keys = ac.block_keys(metric, nlist)
    model = ac.Model(*case.cen.shape)
    model.add(x, None, keys)
    B = ac.ADD_BLOCK
    digests = []
    for split in ((B + 3,), (B, 3), (3, B)):
        h = new_handle(capi, case, 1)
        o = 0
        for m in split:
            h.add(x[o:o + m])
            o += m
            # (a call's last block decides: the three vectors behind a full block take the exact path)
            p = h.last_coarse_pick()
            assert (0 < p <= B) if (m == B and nlist == 68) else p == 0, (split, m, p)
        check_lists(h, model, (nlist, split))
        if len(split) == 1:
            check_search_and_layout(capi, oracle, h, case, model, (nlist, split))
        else:
            cd, ck, _, _ = expected_search(oracle, case, model, ac.finite_queries(case))
            h.search_preassigned(ac.finite_queries(case), K, ck, cd)
        digests.append(h.layout_digest())
        h.close()
    assert digests[0] == digests[1] == digests[2]


@pytest.mark.parametrize("metric", [1, 0])
def test_add_shares_a_handle_with_rankings_and_searches(capi, oracle, metric):
    """add(300), coarse(the same 300, nprobe 1 and 8), add(17), search(300 queries), add(300) on one handle -- the coarse work list is
    cached on the handle by its size and add ranks through it too; then the same vectors in two other orders on fresh handles"""
    case = ac.history_case(metric)
    xs = [x for x, _ in case.adds]
    ks = [ac.expected_keys(metric, x, case.cen) for x in xs]
    h = new_handle(capi, case, 1)
    model = ac.Model(*case.cen.shape)
    h.add(xs[0])
    check_pick(h, case, 300, True, "first add")
    model.add(xs[0], None, ks[0])
    for nprobe in (1, 8):
        D, I = h.coarse(xs[0], nprobe)
        oD, oI = oracle.knn(metric, xs[0], case.cen, nprobe)
        assert np.array_equal(I, oI) and np.array_equal(bits(D), bits(oD)), nprobe
    assert np.array_equal(oI[:, 0], ks[0])
    h.add(xs[1])
    check_pick(h, case, 17, False, "second add")
    model.add(xs[1], None, ks[1])
    xb, assign, ids = model.flat()
    cd, ck = oracle.knn(metric, xs[0], case.cen, 8)
    eD, eI, _ = oracle.search_preassigned(oracle.Lists(metric, case.cen, xb, assign, ids), xs[0], K, ck, cd)
    D, I = h.search(xs[0], K, 8)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    h.add(xs[2])
    check_pick(h, case, 300, False, "third add")
    model.add(xs[2], None, ks[2])
    check_lists(h, model, "one handle")
    check_search_and_layout(capi, oracle, h, case, model, "one handle")
    h.close()
    for order in ((1, 0, 2), (0, 2, 1)):  # sizes (17, 300, 300) and (300, 300, 17)
        g = new_handle(capi, case, 1)
        m2 = ac.Model(*case.cen.shape)
        for j in order:
            g.add(xs[j])
            m2.add(xs[j], None, ks[j])
        check_lists(g, m2, order)
        g.close()


def snapshot(capi, h, sel, xq):
    return dict(ntotal=h.ntotal, sizes=[h.list_size(l) for l in range(h.nlist)], lists=[h.get_list(l) for l in range(h.nlist)],
                digest=h.layout_digest(), dmap=h.direct_map_info(), search=h.search(xq, K, 8), selected=h.search_selected(sel, xq, K, 8))


def same_snapshot(a, b):
    assert a["ntotal"] == b["ntotal"] and a["sizes"] == b["sizes"]
    for (c0, i0), (c1, i1) in zip(a["lists"], b["lists"]):
        assert np.array_equal(i0, i1) and np.array_equal(bits(c0), bits(c1))
    assert a["digest"] == b["digest"] and a["dmap"] == b["dmap"]
    for key in ("search", "selected"):
        assert np.array_equal(a[key][1], b[key][1]) and np.array_equal(bits(a[key][0]), bits(b[key][0])), key


@pytest.mark.parametrize("incremental", [1, 0])
@pytest.mark.parametrize("pos", [3, 0])
@pytest.mark.parametrize("bad", ["nlist", "nlist + 10**12"])
def test_refused_add_leaves_the_index_whole(capi, oracle, bad, pos, incremental):
    """a precomputed list number that cannot be: -2 with the reference's message, and nothing of the index has moved -- not its lists,
    not the device layout, not the direct map, not the selectors made before the call -- whatever stood before the bad number"""
    case = ac.history_case(1)
    xs = [x for x, _ in case.adds]
    nlist = len(case.cen)
    h = new_handle(capi, case, incremental)
    model = ac.Model(*case.cen.shape)
    h.add(xs[0])
    model.add(xs[0], None, ac.expected_keys(1, xs[0], case.cen))
    xq = xs[0][:64]
    h.search(xq, K, 8)
    h.make_direct_map(True)
    sel = h.selector(capi.SUBSET_ID_RANGE, 50, 250)
    before = snapshot(capi, h, sel, xq)
    assert before["dmap"][:3] == [1, 300, 0]
    idx = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], dtype=np.int64)
    idx[pos + 1:] = idx[pos:-1]
    idx[pos] = nlist if bad == "nlist" else nlist + 10 ** 12
    assert pos != 3 or list(idx[:5]) == [0, 1, 2, idx[3], 3]
    with pytest.raises(capi.EngineError) as e:
        h.add(xs[1][:10], precomputed_idx=idx)
    assert e.value.code == -2 and "Invalid list number in add" in str(e.value)
    same_snapshot(before, snapshot(capi, h, sel, xq))
    assert np.array_equal(bits(h.reconstruct([0, 299])), bits(xs[0][[0, 299]]))
    assert h.direct_map_info() == before["dmap"]  # (no pass made again: the lists' generation has not moved)
    # the same call with list numbers that can be, then an add that ranks: the model's lists
    good = np.where(idx >= nlist, -1, idx)
    h.add(xs[1][:10], precomputed_idx=good)
    model.add(xs[1][:10], None, good)
    h.add(xs[2])
    model.add(xs[2], None, ac.expected_keys(1, xs[2], case.cen))
    check_lists(h, model, "after the refusal")
    check_search_and_layout(capi, oracle, h, case, model, "after the refusal")
    with pytest.raises(capi.EngineError):  # (an add that went through does make the old selector stale)
        h.search_selected(sel, xq, K, 8)
    sel.close()
    h.close()


# ---- the C++ mirror: IndexIVFFlat::add of the class mirror ranks through the same engine call
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return mirror_driver.host_mirror_driver(tmp_path_factory)


@pytest.mark.parametrize("metric,count,where", [(1, 9, "first"), (0, 7, "last")])
def test_mirror_add_assigns_as_the_oracle(driver, oracle, tmp_path, metric, count, where):
    """the driver's "fixed" flow adds nb / 3 vectors (the tie case: 300, the picked path), then the rest, compares every list's size
    and content (ids and codes, list by list) and searches the lists it built; every expected tensor is the oracle's over the
    model's lists.  The flow also sends a list number that cannot be through add_core and wants the index unchanged."""
    from oracle import tbundle
    case = ac.tie_case(metric, count, where)
    x = case.adds[0][0]
    xb = np.concatenate([x, x + np.float32(0.25), x[::-1] - np.float32(0.25)])
    keys = ac.expected_keys(metric, xb, case.cen)
    nprobe, xq = 8, np.ascontiguousarray(x[::10] + np.float32(0.125))
    lists = oracle.Lists(metric, case.cen, xb, keys)
    model = ac.Model(*case.cen.shape)
    model.add(xb[:300], None, keys[:300])  # (the driver's two calls)
    model.add(xb[300:], None, keys[300:])
    _, _, list_ids = model.flat()
    assert np.array_equal(list_ids, lists.ids) and np.array_equal(bits(model.flat()[0]), bits(lists.codes))
    cd, ck = oracle.knn(metric, xq, case.cen, nprobe)
    D, I, st = oracle.search_preassigned(lists, xq, K, ck, cd)
    _, Ip, _ = oracle.search_preassigned(lists, xq, K, ck, cd, store_pairs=True)
    t = {"d": x.shape[1], "nlist": len(case.cen), "nprobe": nprobe, "metric": metric, "centroids": case.cen, "xb": xb, "xq": xq,
         "ks": np.array([K], np.int64), "list_sizes": np.bincount(keys, minlength=len(case.cen)).astype(np.int64), f"I_k{K}": I, f"D_k{K}": D,
         f"stats_k{K}": st, f"I_k{K}_pairs": Ip, "list_ids": lists.ids, "list_codes": lists.codes}
    f = str(tmp_path / "in.tb")
    tbundle.save(f, t)
    r = subprocess.run([driver, "fixed", f], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
