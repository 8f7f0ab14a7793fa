"""Exact k-NN over the whole index (amd_ivf_search_exact, ivf_exact.hip): (D, I) are, bit for bit, the pinned CPU
oracle's search_preassigned over every list in list-number order -- and what amd_ivf_search_preassigned returns for those keys on the
same handle -- at every K-step count of the list pass, both metrics, ragged lists (lengths 0, 1, 31, 32, 33, 63, 64, 65, 70), batches
around the 256-query tile and k up to 100; the count of queries that leave the list pass because equal distances met is exactly the
number numpy finds from exact integer distances; calls that do not qualify for the byte pass go the general way whole."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_update import Model, make_case

pytestmark = pytest.mark.gpu

L2, IP = 1, 0
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "exact_child.py")
# list -> length, on the `ragged` case (whose lists 1, 5 and 6 are empty); 70 entries are three blocks, padded to four
SPECIAL = {2: 1, 3: 31, 7: 32, 8: 33, 9: 63, 10: 64, 11: 65, 12: 70}
NB = 20000
# (n, k): one query, a few, one tile's edge on either side of a query block and of the tile, two tiles; every k form
BATCHES = [(1, 100), (3, 65), (64, 10), (65, 64), (257, 1), (300, 10)]


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ragged_assign(nlist, nb=NB):
    """the list numbers of the `ragged` case, repeated to nb entries, with the lists of SPECIAL cut to their lengths"""
    _, _, a, _, _ = make_case("ragged", nlist=nlist)
    a = np.resize(a, nb).copy()
    for l, want in SPECIAL.items():
        idx = np.nonzero(a == l)[0]
        a[idx[want:]] = 0
    sizes = np.bincount(a, minlength=nlist)
    assert all(sizes[l] == n for l, n in SPECIAL.items()) and sizes[1] == sizes[5] == sizes[6] == 0
    return a


def byte_case(d, nlist, seed, top=255, clustered=True, nq=300, nb=NB):
    """byte-valued lists and queries: around byte centroids (the seed search then finds most neighbours), or uniform"""
    rs = np.random.RandomState(seed)
    assign = ragged_assign(nlist, nb)
    cen = rs.randint(0, top + 1, size=(nlist, d)).astype(np.float32)
    if clustered:
        w = max(1, top // 8)
        xb = np.clip(cen[assign] + rs.randint(-w, w + 1, size=(nb, d)), 0, top).astype(np.float32)
        xq = np.clip(cen[rs.randint(0, nlist, size=nq)] + rs.randint(-w, w + 1, size=(nq, d)), 0, top).astype(np.float32)
    else:
        xb = rs.randint(0, top + 1, size=(nb, d)).astype(np.float32)
        xq = rs.randint(0, top + 1, size=(nq, d)).astype(np.float32)
    return cen, assign, xb, xq


def make_handle(capi, metric, cen, xb, assign):
    h = capi.Handle(cen.shape[1], cen.shape[0], metric, 0)
    h.set_centroids(cen)
    h.set_lists_from_assign(xb, assign)
    return h


def identity_keys(n, nlist):
    return np.tile(np.arange(nlist, dtype=np.int64), (n, 1))


def expected(oracle, lists, xq, k):
    keys = identity_keys(len(xq), lists.nlist)
    D, I, _ = oracle.search_preassigned(lists, xq, k, keys, np.zeros(keys.shape, np.float32))
    return D, I


def check(oracle, h, lists, xq, k, what=""):
    """search_exact == the oracle == search_preassigned with identity keys on the same handle; returns last_exact"""
    eD, eI = expected(oracle, lists, xq, k)
    D, I = h.search_exact(xq, k)
    last = h.last_exact()
    bad = np.nonzero((I != eI).any(axis=1) | (bits(D) != bits(eD)).any(axis=1))[0]
    assert bad.size == 0, (what, "queries", bad[:8], last, I[bad[0]][:8], eI[bad[0]][:8], D[bad[0]][:8], eD[bad[0]][:8])
    pD, pI = h.search_preassigned(xq, k, identity_keys(len(xq), lists.nlist))
    assert np.array_equal(pI, eI) and np.array_equal(bits(pD), bits(eD)), (what, "search_preassigned")
    assert last[0] + last[1] + last[2] == len(xq), (what, last)
    return last


def exact_ties(metric, xb, xq, k):
    """queries in which equal values meet among the best min(k + 1, ntotal) distances, from exact int64 arithmetic"""
    a, b = xq.astype(np.int64), xb.astype(np.int64)
    ip = a @ b.T
    dis = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * ip if metric == L2 else -ip
    w = min(k + 1, len(xb))
    best = np.sort(dis, axis=1)[:, :w]
    within = (dis <= best[:, min(k, len(xb)) - 1][:, None]).sum(1)  # entries at or within the true k-th distance
    return (best[:, 1:] == best[:, :-1]).any(axis=1), within


@pytest.mark.parametrize("d,metric,nlist", [(8, L2, 16), (8, IP, 32), (30, L2, 32), (30, IP, 16), (32, L2, 16), (32, IP, 32), (64, L2, 32),
                                            (64, IP, 16), (96, L2, 16), (96, IP, 32), (128, L2, 32), (128, IP, 16)])
def test_exact_equals_oracle_over_ragged_byte_lists(capi, oracle, d, metric, nlist):
    cen, assign, xb, xq = byte_case(d, nlist, seed=100 + d + metric)
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    served = 0
    for n, k in BATCHES:
        h.stats(reset=True)
        last = check(oracle, h, lists, xq[:n], k, (d, metric, nlist, n, k))
        served += last[0]
        if last[0]:
            assert last[3] >= last[0] * k, last  # (a served query has at least its k best among its candidates)
    assert h.scan_arith() == 2
    assert served > 0, "the list pass served no query in any batch"
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("which", ["few_ties", "many_ties"])
def test_the_pass_serves_exactly_the_queries_without_ties(capi, oracle, metric, which):
    n, k = 300, 10
    if which == "few_ties":  # random uint8, d = 128: at most a quarter of the queries tie
        nlist = 32
        cen, assign, xb, xq = byte_case(128, nlist, seed=7, clustered=False, nq=n)
    else:                    # values 0 .. 3, d = 8: at least three quarters tie
        nlist = 16
        cen, assign, xb, xq = byte_case(8, nlist, seed=8, top=3, clustered=False, nq=3 * n)
    # the queries are chosen here, on the CPU: the first n whose entries at or within the true k-th distance fill at most half the
    # default capacity of 1024 slots (a query of small values ties with thousands of entries under the inner product: it would
    # leave the pass for its candidate count, not for its ties)
    tied, within = exact_ties(metric, xb, xq, k)
    pick = np.nonzero(within <= 512)[0][:n]
    assert len(pick) == n, len(pick)
    xq, ties = xq[pick], int(tied[pick].sum())
    assert ties <= n // 4 if which == "few_ties" else ties >= 3 * n // 4, ties
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    h.stats(reset=True)
    last = check(oracle, h, lists, xq, k, which)
    print(which, metric, "numpy ties", ties, "last_exact", last)
    assert last[1] == ties and last[2] == 0 and last[0] == n - ties, (last, ties)
    st = h.stats()
    # check() searches twice.  The exact call counts every list for every query; search_preassigned, like the reference, only the lists
    # that hold entries
    filled = int((np.bincount(assign, minlength=nlist) > 0).sum())
    assert (st["nq"], st["nlist"], st["ndis"]) == (2 * n, n * nlist + n * filled, 2 * n * NB), st
    h.close()


def test_k_beyond_ntotal_and_beyond_the_first_lists(capi, oracle):
    # 60 entries in all: k = 64 ends in the reference's padding; the whole call goes the general way
    cen, assign, xb, xq = byte_case(32, 16, seed=21, nq=40, nb=NB)
    keep = np.concatenate([np.nonzero(assign == l)[0][:6] for l in (0, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13)])[:60]
    lists = oracle.Lists(L2, cen, xb[keep], assign[keep], keep)
    h = capi.Handle(32, 16, L2, 0)
    h.set_centroids(cen)
    h.set_lists_from_assign(xb[keep], assign[keep], keep)
    last = check(oracle, h, lists, xq, 64, "k > ntotal")
    assert last[2] == len(xq) and h.search_exact(xq, 64)[1][:, 60:].max() == -1
    h.close()
    # k = 100 on the ragged index: lists 1 .. 12 hold fewer than k entries each (the first lists a scan meets fill no heap)
    lists = oracle.Lists(IP, cen, xb, assign)
    h = make_handle(capi, IP, cen, xb, assign)
    last = check(oracle, h, lists, xq, 100, "k > first lists")
    assert last[0] > 0
    h.close()


@pytest.mark.parametrize("what", ["query_256", "l2_96", "ip_96", "bytes_200", "byte_codes_off"])
def test_a_call_that_does_not_qualify_goes_the_general_way_whole(capi, oracle, what):
    n, k = 40, 10
    if what in ("l2_96", "ip_96", "bytes_200"):
        metric, cen, assign, xb, xq = make_case(what)
        xq = xq[:n]
    else:
        metric = L2
        cen, assign, xb, xq = byte_case(64, 16, seed=31, nq=n, nb=4000)
        if what == "query_256":
            xq[5, 3] = 256.0  # one value outside the byte rule
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    if what == "byte_codes_off":
        h.set_byte_codes(0)
    h.stats(reset=True)
    last = check(oracle, h, lists, xq, k, what)
    assert last == (0, 0, n, 0), last
    h.close()


def test_after_changes_of_the_lists_on_a_clone_and_resident(capi, oracle):
    metric, cen, assign, xb, xq = make_case("sift_l2")
    nlist, d = cen.shape
    rs = np.random.RandomState(5)
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(nlist, d, xb, assign)
    k = 10
    check(oracle, h, oracle.Lists(metric, cen, *model.flat()), xq[:70], k, "before")

    def lists_now():
        fx, fa, fi = model.flat()
        return oracle.Lists(metric, cen, fx, fa, fi)

    # amd_ivf_add: the journal is pending when the exact call starts
    to = np.array([2] * 40 + [3, 7, 7], np.int64)
    x = np.clip(cen[to] + rs.randint(-25, 26, size=(len(to), d)), 0, 255).astype(np.float32)
    ids = np.arange(50000, 50000 + len(to), dtype=np.int64)
    h.add(x, ids, to)
    model.add(x, ids, to)
    last = check(oracle, h, lists_now(), xq[:70], k, "add")
    assert last[0] > 0 and h.last_update()[0] == 1
    # amd_ivf_remove_ids
    sel = [model.ids[3][1], model.ids[3][-1]] + list(model.ids[9][:50])
    assert h.remove_ids(np.array(sel)) == model.remove_ids(sel)
    check(oracle, h, lists_now(), xq[:70], k, "remove")
    # amd_ivf_update_lists: grow one list, shrink another, overwrite an entry
    sizes = [len(i) for i in model.ids]
    new_sizes = list(sizes)
    new_sizes[4] += 2
    new_sizes[10] -= 3
    where = [(4 << 32) | sizes[4], (4 << 32) | (sizes[4] + 1), (11 << 32) | 0]
    wl = np.array([w >> 32 for w in where])
    x = np.clip(cen[wl] + rs.randint(-25, 26, size=(len(where), d)), 0, 255).astype(np.float32)
    ids = np.arange(60000, 60000 + len(where), dtype=np.int64)
    h.update_lists(new_sizes, np.array(where, np.uint64), ids, x)
    model.update(new_sizes, where, ids, x)
    lists = lists_now()
    check(oracle, h, lists, xq[:70], k, "update_lists")
    # on a clone, and the resident form over a slice that does not start at 0 (on the owner and on the clone)
    c = h.clone()
    last = check(oracle, c, lists, xq[:130], k, "clone")
    assert last[0] > 0
    eD, eI = expected(oracle, lists, xq, k)
    for ctx in (h, c):
        ctx.set_queries(xq)
        D, I = ctx.search_exact_resident(37, 150, k)
        assert np.array_equal(I, eI[37:187]) and np.array_equal(bits(D), bits(eD[37:187]))
        assert sum(ctx.last_exact()[:3]) == 150
    with pytest.raises(capi.EngineError) as e:
        h.search_exact_resident(200, 100, k)  # 256 resident queries
    assert e.value.code == -2
    c.close()
    h.close()


def test_reused_buffers_a_larger_then_a_smaller_call(capi, oracle):
    cen, assign, xb, xq = byte_case(96, 16, seed=41, nq=300, nb=6000)
    lists = oracle.Lists(L2, cen, xb, assign)
    h = make_handle(capi, L2, cen, xb, assign)
    for n, k in ((20, 10), (300, 64), (7, 10), (260, 1), (64, 100)):
        check(oracle, h, lists, xq[:n], k, ("reuse", n, k))
    h.close()


def test_an_empty_index(capi, oracle):
    for metric in (L2, IP):
        h = capi.Handle(32, 16, metric, 0)
        h.set_centroids(np.zeros((16, 32), np.float32))
        h.stats(reset=True)
        D, I = h.search_exact(np.ones((5, 32), np.float32), 3)
        assert (I == -1).all() and (D == (np.float32(3.4028234663852886e38) if metric == L2 else -np.float32(3.4028234663852886e38))).all()
        assert h.last_exact() == (0, 0, 5, 0)
        st = h.stats()
        assert (st["nq"], st["nlist"], st["ndis"], st["nheap_updates"]) == (5, 80, 0, 0)
        h.close()


def test_the_class_mirror(capi, oracle, tmp_path):
    """IndexIVFFlat::search_exact and exact_info of the C++ mirror, and the subset index's on its own handle (tests/cpp/exact_driver.cpp)"""
    from auncel_amd import build
    build.build_host()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "exact_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "exact_driver.cpp"), "-I", os.path.join(root, "auncel_amd", "csrc", "host"),
                    "-L", build.LIBDIR, "-lfaiss_amd", "-launcel_amd", "-Wl,-rpath," + build.LIBDIR, "-pthread", "-o", exe], check=True)
    cen, assign, xb, xq = byte_case(64, 16, seed=51, nq=100, nb=5000)
    order = np.argsort(assign, kind="stable")  # the driver adds list by list: the ids are the positions in that order
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    k = 10
    with open(inp, "wb") as f:
        np.array([64, 16, len(xb), len(xq), k], np.int64).tofile(f)
        cen.tofile(f)
        xb[order].tofile(f)
        assign[order].astype(np.int64).tofile(f)
        xq.tofile(f)
    p = subprocess.run([exe, inp, outp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    raw = np.fromfile(outp, dtype=np.uint8)
    n = len(xq)
    o = 0

    def take(count, dt):
        nonlocal o
        a = raw[o:o + count * np.dtype(dt).itemsize].view(dt)
        o += a.nbytes
        return a

    lists = oracle.Lists(L2, cen, xb[order], assign[order])
    eD, eI = expected(oracle, lists, xq, k)
    D, I, info = take(n * k, np.float32).reshape(n, k), take(n * k, np.int64).reshape(n, k), take(4, np.uint64)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    assert info[0] > 0 and int(info[0] + info[1] + info[2]) == n
    # the subset of the even ids
    even = np.nonzero(np.arange(len(xb)) % 2 == 0)[0]
    sub = oracle.Lists(L2, cen, xb[order][even], assign[order][even], even)
    eD, eI = expected(oracle, sub, xq, k)
    D, I, info = take(n * k, np.float32).reshape(n, k), take(n * k, np.int64).reshape(n, k), take(4, np.uint64)
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    assert int(info[0] + info[1] + info[2]) == n


def run_child(tmp_path, env_extra, calls, arrays):
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, manifest=np.array(json.dumps(calls)), **arrays)
    env = dict(os.environ)
    env.update(env_extra)
    p = subprocess.run([sys.executable, CHILD, inp, outp], env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(outp)


def test_candidate_overflow_in_a_child_process(oracle, tmp_path):
    """AUNCEL_AMD_EXACT_CAP=16: with k = 10 and a threshold from half the lists, queries overflow their 16 slots"""
    cen, assign, xb, xq = byte_case(64, 32, seed=61, clustered=False, nq=200)
    calls = [dict(name=f"m{m}", metric=m, cen="cen", xb="xb", assign="assign", xq="xq", k=10) for m in (L2, IP)]
    out = run_child(tmp_path, {"AUNCEL_AMD_EXACT_CAP": "16", "AUNCEL_AMD_EXACT_SEED": "4"}, calls, dict(cen=cen, xb=xb, assign=assign, xq=xq))
    for m in (L2, IP):
        eD, eI = expected(oracle, oracle.Lists(m, cen, xb, assign), xq, 10)
        last = out[f"m{m}/last"]
        print("cap 16, metric", m, "last_exact", last)
        assert np.array_equal(out[f"m{m}/I"], eI) and np.array_equal(bits(out[f"m{m}/D"]), bits(eD))
        assert last[2] > 0 and last[:3].sum() == len(xq), last


def test_a_loose_seed_in_a_child_process(oracle, tmp_path):
    """AUNCEL_AMD_EXACT_SEED=1 on clustered data: the threshold comes from one list, many candidates per query"""
    cen, assign, xb, xq = byte_case(128, 32, seed=71, nq=200)
    calls = [dict(name=f"m{m}", metric=m, cen="cen", xb="xb", assign="assign", xq="xq", k=10) for m in (L2, IP)]
    out = run_child(tmp_path, {"AUNCEL_AMD_EXACT_SEED": "1"}, calls, dict(cen=cen, xb=xb, assign=assign, xq=xq))
    for m in (L2, IP):
        eD, eI = expected(oracle, oracle.Lists(m, cen, xb, assign), xq, 10)
        last = out[f"m{m}/last"]
        print("seed 1, metric", m, "last_exact", last)
        assert np.array_equal(out[f"m{m}/I"], eI) and np.array_equal(bits(out[f"m{m}/D"]), bits(eD))
        assert last[:3].sum() == len(xq) and last[3] >= last[0] * 10, last
