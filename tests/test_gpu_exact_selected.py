"""Exact k-NN under an id selector (amd_ivf_search_exact_selected): (D, I) are, bit for bit, the pinned CPU oracle's
search_preassigned over every list in list-number order WITH THE NON-MEMBERS REMOVED -- and what search_exact returns on
subset(the same selector), and what search_preassigned_selected returns for identity keys on the same handle.  Byte lists at every
K-step count of the list pass, float lists through the fp16 pass, ragged lists (lengths 0, 1, 31, 32, 33, 63, 64, 65, 70), selectors
from everything to nothing, non-members closer than every member, ties that exist among all entries but not among the members, the
seed rule's two sides, stale and foreign selectors, clones, resident queries, reused buffers and the statistics.  Every comparison is
of bits or integers.

Not checked: "the fp16 pass emits no more under a selector than without one".  It does not follow from the design even at equal seed
nprobe: the selected seed's threshold is the k-th best MEMBER of the lists it read, which lies at or beyond the unfiltered seed's
k-th best entry, so the members within the one can outnumber the entries within the other.  What does follow, and is checked: a
selector that keeps everything emits exactly what the unfiltered call emits, and a served query has at least its k best members among
its candidates."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_exact import IP, L2, NB, SPECIAL, bits, byte_case, exact_ties, expected, identity_keys, make_handle
from test_gpu_subset import filtered, id_bits, oracle_lists, selector
from test_gpu_update import Model, make_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "exact_selected_child.py")
FLT_MAX = np.float32(3.4028234663852886e38)
SELECTORS = ["bits_half", "mod_3_1", "range_third", "bits_lists", "batch_200", "bits_all"]
NLIST = 64  # the default seed of 16 lists, scaled by a selector that keeps a third, stays below it


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def same(D, I, eD, eI):
    return np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))


def seed_under(seed, ntotal, kept):
    """exact_args.h: exact_selected_seed"""
    return -(-seed * ntotal // kept)


def check(oracle, capi, h, metric, cen, model, spec, rule, xq, k, what="", subset=True):
    """search_exact_selected == the oracle over the filtered lists == search_preassigned_selected with identity keys == search_exact of
    the subset; returns (last_exact, last_exact_detail, D, I) of the selected call"""
    kind, a1, a2, sel = spec
    want = filtered(model, rule)
    eD, eI = expected(oracle, oracle_lists(oracle, metric, cen, want), xq, k)
    with h.selector(kind, a1, a2, sel) as s:
        assert s.info()[1] == sum(len(i) for i in want.ids), what
        D, I = h.search_exact_selected(s, xq, k)
        last, detail = h.last_exact(), h.last_exact_detail()
        bad = np.nonzero((I != eI).any(axis=1) | (bits(D) != bits(eD)).any(axis=1))[0]
        assert bad.size == 0, (what, "queries", bad[:8], last, I[bad[0]][:8], eI[bad[0]][:8], D[bad[0]][:8], eD[bad[0]][:8])
        pD, pI = h.search_preassigned_selected(s, xq, k, identity_keys(len(xq), cen.shape[0]))
        assert same(pD, pI, eD, eI), (what, "search_preassigned_selected")
    if subset:
        sub = h.subset(kind, a1, a2, sel)
        for key in ("exact_float", "exact_seed_nprobe"):  # (the options are copied at the cut; said again for the reader)
            assert sub.get_option(key) == h.get_option(key)
        sD, sI = sub.search_exact(xq, k)
        assert same(sD, sI, eD, eI), (what, "subset.search_exact")
        sub.close()
    assert last[0] + last[1] + last[2] == len(xq), (what, last)
    assert last[3] == detail[1] and detail[2] >= last[0] * k, (what, last, detail)
    return last, detail, D, I


@pytest.mark.parametrize("d,metric", [(8, L2), (30, IP), (64, L2), (128, IP), (128, L2)])
def test_parity_on_ragged_byte_lists(capi, oracle, d, metric):
    cen, assign, xb, xq = byte_case(d, NLIST, seed=200 + d + metric)
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(NLIST, d, xb, assign)
    ks = dict(bits_half=10, mod_3_1=64, range_third=1, bits_lists=100, batch_200=10, bits_all=10)
    for name in SELECTORS:
        spec, rule = selector(capi, name, model)
        k = ks[name]
        last, detail, D, I = check(oracle, capi, h, metric, cen, model, spec, rule, xq, k, (d, metric, name))
        print(d, metric, name, "k", k, "last_exact", last, "detail", detail)
        if name == "batch_200":  # 150 members: the scaled seed is past nlist, the whole call goes the general way
            assert last == (0, 0, len(xq), 0) and detail[0] == 0, last
        else:
            assert detail[0] == 1 and last[0] > 0, (name, last, detail)
        if name == "bits_all":  # every entry is a member: the unfiltered call, bit for bit and candidate for candidate
            uD, uI = h.search_exact(xq, k)
            assert same(D, I, uD, uI)
            assert h.last_exact() == last and h.last_exact_detail() == detail
    assert h.scan_arith() == 2
    h.close()


@pytest.mark.parametrize("name", ["l2_96", "ip_96"])
def test_parity_on_float_lists(capi, oracle, name):
    metric, cen, assign, xb, xq = make_case(name)
    nlist, d = cen.shape
    h = make_handle(capi, metric, cen, xb, assign)
    h.set_option("exact_seed_nprobe", 2)  # 16 lists: twice to six times two stays below them
    model = Model(nlist, d, xb, assign)
    for fl in (1, 0):
        h.set_option("exact_float", fl)
        for sel_name in SELECTORS:
            spec, rule = selector(capi, sel_name, model)
            last, detail, D, I = check(oracle, capi, h, metric, cen, model, spec, rule, xq, 10, (name, fl, sel_name), subset=fl == 1)
            print(name, "exact_float", fl, sel_name, "last_exact", last, "detail", detail)
            if fl == 0 or sel_name == "batch_200":
                assert last == (0, 0, len(xq), 0) and detail[0] == 0, last
            else:
                assert detail[0] == 2 and last[0] > 0, (sel_name, last, detail)
                assert detail[2] <= detail[1], detail  # (what the rescoring keeps is among what the pass emitted)
            if fl == 1 and sel_name == "bits_all":
                uD, uI = h.search_exact(xq, 10)
                assert same(D, I, uD, uI)
                assert h.last_exact() == last and h.last_exact_detail() == detail
    h.close()


@pytest.mark.parametrize("kind", ["bytes", "float"])
def test_nothing_kept_is_padding_and_emits_nothing(capi, oracle, kind):
    if kind == "bytes":
        metric = IP
        cen, assign, xb, xq = byte_case(64, NLIST, seed=301, nb=5000)
    else:
        metric, cen, assign, xb, xq = make_case("l2_96")
    h = make_handle(capi, metric, cen, xb, assign)
    h.set_option("exact_float", 1)
    model = Model(cen.shape[0], cen.shape[1], xb, assign)
    spec, rule = selector(capi, "bits_none", model)
    h.stats(reset=True)
    last, detail, D, I = check(oracle, capi, h, metric, cen, model, spec, rule, xq, 5, kind)
    assert (I == -1).all() and (D == (FLT_MAX if metric == L2 else -FLT_MAX)).all()
    assert last == (0, 0, len(xq), 0) and detail == (0, 0, 0, 0)
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_non_members_closer_than_every_member(capi, oracle, metric):
    """the selector excludes exactly each query's unfiltered top k: what a pass that did not read the bits would return"""
    k = 10
    cen, assign, xb, xq = byte_case(64, NLIST, seed=310 + metric)
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(NLIST, 64, xb, assign)
    _, uI = h.search_exact(xq, k)
    best = np.unique(uI[uI >= 0])
    held = set(int(v) for v in best)
    rule = lambda ids, l, seen: np.array([int(v) not in held for v in ids], bool)  # noqa: E731
    eD, eI = expected(oracle, oracle_lists(oracle, metric, cen, filtered(model, rule)), xq, k)
    with h.selector(capi.SUBSET_ID_BATCH, 0, 0, best) as top, ~top as s:
        assert s.info()[1] == NB - len(best)
        D, I = h.search_exact_selected(s, xq, k)
        last, detail = h.last_exact(), h.last_exact_detail()
        assert not np.isin(I, best).any()
        assert same(D, I, eD, eI)
        pD, pI = h.search_preassigned_selected(s, xq, k, identity_keys(len(xq), NLIST))
        assert same(pD, pI, eD, eI)
    assert detail[0] == 1 and last[0] > 0 and sum(last[:3]) == len(xq), (last, detail)
    h.close()


def dup_case(metric, n=300, k=10):
    """5000 random byte rows of d = 128, each stored twice (ids i and i + 5000, in different lists); the queries are those in which,
    by exact integer arithmetic on the CPU, no two of the best k + 1 DISTINCT rows are equally far.  the callers choose which copies are members"""
    nb = 5000
    cen, assign, xb, xq = byte_case(128, NLIST, seed=320 + metric, clustered=False, nq=2 * n, nb=2 * nb)
    xb = np.concatenate([xb[:nb], xb[:nb]])
    tied, within = exact_ties(metric, xb[:nb], xq, k)
    pick = np.nonzero(~tied & (within <= 256))[0][:n]
    assert len(pick) == n, len(pick)
    return cen, assign, xb, xq[pick], nb


@pytest.mark.parametrize("metric", [L2, IP])
def test_ties_count_among_members_only(capi, oracle, metric):
    n, k = 300, 10
    cen, assign, xb, xq, nb = dup_case(metric, n, k)
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(NLIST, 128, xb, assign)
    # every entry: each of a query's best rows is there twice, at the same distance
    h.search_exact(xq, k)
    assert h.last_exact()[1] == n, h.last_exact()
    # one copy of every pair: no query is sent on for a tie
    spec, rule = (capi.SUBSET_ID_RANGE, 0, nb, None), lambda ids, l, seen: ids < nb
    last, detail, _, _ = check(oracle, capi, h, metric, cen, model, spec, rule, xq, k, "one copy")
    print("one copy", metric, last, detail)
    assert last[1] == 0 and last[0] > 0 and detail[0] == 1, (last, detail)
    # both copies kept: the ties are back
    spec, rule = (capi.SUBSET_ID_RANGE, 0, 2 * nb, None), lambda ids, l, seen: ids >= 0
    last, detail, _, _ = check(oracle, capi, h, metric, cen, model, spec, rule, xq, k, "both copies")
    print("both copies", metric, last, detail)
    assert last[1] == n, last
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_statistics(capi, oracle, metric):
    """ndis counts the parent's entries, nlist every list, nheap_updates what the oracle counts over the filtered lists for exactly
    the queries that went the general way: those in which, by numpy, equal distances meet among the best k + 1 members"""
    n, k = 300, 10
    cen, assign, xb, xq, nb = dup_case(metric, n, k)
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(NLIST, 128, xb, assign)
    # one copy of every row, the second of every thirtieth (inner product: seventh -- the best rows are the few longest ones, the same
    # for most queries, so whether a query ties hangs on a handful of rows)
    step = 30 if metric == L2 else 7
    member = lambda ids: (ids < nb) | ((ids - nb) % step == 0)  # noqa: E731
    chosen = np.nonzero(member(np.arange(2 * nb)))[0]
    want = filtered(model, lambda ids, l, seen: member(ids))
    lists = oracle_lists(oracle, metric, cen, want)
    eD, eI = expected(oracle, lists, xq, k)
    tied, _ = exact_ties(metric, xb[chosen], xq, k)
    assert 20 <= tied.sum() <= n - 20, tied.sum()  # (a row of the best 11 that is there twice: some queries, not all)
    with h.selector(capi.SUBSET_ID_BITS, 0, 0, id_bits(chosen, 2 * nb // 64 + 2)) as s:
        h.stats(reset=True)
        D, I = h.search_exact_selected(s, xq, k)
        st, last = h.stats(), h.last_exact()
    assert same(D, I, eD, eI)
    print("statistics", metric, "numpy ties", int(tied.sum()), "last_exact", last, st)
    assert last[1] == tied.sum() and last[2] == 0 and last[0] == n - tied.sum(), (last, tied.sum())
    redo = np.nonzero(tied)[0]
    keys = identity_keys(len(redo), NLIST)
    _, _, est = oracle.search_preassigned(lists, xq[redo], k, keys, np.zeros(keys.shape, np.float32))
    assert (st["nq"], st["nlist"], st["ndis"]) == (n, n * NLIST, n * 2 * nb), st
    assert st["nheap_updates"] == est[2], (st, est)
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_list_ends(capi, oracle, metric):
    """lists of 0, 1, 31, 32, 33, 63, 64, 65 and 70 entries (three blocks, padded to four) under selectors made by NOT: a pass that
    read a keep bit past a list's end, or the padding block behind it, would return a slot that holds nothing"""
    k = 10
    cen, assign, xb, xq = byte_case(96, NLIST, seed=330 + metric)
    # a third of the queries at the short lists' own centres
    short = np.array(sorted(SPECIAL), np.int64)
    xq[:100] = cen[short[np.arange(100) % len(short)]]
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(NLIST, 96, xb, assign)
    sizes = [len(i) for i in model.ids]
    assert all(sizes[l] == v for l, v in SPECIAL.items())
    for name in ("bits_none", "bits_half"):
        (kind, a1, a2, sel), rule = selector(capi, name, model)
        want = filtered(model, lambda ids, l, seen: ~rule(ids, l, seen))
        eD, eI = expected(oracle, oracle_lists(oracle, metric, cen, want), xq, k)
        with h.selector(kind, a1, a2, sel) as a, ~a as s:
            assert s.info()[1] == sum(len(i) for i in want.ids)
            D, I = h.search_exact_selected(s, xq, k)
            last, detail = h.last_exact(), h.last_exact_detail()
        assert (I >= 0).all()
        assert same(D, I, eD, eI), name
        assert detail[0] == 1 and last[0] > 0 and sum(last[:3]) == len(xq), (name, last, detail)
        if name == "bits_none":
            uD, uI = h.search_exact(xq, k)
            assert same(D, I, uD, uI) and h.last_exact() == last
    h.close()


def test_few_members(capi, oracle):
    metric = L2
    cen, assign, xb, xq = byte_case(32, NLIST, seed=341, nb=NB)
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(NLIST, 32, xb, assign)
    n = len(xq)
    # ten members: k == kept, and k == kept + 1 with the padding in the last column
    ten = np.array([3, 500, 501, 7777, 12000, 12001, 15000, 19000, 19998, 19999], np.int64)
    spec, rule = (capi.SUBSET_ID_BATCH, 0, 0, ten), lambda ids, l, seen: np.isin(ids, ten)
    last, _, D, I = check(oracle, capi, h, metric, cen, model, spec, rule, xq, 10, "k == kept")
    assert last == (0, 0, n, 0) and (I >= 0).all()
    last, _, D, I = check(oracle, capi, h, metric, cen, model, spec, rule, xq, 11, "k == kept + 1")
    assert last == (0, 0, n, 0) and (I[:, :10] >= 0).all() and (I[:, 10] == -1).all() and (D[:, 10] == FLT_MAX).all()
    # one in a hundred: sixteen lists scaled by a hundred is every list, the whole call goes the general way
    spec, rule = selector(capi, "bits_1pct", model)
    last, detail, _, _ = check(oracle, capi, h, metric, cen, model, spec, rule, xq, 10, "bits_1pct")
    assert last == (0, 0, n, 0) and detail[0] == 0
    # one in ten, with a seed of two lists: twenty of sixty-four, the pass serves queries
    h.set_option("exact_seed_nprobe", 2)
    spec, rule = (capi.SUBSET_ID_MOD, 10, 3, None), lambda ids, l, seen: ids % 10 == 3
    assert seed_under(2, NB, NB // 10) == 20
    last, detail, _, _ = check(oracle, capi, h, metric, cen, model, spec, rule, xq, 10, "mod_10_3")
    print("mod_10_3", last, detail)
    assert detail[0] == 1 and last[0] > 0, (last, detail)
    # ... and with the default of sixteen the same selector is past nlist: the same bits by the other path
    h.set_option("exact_seed_nprobe", float("nan"))
    assert seed_under(16, NB, NB // 10) >= NLIST
    last, detail, _, _ = check(oracle, capi, h, metric, cen, model, spec, rule, xq, 10, "mod_10_3, default seed", subset=False)
    assert last == (0, 0, n, 0)
    h.close()


def test_lifetime_clone_resident_and_reused_buffers(capi, oracle):
    metric, cen, assign, xb, xq = make_case("sift_l2")
    nlist, d = cen.shape
    rs = np.random.RandomState(5)
    k = 10
    h = make_handle(capi, metric, cen, xb, assign)
    h.set_option("exact_seed_nprobe", 2)  # (16 lists; a selector that keeps a third makes it six)
    other = make_handle(capi, metric, cen, xb, assign)
    model = Model(nlist, d, xb, assign)
    L = capi.lib()

    def refused(f, word):
        with pytest.raises(capi.EngineError) as e:
            f()
        assert e.value.code == -2 and word in L.amd_ivf_last_error().decode(), L.amd_ivf_last_error()

    def right(ctx, s, rule, what):
        eD, eI = expected(oracle, oracle_lists(oracle, metric, cen, filtered(model, rule)), xq, k)
        D, I = ctx.search_exact_selected(s, xq, k)
        assert same(D, I, eD, eI), what
        assert sum(ctx.last_exact()[:3]) == len(xq)
        return eD, eI

    spec, rule = selector(capi, "mod_3_1", model)
    s0 = h.selector(*spec)
    right(h, s0, rule, "before")
    assert h.last_exact()[0] > 0
    # another index's selector
    foreign = other.selector(*spec)
    refused(lambda: h.search_exact_selected(foreign, xq, k), "another index")
    refused(lambda: h.search_exact_resident_selected(foreign, 0, 1, k), "another index")
    foreign.close()
    other.close()
    # amd_ivf_add: the old selector is stale, whether or not the journal has been applied; a new one sees the new entries
    to = np.array([2] * 40 + [3, 7, 7], np.int64)
    x = np.clip(cen[to] + rs.randint(-25, 26, size=(len(to), d)), 0, 255).astype(np.float32)
    ids = np.arange(50002, 50002 + 3 * len(to), 3, dtype=np.int64)  # (% 3 == 1: members)
    h.add(x, ids, to)
    model.add(x, ids, to)
    refused(lambda: h.search_exact_selected(s0, xq, k), "stale")
    s0.close()
    s1 = h.selector(*spec)
    right(h, s1, rule, "add")
    assert h.last_exact()[0] > 0
    # amd_ivf_remove_ids
    gone = [model.ids[3][1], model.ids[3][-1]] + list(model.ids[9][:50])
    assert h.remove_ids(np.array(gone)) == model.remove_ids(gone)
    refused(lambda: h.search_exact_selected(s1, xq, k), "stale")
    s1.close()
    s = h.selector(*spec)
    eD, eI = right(h, s, rule, "remove")
    # a clone, and resident queries over a slice that does not start at 0 (on the owner and on the clone)
    c = h.clone()
    right(c, s, rule, "clone")
    assert c.last_exact()[0] > 0
    for ctx in (h, c):
        ctx.set_queries(xq)
        D, I = ctx.search_exact_resident_selected(s, 37, 150, k)
        assert same(D, I, eD[37:187], eI[37:187])
        assert sum(ctx.last_exact()[:3]) == 150
    refused(lambda: h.search_exact_resident_selected(s, 200, 100, k), "range")  # 256 resident queries
    # a larger call, then smaller ones, then a larger k: the workspaces left behind change nothing
    for n, kk in ((256, 64), (7, 10), (130, 1), (64, 100)):
        eD, eI = expected(oracle, oracle_lists(oracle, metric, cen, filtered(model, rule)), xq[:n], kk)
        D, I = h.search_exact_selected(s, xq[:n], kk)
        assert same(D, I, eD, eI), (n, kk)
        D, I = c.search_exact_selected(s, xq[:n], kk)
        assert same(D, I, eD, eI), ("clone", n, kk)
    c.close()
    s.close()
    h.close()


def run_child(tmp_path, env_extra, calls, arrays):
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, manifest=np.array(json.dumps(calls)), **arrays)
    env = dict(os.environ)
    env.update(env_extra)
    p = subprocess.run([sys.executable, CHILD, inp, outp], env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(outp)


@pytest.mark.parametrize("what", ["overflow", "loose_seed"])
def test_candidate_overflow_and_a_loose_seed_in_a_child_process(oracle, tmp_path, what):
    """overflow: AUNCEL_AMD_EXACT_CAP=16 with k = 10 and a threshold from an eighth of the lists -- queries overflow their 16 slots and
    go the general way; loose_seed: AUNCEL_AMD_EXACT_SEED=1 on clustered data -- the threshold comes from two lists of 32"""
    if what == "overflow":
        cen, assign, xb, xq = byte_case(64, 32, seed=361, clustered=False, nq=200)
        env = {"AUNCEL_AMD_EXACT_CAP": "16", "AUNCEL_AMD_EXACT_SEED": "2"}
    else:
        cen, assign, xb, xq = byte_case(128, 32, seed=371, nq=200)
        env = {"AUNCEL_AMD_EXACT_SEED": "1"}
    calls = [dict(name=f"m{m}", metric=m, cen="cen", xb="xb", assign="assign", xq="xq", k=10, kind=1, a1=2, a2=1, sel=None) for m in (L2, IP)]
    out = run_child(tmp_path, env, calls, dict(cen=cen, xb=xb, assign=assign, xq=xq))
    model = Model(32, cen.shape[1], xb, assign)
    want = filtered(model, lambda ids, l, seen: ids % 2 == 1)
    for m in (L2, IP):
        eD, eI = expected(oracle, oracle_lists(oracle, m, cen, want), xq, 10)
        last, detail = out[f"m{m}/last"], out[f"m{m}/detail"]
        print(what, "metric", m, "last_exact", last, "detail", detail)
        assert same(out[f"m{m}/D"], out[f"m{m}/I"], eD, eI)
        assert last[:3].sum() == len(xq) and detail[0] == 1, (last, detail)
        if what == "overflow":
            assert last[2] > 0 and detail[3] > 16, (last, detail)
        else:
            assert last[3] >= last[0] * 10, last


def test_the_class_mirror(capi, oracle, tmp_path):
    """IndexIVFFlat::search_exact_selected with an IDSelectorRange and an IDSelectorBatch (tests/cpp/exact_selected_driver.cpp) against
    search_preassigned_selected of a handle over the same lists and the oracle; the selector search_selected made is not made again"""
    from auncel_amd import build
    build.build_host()
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "exact_selected_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "exact_selected_driver.cpp"), "-I",
                    os.path.join(root, "auncel_amd", "csrc", "host"), "-L", build.LIBDIR, "-lfaiss_amd", "-launcel_amd",
                    "-Wl,-rpath," + build.LIBDIR, "-pthread", "-o", exe], check=True)
    d, k = 64, 10
    cen, assign, xb, xq = byte_case(d, NLIST, seed=351, nq=100, nb=5000)
    order = np.argsort(assign, kind="stable")  # the driver adds list by list: the ids are the positions in that order
    xb, assign = xb[order], assign[order]
    imin, imax = 1000, 3500
    batch = np.random.RandomState(9).choice(len(xb), 2000, replace=False).astype(np.int64)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([d, NLIST, len(xb), len(xq), k, imin, imax, len(batch)], np.int64).tofile(f)
        cen.tofile(f)
        xb.tofile(f)
        assign.astype(np.int64).tofile(f)
        xq.tofile(f)
        batch.tofile(f)
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

    h = make_handle(capi, L2, cen, xb, assign)
    model = Model(NLIST, d, xb, assign)
    cases = [((capi.SUBSET_ID_RANGE, imin, imax, None), lambda ids, l, seen: (ids >= imin) & (ids < imax), 1),
             ((capi.SUBSET_ID_BATCH, 0, 0, batch), lambda ids, l, seen: np.isin(ids, batch), 2)]
    for spec, rule, passes in cases:
        D, I = take(n * k, np.float32).reshape(n, k), take(n * k, np.int64).reshape(n, k)
        info, made = take(4, np.uint64), take(3, np.uint64)
        eD, eI = expected(oracle, oracle_lists(oracle, L2, cen, filtered(model, rule)), xq, k)
        assert same(D, I, eD, eI)
        with h.selector(*spec) as s:
            pD, pI = h.search_preassigned_selected(s, xq, k, identity_keys(n, NLIST))
        assert same(D, I, pD, pI)
        assert info[0] > 0 and int(info[0] + info[1] + info[2]) == n, info
        assert list(made) == [passes] * 3, made  # (search_selected made it; neither exact call made it again)
    h.close()
