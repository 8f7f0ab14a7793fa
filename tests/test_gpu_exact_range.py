"""Exact range search over the whole index (amd_ivf_range_search_exact, ivf_exact.hip): lims, labels and distances
are, bit for bit, the pinned CPU oracle's range_search_preassigned over every list in list-number order -- and what range_search with
identity keys returns on the same handle -- over ragged byte lists at every K-step count, at the strict edge of the radius, through
the fp16 and the wide fp16 pass, with candidate overflow, under selectors, at degenerate radii and shapes, whatever the handle ran
before, and through the class mirror."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_exact import IP, L2, NB, bits, byte_case, identity_keys, make_handle
from test_gpu_exact_float import float_case
from test_gpu_subset import filtered, oracle_lists, selector
from test_gpu_update import Model

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "exact_range_child.py")
CAP = 1024  # the default candidate slots per query


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def int_dis(metric, xb, xq):
    """exact int64 distances of byte-valued rows, as the reference's fp32 holds them"""
    a, b = xq.astype(np.int64), xb.astype(np.int64)
    ip = a @ b.T
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * ip if metric == L2 else ip


def inside(metric, dis, radius):
    """the reference's strict range test"""
    return dis < radius if metric == L2 else dis > radius


def emitted(metric, dis, radius):
    """what the list pass emits: the non-strict test"""
    return dis <= radius if metric == L2 else dis >= radius


def quantile_radius(metric, dis, mean):
    """the distance value below (L2) / above (IP) which about `mean` entries per query lie"""
    m = int(mean * dis.shape[0])
    flat = dis.ravel()
    return float(np.partition(flat, m)[m] if metric == L2 else -np.partition(-flat, m)[m])


def want(oracle, lists, xq, radius):
    lims, lab, dis, _ = oracle.range_search_preassigned(lists, xq, radius, identity_keys(len(xq), lists.nlist))
    return lims, lab, dis


def same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and np.array_equal(bits(got[2]), bits(exp[2]))


def check(oracle, h, lists, xq, radius, what="", exp=None):
    """range_search_exact == the oracle == range_search with identity keys on the same handle; returns (last_range_exact, expected)"""
    exp = want(oracle, lists, xq, radius) if exp is None else exp
    got = h.range_search_exact(xq, radius)
    last = h.last_range_exact()
    assert np.array_equal(got[0], exp[0]), (what, "lims", last, np.nonzero(np.diff(got[0]) != np.diff(exp[0]))[0][:8])
    assert same(got, exp), (what, "labels / distances", last)
    gen = h.range_search(xq, radius, lists.nlist, keys=identity_keys(len(xq), lists.nlist))
    assert same(gen, exp), (what, "range_search with identity keys")
    return last, exp


def uniform_bytes(d, metric, nlist, seed, nq=300):
    """uniform byte lists over the ragged assignment; the queries are the nq of 3 nq whose squared norms lie nearest the median (under the
    inner product a query of large norm alone would hold thousands of results), query 3 one that has no result at any radius used"""
    cen, assign, xb, xq = byte_case(d, nlist, seed=seed, clustered=False, nq=3 * nq)
    s = (xq * xq).sum(1)
    xq = xq[np.sort(np.argsort(np.abs(s - np.median(s)), kind="stable")[:nq])].copy()
    xq[3] = 255 if metric == L2 else 0
    return cen, assign, xb, xq


# ---- 1. the byte pass over ragged lists
@pytest.mark.parametrize("d,metric,nlist", [(8, L2, 16), (8, IP, 32), (30, L2, 32), (30, IP, 16), (64, L2, 16), (64, IP, 32), (128, L2, 32), (128, IP, 16)])
def test_byte_pass_over_ragged_lists(capi, oracle, d, metric, nlist):
    cen, assign, xb, xq = uniform_bytes(d, metric, nlist, seed=500 + d + metric)
    dis = int_dis(metric, xb, xq)
    radius = quantile_radius(metric, dis, 20)
    counts = inside(metric, dis, radius).sum(1)
    most = int(emitted(metric, dis, radius).sum(1).max())
    print(d, metric, "radius", radius, "mean", counts.mean(), "zero", int((counts == 0).sum()), "largest emitted", most)
    assert 10 <= counts.mean() <= 20 and (counts == 0).any() and most < CAP  # the reference alone: no query overflows
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    exp_all = want(oracle, lists, xq, radius)
    assert np.array_equal(np.diff(exp_all[0]), counts)
    for n in (1, 65, 257, 300):
        exp = (exp_all[0][:n + 1], exp_all[1][:exp_all[0][n]], exp_all[2][:exp_all[0][n]])
        last, _ = check(oracle, h, lists, xq[:n], radius, (d, metric, n), exp)
        assert last[:3] == (1, n, 0) and last[3] == int(emitted(metric, dis[:n], radius).sum(1).max()), (n, last)
    assert h.scan_arith() == 2
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_counts_on_either_side_of_one_wave_and_of_the_slots(capi, oracle, metric):
    """about 300 results a query: counts below and beyond the 256 candidates one wave sorts, and queries beyond the 1024 slots -- the split
    between the pass and the general way is numpy's"""
    d, nlist = 64, 16
    cen, assign, xb, xq = uniform_bytes(d, metric, nlist, seed=540 + metric)
    dis = int_dis(metric, xb, xq)
    radius = quantile_radius(metric, dis, 300)
    em = emitted(metric, dis, radius).sum(1)
    over = int((em > CAP).sum())
    print(metric, "radius", radius, "emitted <= 256:", int((em <= 256).sum()), "257 .. 1024:", int(((em > 256) & (em <= CAP)).sum()), "beyond:", over)
    assert (em <= 256).sum() > 20 and ((em > 256) & (em <= CAP)).sum() > 20 and over > 0
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    last, _ = check(oracle, h, lists, xq, radius, ("wide counts", metric))
    assert last == (1, len(xq) - over, over, int(em.max())), last
    h.close()


# ---- 2. the strict edge
@pytest.mark.parametrize("metric", [L2, IP])
def test_the_strict_edge_on_byte_lists(capi, oracle, metric):
    d, nlist = 30, 16
    cen, assign, xb, xq = uniform_bytes(d, metric, nlist, seed=560 + metric, nq=40)
    dis = int_dis(metric, xb, xq)
    v = float(np.sort(dis[0])[15] if metric == L2 else -np.sort(-dis[0])[15])  # a stored integer distance of query 0
    at = int((dis[0] == v).sum())
    assert at >= 1
    past = float(np.nextafter(np.float32(v), np.float32(np.inf if metric == L2 else -np.inf)))
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    for radius, counts in ((v, inside(metric, dis, v).sum(1)), (past, emitted(metric, dis, v).sum(1))):
        last, exp = check(oracle, h, lists, xq, radius, ("edge", metric, radius))
        assert np.array_equal(np.diff(exp[0]), counts), radius
        assert last[:3] == (1, len(xq), 0), last
    assert int(emitted(metric, dis[0], v).sum() - inside(metric, dis[0], v).sum()) == at
    h.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_the_strict_edge_on_float_lists(capi, oracle, metric):
    d, nlist = 64, 16
    cen, assign, xb, xq = float_case(d, nlist, seed=570 + metric, nq=40, nb=6000)
    lists = oracle.Lists(metric, cen, xb, assign)
    a, b = xq.astype(np.float64), xb.astype(np.float64)
    dis64 = ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * a @ b.T) if metric == L2 else a @ b.T
    first = want(oracle, lists, xq, quantile_radius(metric, dis64[:1], 12))
    assert first[0][1] >= 4
    d0, l0 = first[2][:first[0][1]], first[1][:first[0][1]]
    j = int(np.argmax(d0) if metric == L2 else np.argmin(d0))  # the farthest entry the oracle returned for query 0
    v, label = np.float32(d0[j]), int(l0[j])
    past = float(np.nextafter(v, np.float32(np.inf if metric == L2 else -np.inf)))
    h = make_handle(capi, metric, cen, xb, assign)
    h.set_option("exact_float", 1)
    last, exp = check(oracle, h, lists, xq, float(v), ("float edge at", metric))
    assert label not in exp[1][:exp[0][1]] and last[0] == 2, last
    last, exp = check(oracle, h, lists, xq, past, ("float edge past", metric))
    assert label in exp[1][:exp[0][1]] and last[0] == 2, last
    h.close()


# ---- 3. the fp16 pass
def float_radius(metric, xb, xq, mean):
    a, b = xq.astype(np.float64), xb.astype(np.float64)
    dis = ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * a @ b.T) if metric == L2 else a @ b.T
    radius = quantile_radius(metric, dis, mean)
    return radius, inside(metric, dis, radius).sum(1)


@pytest.mark.parametrize("d,metric", [(64, L2), (64, IP), (96, L2), (96, IP), (128, L2), (128, IP)])
def test_fp16_pass_over_clustered_float_lists(capi, oracle, d, metric):
    nlist, n = 16, 300
    cen, assign, xb, xq = float_case(d, nlist, seed=600 + d + metric, nq=n)
    radius, approx = float_radius(metric, xb, xq, 20)
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    h.set_option("exact_float", 1)
    last, exp = check(oracle, h, lists, xq, radius, ("fp16", d, metric))
    counts = np.diff(exp[0])
    print(d, metric, "radius", radius, "mean", counts.mean(), "largest", counts.max(), "last_range_exact", last)
    assert last[0] == 2 and last[1] + last[2] == n and last[1] > n // 2, last
    # emitted >= valid: no answered query has more results than the largest emitted count; every query beyond the slots left the pass
    assert last[3] >= min(int(counts.max()), CAP) and last[2] >= int((counts > CAP).sum()), (last, counts.max())
    assert h.scan_arith() != 2
    h.close()


def test_fp16_pass_a_stored_zero_vector_and_a_zero_query(capi, oracle):
    """|x|^2 + |y|^2 = 0: the bound of the keep rule is 0 and the entry is still emitted (the S = 0 case)"""
    d, nlist = 64, 16
    cen, assign, xb, xq = float_case(d, nlist, seed=650, nq=70, nb=6000)
    xb[100] = 0
    xq[0] = 0
    lists = oracle.Lists(L2, cen, xb, assign)
    h = make_handle(capi, L2, cen, xb, assign)
    h.set_option("exact_float", 1)
    last, exp = check(oracle, h, lists, xq, 1e-30, "zero pair")
    assert last[:3] == (2, len(xq), 0), last
    assert exp[0][1] == 1 and exp[1][0] == 100 and bits(exp[2][:1])[0] == 0 and exp[0][-1] == 1
    h.close()


# ---- 4. the wide pass
@pytest.mark.parametrize("d,metric", [(160, L2), (160, IP), (960, L2), (960, IP)])
def test_wide_pass_and_the_general_way_without_the_options(capi, oracle, d, metric):
    nlist, n = 16, 150
    cen, assign, xb, xq = float_case(d, nlist, seed=600 + d + metric, nq=n, nb=4000)
    radius, approx = float_radius(metric, xb, xq, 20)
    assert approx.max() < CAP - 50
    lists = oracle.Lists(metric, cen, xb, assign)
    h = make_handle(capi, metric, cen, xb, assign)
    exp = want(oracle, lists, xq, radius)
    last, _ = check(oracle, h, lists, xq, radius, ("no options", d, metric), exp)
    assert last == (0, 0, n, 0), last
    h.set_option("exact_float", 1)
    last, _ = check(oracle, h, lists, xq, radius, ("exact_float alone", d, metric), exp)
    assert last == (0, 0, n, 0), last
    h.set_option("exact_wide", 1)
    last, _ = check(oracle, h, lists, xq, radius, ("wide", d, metric), exp)
    print(d, metric, "radius", radius, "largest", np.diff(exp[0]).max(), "last_range_exact", last)
    assert last[:3] == (3, n, 0) and last[3] >= np.diff(exp[0]).max(), last
    h.close()


# ---- 5. overflow
def test_candidate_overflow_in_a_child_process(oracle, tmp_path):
    """AUNCEL_AMD_EXACT_CAP=8: some queries hold at most 8 candidates, some more; the split is numpy's"""
    d, nlist = 64, 32
    arrays, calls, cases = {}, [], {}
    for metric in (L2, IP):
        cen, assign, xb, xq = uniform_bytes(d, metric, nlist, seed=700 + metric, nq=200)
        dis = int_dis(metric, xb, xq)
        radius = quantile_radius(metric, dis, 8)
        em = emitted(metric, dis, radius).sum(1)
        assert (em <= 8).sum() > 20 and (em > 8).sum() > 20
        tag = f"m{metric}"
        arrays.update({tag + "cen": cen, tag + "xb": xb, tag + "assign": assign, tag + "xq": xq})
        calls.append(dict(name=tag, metric=metric, cen=tag + "cen", xb=tag + "xb", assign=tag + "assign", xq=tag + "xq", radius=radius))
        cases[tag] = (metric, cen, assign, xb, xq, radius, em)
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, manifest=np.array(json.dumps(calls)), **arrays)
    env = dict(os.environ)
    env["AUNCEL_AMD_EXACT_CAP"] = "8"
    p = subprocess.run([sys.executable, CHILD, inp, outp], env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    out = np.load(outp)
    for tag, (metric, cen, assign, xb, xq, radius, em) in cases.items():
        exp = want(oracle, oracle.Lists(metric, cen, xb, assign), xq, radius)
        last = tuple(int(v) for v in out[tag + "/last"])
        print("cap 8, metric", metric, "last_range_exact", last)
        assert same((out[tag + "/lims"], out[tag + "/labels"], out[tag + "/dist"]), exp), tag
        assert last == (1, int((em <= 8).sum()), int((em > 8).sum()), int(em.max())), last


# ---- 6. selectors
@pytest.mark.parametrize("metric,floats", [(L2, False), (IP, False), (L2, True)])
def test_under_a_selector(capi, oracle, metric, floats):
    d, nlist = 64, 16
    if floats:
        cen, assign, xb, xq = float_case(d, nlist, seed=800, nq=130, nb=6000)
        radius, _ = float_radius(metric, xb, xq, 30)
    else:
        cen, assign, xb, xq = uniform_bytes(d, metric, nlist, seed=800 + metric, nq=130)
        radius = quantile_radius(metric, int_dis(metric, xb, xq), 30)
    h = make_handle(capi, metric, cen, xb, assign)
    h.set_option("exact_float", 1)
    model = Model(nlist, d, xb, assign)
    whole = h.range_search_exact(xq, radius)
    keys = identity_keys(len(xq), nlist)
    for name in ("range_third", "mod_3_1", "bits_lists"):  # (bits_lists: lists 0, 1 and 9 are emptied whole)
        (kind, a1, a2, sel), rule = selector(capi, name, model)
        kept = filtered(model, rule)
        members = set(int(v) for v in np.concatenate(kept.ids))
        exp = want(oracle, oracle_lists(oracle, metric, cen, kept), xq, radius)
        with h.selector(kind, a1, a2, sel) as s:
            got = h.range_search_exact_selected(s, xq, radius)
            last = h.last_range_exact()
            assert same(got, exp), (name, last)
            assert same(h.range_search_selected(s, xq, radius, nlist, keys=keys), exp), name
        sub = h.subset(kind, a1, a2, sel)
        assert same(sub.range_search_exact(xq, radius), exp), (name, "subset")
        sub.close()
        assert last[0] == (2 if floats else 1) and last[1] + last[2] == len(xq), (name, last)
        # a non-member inside the radius appears nowhere
        assert any(int(v) not in members for v in whole[1]) and all(int(v) in members for v in got[1]), name
    h.close()


def test_a_selector_that_is_stale_foreign_or_empty(capi, oracle):
    cen, assign, xb, xq = uniform_bytes(30, L2, 16, seed=850, nq=20)
    h = make_handle(capi, L2, cen, xb, assign)
    other = make_handle(capi, L2, cen, xb, assign)
    with h.selector(capi.SUBSET_ID_RANGE, 10 ** 9, 10 ** 9 + 5) as s:  # no member
        h.stats(reset=True)
        lims, lab, dis = h.range_search_exact_selected(s, xq, 1e9)
        assert not lims.any() and len(lims) == 21 and len(lab) == 0 and h.last_range_exact() == (0, 0, 0, 0)
    with h.selector(capi.SUBSET_ID_MOD, 3, 1) as s:
        with pytest.raises(capi.EngineError) as e:
            other.range_search_exact_selected(s, xq, 100.0)
        assert e.value.code == -2
        h.add(xb[:3], np.arange(10 ** 6, 10 ** 6 + 3, dtype=np.int64), np.array([2, 3, 4], np.int64))
        with pytest.raises(capi.EngineError) as e:
            h.range_search_exact_selected(s, xq, 100.0)
        assert e.value.code == -2 and "stale" in str(e.value)
    other.close()
    h.close()


# ---- 7. degenerate radii and shapes
def test_degenerate_radii_and_shapes(capi, oracle):
    d, nlist = 30, 16
    cen, assign, xb, xq = uniform_bytes(d, L2, nlist, seed=900, nq=70)
    dis = int_dis(L2, xb, xq)
    lists = oracle.Lists(L2, cen, xb, assign)
    h = make_handle(capi, L2, cen, xb, assign)
    n = len(xq)
    for radius in (float("nan"), -1.0, -float("inf"), -1e30):
        got = h.range_search_exact(xq, radius)
        assert not got[0].any() and len(got[0]) == n + 1 and len(got[1]) == 0, radius
        if radius == radius:
            last, _ = check(oracle, h, lists, xq, radius, ("empty side", radius))
            assert last == (1, n, 0, 0), (radius, last)
        else:
            assert h.last_range_exact() == (0, 0, 0, 0)
    for radius in (float("inf"), 1e30):  # every entry of every list, through the overflow, still equal
        last, exp = check(oracle, h, lists, xq[:2], radius, ("full side", radius))
        assert np.array_equal(exp[0], [0, NB, 2 * NB]) and last == (1, 0, 2, NB), last
    # the resident form equals the row form, on the owner and on a clone; outside the resident queries: refused
    radius = quantile_radius(L2, dis, 20)
    exp = want(oracle, lists, xq, radius)
    c = h.clone()
    for ctx in (h, c):
        ctx.set_queries(xq)
        assert same(ctx.range_search_exact_resident(0, n, radius), exp)
        part = ctx.range_search_exact_resident(7, 40, radius)
        assert np.array_equal(part[0], exp[0][7:48] - exp[0][7]) and np.array_equal(part[1], exp[1][exp[0][7]:exp[0][47]])
        assert np.array_equal(bits(part[2]), bits(exp[2][exp[0][7]:exp[0][47]]))
        assert ctx.last_range_exact()[:3] == (1, 40, 0)
        assert same(ctx.range_search_exact(xq, radius), exp)
        with pytest.raises(capi.EngineError) as e:
            ctx.range_search_exact_resident(60, 20, radius)
        assert e.value.code == -2
    c.close()
    # n = 0
    lims, lab, dd = h.range_search_exact(np.zeros((0, d), np.float32), radius)
    assert list(lims) == [0] and len(lab) == 0 and h.last_range_exact() == (0, 0, 0, 0)
    h.close()
    # an empty index
    for metric in (L2, IP):
        e = capi.Handle(d, nlist, metric, 0)
        e.set_centroids(cen)
        e.stats(reset=True)
        lims, lab, dd = e.range_search_exact(xq[:5], 1e9 if metric == L2 else -1e9)
        assert list(lims) == [0] * 6 and len(lab) == 0 and e.last_range_exact() == (0, 0, 0, 0)
        st = e.stats()
        assert (st["nq"], st["nlist"], st["ndis"], st["nheap_updates"]) == (5, 5 * nlist, 0, 0)
        e.close()


# ---- 8. the handle's history
@pytest.mark.parametrize("metric", [L2, IP])
def test_the_result_does_not_depend_on_what_the_handle_ran_before(capi, oracle, metric):
    d, nlist, n, k = 64, 16, 130, 10
    cen, assign, xb, xq = uniform_bytes(d, metric, nlist, seed=950 + metric, nq=n)
    radius = quantile_radius(metric, int_dis(metric, xb, xq), 20)
    keys = identity_keys(n, nlist)

    def fresh(f):
        g = make_handle(capi, metric, cen, xb, assign)
        r = f(g)
        g.close()
        return r

    ops = [lambda g: g.search_exact(xq, k), lambda g: g.range_search_exact(xq, radius), lambda g: g.range_search(xq, radius, nlist, keys=keys),
           lambda g: g.search_exact(xq, k)]
    alone = [fresh(f) for f in ops]
    h = make_handle(capi, metric, cen, xb, assign)
    for i, f in enumerate(ops):
        h.stats(reset=True)
        before = h.stats()
        got = f(h)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, alone[i])), i
        if i == 1:
            st = h.stats()
            assert (st["nq"], st["nlist"], st["ndis"], st["nheap_updates"]) == (n, n * nlist, n * NB, before["nheap_updates"]), st
            assert h.last_range_exact()[:3] == (1, n, 0)
    # ... and twice in a row the counts are the call's own
    h.range_search_exact(xq[:7], radius)
    assert h.last_range_exact()[:3] == (1, 7, 0)
    h.close()


# ---- 9. the class mirror
def test_the_class_mirror(capi, oracle, tmp_path):
    """IndexIVFFlat::range_search_exact / _selected / range_exact_info and the subset index's (tests/cpp/exact_range_driver.cpp)"""
    from auncel_amd import build
    build.build_host()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "exact_range_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "exact_range_driver.cpp"), "-I", os.path.join(root, "auncel_amd", "csrc", "host"),
                    "-L", build.LIBDIR, "-lfaiss_amd", "-launcel_amd", "-Wl,-rpath," + build.LIBDIR, "-pthread", "-o", exe], check=True)
    d, nlist = 64, 16
    cen, assign, xb, xq = uniform_bytes(d, L2, nlist, seed=990, nq=100)
    xb, assign = xb[:5000], assign[:5000]
    order = np.argsort(assign, kind="stable")  # the driver adds list by list: the ids are the positions in that order
    xb, assign = xb[order], assign[order]
    radius = quantile_radius(L2, int_dis(L2, xb, xq), 20)
    a1, a2 = 1000, 3500
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([d, nlist, len(xb), len(xq), a1, a2], np.int64).tofile(f)
        np.array([radius], np.float32).tofile(f)
        cen.tofile(f)
        xb.tofile(f)
        assign.astype(np.int64).tofile(f)
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

    ids = np.arange(len(xb))
    for what, keep in (("index", ids >= 0), ("IDSelectorRange", (ids >= a1) & (ids < a2)), ("subset of the even ids", ids % 2 == 0)):
        exp = want(oracle, oracle.Lists(L2, cen, xb[keep], assign[keep], ids[keep]), xq, radius)
        lims = take(n + 1, np.uint64).astype(np.int64)
        got = (lims, take(int(lims[n]), np.int64), take(int(lims[n]), np.float32))
        info = take(4, np.uint64)
        assert same(got, exp), what
        assert int(info[0]) == 1 and int(info[1] + info[2]) == n, (what, info)
    assert o == len(raw)
