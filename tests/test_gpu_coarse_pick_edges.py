"""The matrix-core coarse ranking (coarse_gemm16_kernel -> coarse_pick_kernel -> the exact re-run of the flagged rankings) at the edges
test_gpu_coarse_pick.py does not reach: tile, key and recomputation-loop edges, both sides of the engine's gate, the candidate cap, the
padded list of flagged rankings, degenerate queries -- and data whose fp16 rounding is coherent, so that the approximate distances are
off by half of the error bound and a too-small constant loses true neighbours (coarse_pick_cases.py: the data and the model).

Every comparison is bit for bit with the pinned oracle's ranking of ALL queries of the call; the exact path (coarse_pick = 0) of the
same call is a second check.  Every call also bounds last_coarse_pick() from the reference: with a / b the queries whose nprobe + 1 /
nprobe best reference distances are finite and pairwise distinct, a <= picked <= b -- the picked path answered what the design says it
answers (a ranking is flagged only for equal or non-finite distances among its candidates' first nprobe + 1), not less."""
import numpy as np
import pytest

import coarse_pick_cases as cp
from coarse_pick_cases import bits

pytestmark = pytest.mark.gpu


def run_forms(metric, xq, cen, nprobe, expect, tag, h=None, forms=(2, 1), options=()):
    """coarse_pick 0, then `forms`, on one handle against pyoracle.knn over every query.  expect: "served" (a <= picked <= b with
    a > 0), "bounds" (a <= picked <= b), "none" (picked == 0), or a dict form -> one of those.  -> {form: picked}, a, b"""
    from auncel_amd import capi
    from oracle import pyoracle
    n, d = xq.shape
    oD, oI = pyoracle.knn(metric, xq, cen, nprobe)
    a, b = cp.distinct_counts(pyoracle.knn(metric, xq, cen, nprobe + 1)[0]) if nprobe < len(cen) else (0, 0)
    own = h is None
    if own:
        h = capi.Handle(d, len(cen), metric, 0)
    h.set_centroids(cen)
    for key, value in options:
        h.set_option(key, value)
    h.set_option("coarse_pick", 0)
    D0, I0 = h.coarse(xq, nprobe, mode=0)
    assert h.last_coarse_pick() == 0
    assert np.array_equal(I0, oI) and np.array_equal(bits(D0), bits(oD)), (tag, "exact path")
    picked = {}
    for form in forms:  # approximate distances from fp16 operands (the default) / fp32 operands
        h.set_option("coarse_pick", form)
        D1, I1 = h.coarse(xq, nprobe, mode=0)
        picked[form] = p = h.last_coarse_pick()
        print(f"{tag} form={form}: picked {p} of {n}, reference bounds a={a} b={b}")
        wrong = np.nonzero((I1 != oI).any(axis=1) | (bits(D1) != bits(oD)).any(axis=1))[0]
        assert wrong.size == 0, (tag, form, f"{wrong.size} of {n} rankings differ from the oracle's, first {wrong[:8]}")
        e = expect[form] if isinstance(expect, dict) else expect
        if e == "none":
            assert p == 0, (tag, form, p)
        else:
            assert a <= p <= b, (tag, form, p, a, b)
            if e == "served":
                assert a > 0, (tag, "the reference leaves the picked path nothing to answer")
    if own:
        h.close()
    return picked, a, b


# ------------------------------------------------------------------------------------------ 1. shapes and the gate
KINDS = [(1, "float"), (1, "bytes"), (0, "float"), (0, "bytes")]


def shape_case(metric, kind, nlist, nprobe, n, d, expect="served", options=()):
    cen, xq = cp.near_centroids(kind, metric, nlist, n, d)
    return run_forms(metric, xq, cen, nprobe, expect, f"{kind} metric={metric} nlist={nlist} nprobe={nprobe} n={n} d={d}", options=options)


@pytest.mark.parametrize("metric,kind", KINDS)
@pytest.mark.parametrize("nlist,nprobe", [(68, 1), (577, 128), (1000, 32), (3841, 8), (4095, 32), (4096, 128)])
def test_nlist_edges(metric, kind, nlist, nprobe):
    """128-wide centroid tiles with a ragged last one (c0 + row < ny), the 256-wide key loop of coarse_pick_kernel with all 16 keys a
    thread in use from nlist = 3841, the engine's upper limit nlist = 4096, the lowest nlist of the gate at nprobe = 1 and 128"""
    shape_case(metric, kind, nlist, nprobe, 256, 8)


@pytest.mark.parametrize("metric,kind", KINDS)
@pytest.mark.parametrize("n", [255, 256, 257, 385])
def test_n_edges(metric, kind, n):
    """n = 255 keeps the exact path (the gate n >= 256); 257 and 385 leave a ragged last query tile (q0 + row < nq) of 1 row"""
    shape_case(metric, kind, 256, 8, n, 16, expect="none" if n < 256 else "served")


@pytest.mark.parametrize("metric,kind", KINDS)
@pytest.mark.parametrize("nprobe,nlist,open_", [(16, 128, True), (16, 127, False), (128, 576, True), (128, 575, False), (129, 1024, False)])
def test_gate_on_nlist_and_nprobe(metric, kind, nprobe, nlist, open_):
    """nlist >= 4 nprobe + 64 on both sides, and nprobe <= 128.  (Rankings longer than 128 are sorted, and a call of 20 queries or more
    leaves runs of equal distances in centroid-number order unless coarse_ties = 1 asks for the reference's heap: the oracle's order is
    promised with that option, so the nprobe = 129 case sets it.)"""
    picked, _, _ = shape_case(metric, kind, nlist, nprobe, 256, 16, expect="served" if open_ else "none",
                              options=(("coarse_ties", 1),) if nprobe > 128 else ())
    assert all((p > 0) == open_ for p in picked.values()), picked


@pytest.mark.parametrize("metric,kind", KINDS)
@pytest.mark.parametrize("d", [4, 30, 36, 60, 68, 124, 128, 132, 200, 960])
def test_d_edges(metric, kind, d):
    """K chunks of 32 in coarse_gemm16_kernel and the 64-element body of coarse_pick_kernel's recomputation with its remainder
    (e + 60 < dpad).  The handle pads rows with zeros to dpad = a multiple of four and hands the kernels dpad for d, so d = 30 runs as
    32: one whole chunk whose last two elements are the padding's zeros, which must change neither the fp16 product nor the order of
    the four exact sums -- no guard cuts inside a float4.  The guard k0 + 4 c < d cuts a chunk at d = 4, 36, 60, 68, 124, 132, 200 (dpad
    % 32 != 0); 128 and 960 end on a chunk; the recomputation's body runs 0 times (d <= 60), once with a remainder (68, 124), exactly
    (128), and 15 times (960)."""
    shape_case(metric, kind, 128, 8, 256, d)


# ------------------------------------------------------------------------------------------ 2. the bound, where rounding is coherent
@pytest.mark.parametrize("metric,d,nlist,nprobe,W", cp.BOUND_CASES)
def test_bound_where_rounding_is_coherent(metric, d, nlist, nprobe, W):
    """Operands that all round the same way within a family: the approximate distances are off by half of eps, and a query's distances
    to the two families of centroids are displaced against each other.  With the fp32 form's constant behind the fp16 product, at
    least 10 % of these queries (15 % to 98 % in the model) lose a member of their true top-nprobe; with exact_float_constant none
    does.  (An engine built with that mutation fails all six cases: 117 to 249 of the 256 rankings wrong.)  A widening of 1 eps in
    place of 2 would still pass on this data (the model: lost_one_eps = 0).
    Then the same data with the centroids multiplied by 2^-20 and the queries by 2^18: the same rounding pattern with the scale
    exponents at the other end of what half_scale_of accepts.  (For L2 that makes every distance of a query equal in fp32 -- |c| is
    below half a unit in the last place of x -- so that call checks the all-flagged path instead; L2 also runs with both sides
    multiplied by 2^-20, which keeps the distances apart.)"""
    from oracle import pyoracle
    from auncel_amd import capi
    cen, xq, _ = cp.coherent(d, nlist, cp.BOUND_N, W)
    n = len(xq)
    top = pyoracle.knn(metric, xq, cen, nprobe)[1]
    r = cp.bound_report(metric, xq, cen, nprobe, top=top)
    print(r)
    assert r["lost_fp32"] >= 0.1 * n and r["lost_unwidened"] >= 0.1 * n and r["lost"] == 0 and r["most"] <= cp.PICK_CAP
    tag = f"coherent metric={metric} d={d} nlist={nlist} nprobe={nprobe} W={W}"
    h = capi.Handle(d, nlist, metric, 0)
    _, a, _ = run_forms(metric, xq, cen, nprobe, "served", tag, h=h)
    assert a >= n // 2  # the kernel, not the fallback, answered
    scaled = [(2.0 ** -20, 2.0 ** 18)] + ([(2.0 ** -20, 2.0 ** -20)] if metric == 1 else [])
    for cs, qs in scaled:
        c2, x2 = cen * np.float32(cs), xq * np.float32(qs)
        _, a2, _ = run_forms(metric, x2, c2, nprobe, "bounds", f"{tag} centroids * 2^{int(np.log2(cs))} queries * 2^{int(np.log2(qs))}", h=h)
        assert a2 == a or (metric == 1 and cs != qs)  # (powers of two: the reference meets the same ties)
    h.close()


# ------------------------------------------------------------------------------------------ 3. the candidate cap
def test_more_candidates_than_the_cap():
    """L2 distances that are tiny beside the norms: all 4096 centroids lie under the widened threshold of every query, the guarded
    write (slot < PICK_CAP) drops three quarters of them and C > PICK_CAP flags every ranking -- n = 259 flagged rankings, padded to
    264.  (The fp32 form's eps is three orders smaller and still spans most of these distances: 3554 candidates at the least in the
    model, so it flags every ranking too.)"""
    nlist, nprobe, n = cp.CAP_OVER
    cen, xq, _ = cp.coherent(cp.CAP_D, nlist, n, cp.CAP_W)
    r = cp.bound_report(1, xq, cen, nprobe)
    assert r["fewest_at_first_stop"] >= 2 * cp.PICK_CAP and n % 8 != 0
    assert cp.fewest_candidates_fp32_form(1, xq, cen, nprobe) >= 2 * cp.PICK_CAP
    run_forms(1, xq, cen, nprobe, "none", "over the cap")


def test_exactly_as_many_candidates_as_the_cap():
    """the same data with nlist = 1024: every centroid is a candidate, C == PICK_CAP -- not flagged, a full 1024-slot sort.  (Such data
    has exactly equal fp32 distances: the bounds are asserted, no share.)"""
    nlist, nprobe, n = cp.CAP_AT
    cen, xq, _ = cp.coherent(cp.CAP_D, nlist, n, cp.CAP_W)
    r = cp.bound_report(1, xq, cen, nprobe)
    assert r["fewest_at_first_stop"] == r["most"] == nlist == cp.PICK_CAP
    run_forms(1, xq, cen, nprobe, "bounds", "at the cap")


# ------------------------------------------------------------------------------------------ 4. the flagged list
@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("n", [257, 263])
def test_every_ranking_flagged_through_ties(metric, n):
    """every centroid has a twin, nprobe = 1: the best two distances of every query are equal, every ranking is flagged; the list of n
    is padded to a multiple of eight with 7 / 1 copies of its first entry"""
    cen, xq = cp.near_centroids("bytes", metric, 256, n, 16)
    cen = cen.copy()
    cen[1::2] = cen[0::2]
    run_forms(metric, xq, cen, 1, "none", f"twins metric={metric} n={n}")


def test_exactly_one_ranking_flagged():
    """one query of 1e20s: its L2 distances overflow to +inf, the fp32 form flags it alone -- the list of one is padded with seven
    copies, which are ranked and scattered onto the same row; the rows around it must stay the picked path's.  Under the fp16 form
    the queries have no usable scale (2^66 beside 1): every ranking is flagged."""
    cen, xq = cp.near_centroids("float", 1, 256, 256, 16)
    xq = xq.copy()
    xq[100] = 1e20
    picked, a, b = run_forms(1, xq, cen, 8, {2: "none", 1: "bounds"}, "one flagged")
    assert a == b == len(xq) - 1  # (the reference excuses no other query: Gaussian data, no equal distances)
    assert picked[1] == len(xq) - 1


@pytest.mark.parametrize("metric,kind", KINDS)
def test_an_all_zero_query(metric, kind):
    """IP: eps = 0 and every approximate and exact distance of the query is equal (flagged); L2: its distances are the centroids' norms.
    A zero row is left out of the rule for one scale per matrix."""
    cen, xq = cp.near_centroids(kind, metric, 256, 256, 16)
    xq = xq.copy()
    xq[5] = 0
    run_forms(metric, xq, cen, 8, "served", f"zero query {kind} metric={metric}")


# ------------------------------------------------------------------------------------------ 5. through a search
@pytest.mark.parametrize("metric", [1, 0])
def test_the_ranking_reaches_the_list_scan(metric):
    """search and range_search with their own coarse ranking over the bound-edge centroids: results and statistics are the oracle's
    over the oracle's ranking"""
    from auncel_amd import capi
    from oracle import pyoracle
    d, nlist, nprobe, k = 64, 1024, 16, 10
    cen, xq, xb = cp.coherent(d, nlist, cp.BOUND_N, 128 if metric == 0 else 1024, nb=4096)
    assign = pyoracle.knn(metric, xb, cen, 1)[1][:, 0]
    lists = pyoracle.Lists(metric, cen, xb, assign)
    od, ok = pyoracle.knn(metric, xq, cen, nprobe)
    eD, eI, est = pyoracle.search_preassigned(lists, xq, k, ok, od)
    h = capi.Handle(d, nlist, metric, 0)
    h.set_centroids(cen)
    h.set_lists_from_assign(xb, assign)
    h.stats(reset=True)
    D, I = h.search(xq, k, nprobe)
    assert h.last_coarse_pick() > 0
    assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD))
    st = h.stats()
    assert [st["nlist"], st["ndis"], st["nheap_updates"]] == list(est)
    # range search around the median of the first distances, as test_gpu_random.py chooses it
    fD = pyoracle.search_preassigned(lists, xq, 1, ok, od)[0]
    fin = fD[np.isfinite(fD) & (np.abs(fD) < 1e37)]
    radius = float(np.median(fin)) * (1.5 if metric == 1 else 0.7)
    elims, elab, edis, est = pyoracle.range_search_preassigned(lists, xq, radius, ok)
    assert 0 < elims[-1]
    h.stats(reset=True)
    lims, lab, dis = h.range_search(xq, radius, nprobe)
    assert h.last_coarse_pick() > 0
    assert np.array_equal(lims, elims) and np.array_equal(lab, elab) and np.array_equal(bits(dis), bits(edis))
    st = h.stats()
    assert [st["nlist"], st["ndis"]] == list(est)
    h.close()
