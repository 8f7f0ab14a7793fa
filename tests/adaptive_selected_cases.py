"""Worlds, selectors and the oracle's answers for the tests of the adaptive rule under an id selector (test_gpu_adaptive_selected.py;
what those tests lean on is asserted without a GPU by test_adaptive_selected_cases_cpu.py).  numpy only; the oracle is passed in by
the caller and the engine is never imported here.

The contract under test: amd_ivf_search_adaptive_selected & co return, bit for bit, what the unselected call returns on the subset of
the same selector, and that is the reference's tuned search_preassigned over the lists with the non-members removed, in order.  Ids are
row numbers (amd_ivf_set_lists_from_assign), so a selector is a boolean mask over the rows and the filtered lists are
oracle.Lists(metric, cen, xb[mask], assign[mask], ids = the rows kept).

World A   nlist 32, d 16, 3000 rows in ragged lists, 48 queries, Kmax 20, query_topk 10, multipler 2, bounds from {0.8, 0.9, 0.95}.
          L2: integer-valued rows (byte codes apply); IP: rows of norm 0.9.
World B   nlist 256, d 32, ~12000 rows, 60 queries, Kmax 20, query_topk 10, multipler 1 (a query stops where it fires, so one can
          stop after its first probe).  Rows are duplicated under other ids -- the selectors keep some copies and drop others, so
          equal distances meet inside the kept set -- and groups of queries read runs of equal coarse distances: L2 over small
          integers (integer distances collide, as in tests/test_gpu_coarse_ties.py), IP over rows of norm 0.9 with twelve centroids
          once more under other list numbers.
The rule runs past the first round (12 probes) for a good share of world B's queries: nlist / 8 = 32."""
import functools
from types import SimpleNamespace

import numpy as np

L2, IP = 1, 0
KMAX, QK = 20, 10
ROUND0 = 12  # probes of an adaptive search's first round (option "round_first")
SELECTORS = ["range_10pct", "mod_3_1", "batch", "everything", "sparse", "few"]
WORLDS = [("A", L2), ("A", IP), ("B", L2), ("B", IP)]
# (kind, a1, a2) of the ABI: SUBSET_ID_RANGE 0, SUBSET_ID_MOD 1, SUBSET_ID_BITS 5, SUBSET_ID_BATCH 6
ID_RANGE, ID_MOD, ID_BITS, ID_BATCH = 0, 1, 5, 6


def ntraces(nlist):
    n = 1
    while (1 << n) <= nlist // 8:
        n += 1
    return n


def make_traces(rs, nlist):
    """as test_gpu_subset.py builds them"""
    traces = []
    for _ in range(ntraces(nlist)):
        n = int(rs.randint(5, 40))
        tx = np.sort(rs.rand(n) * 25.0).astype(np.float32) + np.arange(n, dtype=np.float32) * 1e-3
        traces.append((tx, (0.5 + rs.rand(n) * 2.5).astype(np.float32), (rs.rand(n) * 0.5).astype(np.float32)))
    return traces


def unit(x, scale=0.9):
    return (x / np.linalg.norm(x, axis=1, keepdims=True) * scale).astype(np.float32)


def id_bits(ids, nwords):
    w = np.zeros(nwords, np.uint64)
    ids = np.asarray(ids, np.int64)
    np.bitwise_or.at(w, ids >> 6, np.uint64(1) << (ids & 63).astype(np.uint64))
    return w


SEEDS = {("A", L2): 9001, ("A", IP): 9002, ("B", L2): 9103, ("B", IP): 9104}


@functools.lru_cache(maxsize=None)
def world(name, metric):
    rs = np.random.RandomState(SEEDS[(name, metric)])
    if name == "A":
        nlist, d, nb, nq, mult = 32, 16, 3000, 48, 2.0
        assign = rs.randint(0, nlist, size=nb)
        # ragged: empty lists and long ones.  (Inner product: lists of one size -- the reference converts all Kmax heap values to angles
        # after every probe and throws on the empty heap's sentinel, so a tuned inner-product search needs Kmax members in the first
        # list it probes; under the selectors that leave fewer, the reference throws and the calls under test are refused alike.)
        for a, b in ((1, 0), (5, 4), (6, 4)) if metric == L2 else ():
            assign[assign == a] = b
        if metric == L2:
            cen = rs.randint(10, 200, size=(nlist, d)).astype(np.float32)
            xb = np.clip(cen[assign] + rs.randint(-40, 41, size=(nb, d)), 0, 255).astype(np.float32)
            xq = np.clip(cen[rs.randint(0, nlist, size=nq)] + rs.randint(-40, 41, size=(nq, d)), 0, 255).astype(np.float32)
        else:
            c = rs.rand(nlist, d) - 0.5
            cen = unit(c)
            xb = unit(c[assign] + 0.25 * rs.randn(nb, d))
            xq = unit(c[rs.randint(0, nlist, size=nq)] + 0.25 * rs.randn(nq, d))
        req = rs.choice([0.8, 0.9, 0.95], size=nq).astype(np.float32)
    else:
        nlist, d, nq, mult = 256, 32, 60, 1.0
        nseed = 8000
        if metric == L2:
            # small integers: distances to the centroids are integers below 2^11, so every ranking of 256 holds runs of equal ones
            # (tests/test_gpu_coarse_ties.py's grid); the queries next to the centroids read them at the head of their rankings
            rows = rs.randint(0, 9, size=(nseed, d)).astype(np.float32)
            cen = rows[rs.choice(nseed, nlist, replace=False)].copy()
            tied = np.arange(nlist)
            qrows = lambda of: np.clip(of + rs.randint(-1, 2, size=of.shape), 0, 8).astype(np.float32)
        else:
            # twelve centroids once more under other list numbers: runs of equal coarse distances for every query, at the head of
            # the rankings of the queries near them
            ncen = nlist - 12
            c = rs.rand(ncen, d) - 0.5
            rows = unit(c[rs.randint(0, ncen, size=nseed)] + 0.35 * rs.randn(nseed, d))
            twins = rs.choice(ncen, 12, replace=False)
            perm = rs.permutation(nlist)
            cen = np.vstack([unit(c), unit(c)[twins]])[perm]
            tied = np.nonzero(np.isin(perm, np.concatenate([twins, np.arange(ncen, nlist)])))[0]
            qrows = lambda of: unit(of + 0.02 * rs.randn(*of.shape))
        # half of the rows once more under another id
        xb = np.vstack([rows, rows[rs.choice(nseed, nseed // 2, replace=False)]])
        xb = xb[rs.permutation(len(xb))]
        nb = len(xb)
        x64, c64 = xb.astype(np.float64), cen.astype(np.float64)
        dist = (c64 * c64).sum(1)[None, :] - 2.0 * (x64 @ c64.T) if metric == L2 else -(x64 @ c64.T)
        near = np.argsort(dist, axis=1, kind="stable")[:, :3]
        assign = near[np.arange(nb), rs.randint(0, 3, size=nb)]  # (one of the three nearest lists: later probes hold neighbours)
        # a third of the queries next to a twinned centroid, the rest next to stored rows
        nt = nq // 3
        xq = np.vstack([qrows(cen[rs.choice(tied, nt)]), qrows(xb[rs.choice(nb, nq - nt, replace=False)])]).astype(np.float32)
        req = rs.choice([0.5, 0.8, 0.9, 0.95, 0.99], size=nq).astype(np.float32)
    traces = make_traces(rs, nlist)
    for a in (cen, assign, xb, xq, req):
        a.setflags(write=False)
    return SimpleNamespace(name=name, metric=metric, nlist=nlist, d=d, nb=len(xb), nq=nq, K=KMAX, qk=QK, mult=mult, std_m=1.0, cen=cen,
                           assign=assign.astype(np.int64), xb=xb, xq=xq, req=req, traces=traces,
                           sizes=np.bincount(assign, minlength=nlist))


@functools.lru_cache(maxsize=None)
def selector(name, metric, sel):
    """-> ((kind, a1, a2, array or None) of the ABI, boolean mask over the rows)"""
    w = world(name, metric)
    rs = np.random.RandomState(77)
    ids = np.arange(w.nb, dtype=np.int64)
    nwords = (w.nb + 63) // 64 + 2
    if sel == "range_10pct":
        a1, a2 = w.nb // 2, w.nb // 2 + w.nb // 10
        return (ID_RANGE, a1, a2, None), (ids >= a1) & (ids < a2)
    if sel == "mod_3_1":
        return (ID_MOD, 3, 1, None), ids % 3 == 1
    if sel == "batch":
        picked = rs.choice(ids, w.nb // 5, replace=False)
        batch = np.concatenate([picked, picked[:20], np.array([w.nb + 5, -3, 10 ** 12])]).astype(np.int64)
        return (ID_BATCH, 0, 0, batch), np.isin(ids, picked)
    if sel == "everything":
        return (ID_RANGE, 0, w.nb, None), np.ones(w.nb, bool)
    if sel == "sparse":
        # the rows of three lists in eight, thinned to a half: nothing is kept in five lists of eight
        mask = np.isin(w.assign % 8, (0, 3, 6)) & (rs.rand(w.nb) < 0.5)
        return (ID_BITS, 0, 0, id_bits(ids[mask], nwords)), mask
    assert sel == "few"
    few = rs.choice(ids, KMAX - 7, replace=False)
    return (ID_BATCH, 0, 0, few.astype(np.int64)), np.isin(ids, few)


_REFERENCE = {}


def reference(oracle, arcos, name, metric, sel, profile=False):
    """the oracle's tuned search over the filtered lists, with the filtered ground truth; computed once and left unchanged"""
    key = (name, metric, sel, profile)
    if key not in _REFERENCE:
        w = world(name, metric)
        _, mask = selector(name, metric, sel)
        kept = np.nonzero(mask)[0].astype(np.int64)
        fb, fa = np.ascontiguousarray(w.xb[mask]), np.ascontiguousarray(w.assign[mask])
        lists = oracle.Lists(metric, w.cen, fb, fa, kept)
        cd, ck = oracle.knn(metric, w.xq, w.cen, w.nlist, nthreads=8)
        gtD, gtI = oracle.knn(metric, w.xq, fb, w.K, nthreads=8) if len(kept) >= w.K else padded_knn(oracle, metric, w.xq, fb, w.K)
        tun = oracle.Tuner(oracle.interdis(metric, w.cen), w.traces, w.K, w.nq, arcos=arcos)
        stt = tun.struct(w.qk, w.req, w.mult, w.std_m, gt_D=gtD, profile=profile)
        D, I, st = oracle.search_preassigned(lists, w.xq, w.K, ck, cd, tuner=stt, offset=0, nthreads=1)
        out = SimpleNamespace(D=D, I=I, my_nprobe=tun.my_nprobe.astype(np.int64).copy(), t_recalls=tun.t_recalls.copy(), ck=ck, cd=cd,
                              gtD=gtD, kept=kept, kept_sizes=np.bincount(fa, minlength=w.nlist), lists=lists)
        for a in (out.D, out.I, out.my_nprobe, out.t_recalls, out.ck, out.cd, out.gtD, out.kept, out.kept_sizes):
            a.setflags(write=False)
        _REFERENCE[key] = out
    return _REFERENCE[key]


def padded_knn(oracle, metric, xq, fb, K):
    """exact k-NN over fewer than K rows: the reference's padding behind what there is"""
    n = len(fb)
    D = np.full((len(xq), K), np.finfo(np.float32).max if metric == L2 else -np.finfo(np.float32).max, np.float32)
    I = np.full((len(xq), K), -1, np.int64)
    if n:
        d, i = oracle.knn(metric, xq, fb, n, nthreads=8)
        D[:, :n], I[:, :n] = d, i
    return D, I


def first_run(cd_row):
    """start of the first run of equal coarse distances in a ranking (its length where there is none)"""
    eq = np.nonzero(cd_row[1:] == cd_row[:-1])[0]
    return int(eq[0]) if len(eq) else len(cd_row)
