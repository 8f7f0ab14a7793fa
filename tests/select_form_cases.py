"""Worlds, queries and expected values of test_gpu_select_forms.py; their preconditions are asserted by test_select_form_cases_cpu.py.
Every expected value comes from oracle.pyoracle (Lists, knn, search_preassigned, Tuner, interdis) over lists built here; nothing is
taken from the engine.

What a query's selection form depends on is k (ivf_select.hip: launch_select_sorted, launch_replay, launch_tie_fix), so the worlds
are small and fixed and the tests walk K_FIXED over them:

  "ties"      integer grid rows (values 0 .. 3, d = 8) drawn from a pool of 300 base rows: equal candidate distances are the rule.  Half
              of the pool's rows occur once, the other half about forty times each, and half of the queries are rows that occur once:
              such a query's best candidate is alone at its distance, so that at small k the k best can be all different while a
              copy of the k-th value was admitted and evicted -- the one case in which only the `amb` note of select_sorted_kernel
              sends a query through the tie replay.
  "distinct"  random reals, d = 30: no two candidate distances of a query are equal.
  selected    "ties" under a membership vector that keeps 40 % of every list but one, which loses all its members.
  adaptive    handle_history_cases.adaptive_world("bytes") with 70 of its queries ("bytes"), integer grid rows with span 12 ("grid":
              equal candidate distances, and equal coarse distances, under the stop rule), unit-norm rows under the inner product
              ("unit").

The tie replay.  select_sorted_kernel hands a query to tie_fix_kernel when the heap's history can decide an id or an output order:
(a) two of its final k values are equal, or (b) its final worst value equals a value that was evicted while an equal one stayed (an
edge tie that the admissions split).  `replay_counts` restates both from the oracle's candidates in the reference's scan order
(probe by probe, list position by list position; a candidate is admitted iff it is strictly better than the worst of the k) and
returns, per k, how many queries (b) holds for, how many (a) or (b), and how many (b) but not (a)."""
import bisect
import functools

import numpy as np

import handle_history_cases as hc

K_FIXED = (1, 2, 3, 9, 10, 11, 63, 64, 65, 99, 100, 101, 127, 128, 129, 160)
NLIST, NQ, NPROBE = 16, 70, 6
# ragged: list 0 empty, list 1 shorter than 64, no other length a multiple of 64
SIZES = (0, 37, 411, 523, 289, 350, 477, 391, 333, 451, 402, 365, 498, 310, 571, 592)
NB = sum(SIZES)
assert NB == 6000 and all(v % 64 for v in SIZES[1:])
POOL, ONCE = 300, 150  # base rows of "ties"; the first ONCE of them occur once
DIMS = {"ties": 8, "distinct": 30}
FLT_MAX = hc.FLT_MAX
SELECTED_K = (1, 2, 11, 65, 101, 127, 128, 129)
EACH_K = (65, 128)
TIE_FIX_K = (2, 65, 127, 128)
UP_AND_DOWN_K = (128, 2, 129, 65, 10)
EMPTIED_LIST = 5  # the list whose members the selector drops, all of them
KEEP = 0.4

_freeze = hc._freeze


def _seed(name, metric):
    return 9900 + 10 * sorted(DIMS).index(name) + metric


@functools.lru_cache(maxsize=None)
def world(name, metric):
    """-> dict(d, metric, cen, xb, assign, xq, keys, dis): keys / dis are the oracle's ranking of the centroids, NPROBE entries"""
    from oracle import pyoracle
    rs = np.random.RandomState(_seed(name, metric))
    d = DIMS[name]
    if name == "ties":
        pool = rs.randint(0, 4, size=(POOL, d)).astype(np.float32)
        rows = np.concatenate([np.arange(ONCE), ONCE + rs.randint(0, POOL - ONCE, size=NB - ONCE)])
        xb = pool[rows[rs.permutation(NB)]]
        xq = np.concatenate([pool[rs.choice(ONCE, NQ // 2, replace=False)], rs.randint(0, 4, size=(NQ - NQ // 2, d)).astype(np.float32)])
        xq = xq[rs.permutation(NQ)]
        cen = rs.randint(0, 4, size=(NLIST, d)).astype(np.float32)
    else:
        xb = rs.randn(NB, d).astype(np.float32)
        xq = rs.randn(NQ, d).astype(np.float32)
        cen = rs.randn(NLIST, d).astype(np.float32)
    assign = np.repeat(np.arange(NLIST), SIZES)
    assign = assign[rs.permutation(NB)]
    dis, keys = pyoracle.knn(metric, xq, cen, NPROBE)
    if name == "distinct":
        # A few thousand fp32 distances of one query do collide now and then (a birthday's worth): the rows behind the later of two
        # equal distances are drawn again until no query has any.
        order = np.argsort(assign, kind="stable")
        off = np.concatenate([[0], np.cumsum(SIZES)])
        for _ in range(50):
            D, I, _ = pyoracle.search_preassigned(pyoracle.Lists(metric, cen, xb, assign), xq, NB + 1, keys, dis, store_pairs=True)
            again = set()
            for q in range(NQ):
                n = int((I[q] >= 0).sum())
                same = np.nonzero(D[q, 1:n].view(np.uint32) == D[q, :n - 1].view(np.uint32))[0] + 1
                again.update(order[off[I[q, same] >> 32] + (I[q, same] & 0xffffffff)].tolist())
            if not again:
                break
            xb[sorted(again)] = rs.randn(len(again), d).astype(np.float32)
        else:
            raise AssertionError("equal candidate distances remain")
    _freeze(cen, xb, assign, xq, keys, dis)
    return dict(name=name, d=d, metric=metric, cen=cen, xb=xb, assign=assign, xq=xq, keys=keys, dis=dis)


@functools.lru_cache(maxsize=None)
def members(metric):
    """a boolean per row of "ties": KEEP of every list (rounded), none of list EMPTIED_LIST"""
    w = world("ties", metric)
    rs = np.random.RandomState(9950 + metric)
    m = np.zeros(NB, bool)
    for l in range(NLIST):
        rows = np.nonzero(w["assign"] == l)[0]
        if l != EMPTIED_LIST and len(rows):
            m[rs.choice(rows, int(round(KEEP * len(rows))), replace=False)] = True
    _freeze(m)
    return m


def lists_of(w, member=None):
    from oracle import pyoracle
    assign = w["assign"] if member is None else np.where(member, w["assign"], -1)
    return pyoracle.Lists(w["metric"], w["cen"], w["xb"], assign)


@functools.lru_cache(maxsize=None)
def expected(name, metric, k, store_pairs=False, selected=False):
    """the oracle's (D, I, stats) of the world's queries at this k; selected: over the members' lists (`complement`: the others')"""
    from oracle import pyoracle
    w = world(name, metric)
    member = None
    if selected:
        member = members(metric) if selected != "complement" else ~members(metric)
    D, I, st = pyoracle.search_preassigned(lists_of(w, member), w["xq"], k, w["keys"], w["dis"], store_pairs=store_pairs)
    _freeze(D, I, st)
    return D, I, st


@functools.lru_cache(maxsize=None)
def candidates(name, metric):
    """per query, the distances of its probed candidates in the reference's scan order (a list of float32 arrays): the oracle's
    search with a k no query fills and (list, position) pairs as labels -- every candidate enters such a heap"""
    from oracle import pyoracle
    w = world(name, metric)
    kbig = NB + 1
    D, I, _ = pyoracle.search_preassigned(lists_of(w), w["xq"], kbig, w["keys"], w["dis"], store_pairs=True)
    out = []
    for q in range(NQ):
        n = int((I[q] >= 0).sum())
        lst, pos = I[q, :n] >> 32, I[q, :n] & 0xffffffff
        rank = np.full(NLIST, -1, np.int64)
        rank[w["keys"][q]] = np.arange(NPROBE)
        assert (rank[lst] >= 0).all() and n == sum(SIZES[l] for l in w["keys"][q])
        a = D[q, :n][np.lexsort((pos, rank[lst]))].copy()
        _freeze(a)
        out.append(a)
    return out


def order_keys(vals, metric):
    """smaller = better (negation is exact)"""
    return vals if metric == 1 else -vals


def replay_one(keys, k):
    """the sorted array's admissions over one query's candidates (order keys, scan order) -> (equal values among the final k, final
    worst equals an evicted value of which a copy stayed)"""
    arr, amb = [], None
    for v in keys.tolist():
        if len(arr) < k:  # (the entries that go are empty ones: nothing to note)
            bisect.insort_right(arr, v)
        elif v < arr[-1]:
            evicted = arr.pop()
            bisect.insort_right(arr, v)
            if arr[-1] == evicted:
                amb = evicted
    dup = any(a == b for a, b in zip(arr, arr[1:]))
    split = len(arr) == k and amb is not None and arr[-1] == amb
    return dup, split


@functools.lru_cache(maxsize=None)
def replay_counts(name, metric, k):
    """-> (queries whose edge tie the admissions split, queries that need the replay, queries that need it for the split alone)"""
    res = [replay_one(order_keys(c, metric), k) for c in candidates(name, metric)]
    return sum(s for _, s in res), sum(d or s for d, s in res), sum(s and not d for d, s in res)


@functools.lru_cache(maxsize=None)
def edge_tie_counts(name, metric, k):
    """-> (queries with a (k + 1)-th candidate, those of them whose k-th and (k + 1)-th best distances are bit-equal)"""
    have = tied = 0
    for c in candidates(name, metric):
        if k < len(c):
            s = np.sort(c).view(np.uint32)
            s = s if metric == 1 else s[::-1]
            have += 1
            tied += int(s[k - 1] == s[k])
    return have, tied


def held_to_tie_condition(metric):
    """the k of K_FIXED at which at least half of the queries have a tie across the heap's edge"""
    return tuple(k for k in K_FIXED if 2 * edge_tie_counts("ties", metric, k)[1] >= NQ)


# ---- adaptive worlds ------------------------------------------------------------------------------------------------------------------
A_NLIST, A_NB, A_N, A_D = hc.A_NLIST, hc.A_NB, 70, 32
A_CASES = ((64, 1), (65, 10), (65, 11), (96, 96), (127, 11), (127, 127), (128, 10), (128, 128), (129, 11))
A_IP_CASE = (65, 11)
A_MULTIPLER, A_STD_M = hc.A_MULTIPLER, hc.A_STD_M
A_VARIANTS = ("bytes", "grid")


def _traces(rs, nlist):
    ntr = 1
    while (1 << ntr) <= nlist // 8:
        ntr += 1
    traces = []
    for _ in range(ntr):
        m = int(rs.randint(20, 60))
        x = np.sort(rs.rand(m) * 25.0).astype(np.float32)
        x += np.arange(m, dtype=np.float32) * 1e-3  # strictly ascending
        traces.append((x, (0.5 + rs.rand(m) * 2.5).astype(np.float32), (rs.rand(m) * 0.5).astype(np.float32)))
    return traces


@functools.lru_cache(maxsize=None)
def adaptive_world(variant):
    """-> dict(d, metric, xb, cen, assign, traces, xq, req)"""
    from oracle import pyoracle
    rs = np.random.RandomState(9970 + len(variant))
    req = rs.choice([0.5, 0.9, 0.99], size=A_N).astype(np.float32)
    if variant == "bytes":
        w = hc.adaptive_world("bytes", A_D)
        # stored vectors and points half way between clusters, as its "easy" and "hard" ranges
        xq = np.concatenate([w["xq"][:24], w["xq"][hc.A_N:hc.A_N + 24], w["xq"][2 * hc.A_N:2 * hc.A_N + 22]])
        out = dict(d=A_D, metric=1, xb=w["xb"], cen=w["cen"], assign=w["assign"], traces=w["traces"])
    elif variant == "grid":
        xb = rs.randint(0, 12, size=(A_NB, A_D)).astype(np.float32)
        xq = rs.randint(0, 12, size=(A_N, A_D)).astype(np.float32)
        cen = xb[rs.choice(A_NB, A_NLIST, replace=False)].copy()
        _, a = pyoracle.knn(1, xb, cen, 1, nthreads=8)
        out = dict(d=A_D, metric=1, xb=xb, cen=cen, assign=a[:, 0].copy(), traces=_traces(rs, A_NLIST))
    else:
        assert variant == "unit"
        nblobs = A_NLIST // 2
        centres = rs.rand(nblobs, A_D) * 160.0

        def draw(n):
            x = centres[rs.randint(0, nblobs, n)] / 160.0 - 0.5 + rs.randn(n, A_D) * 0.15
            return (x / np.linalg.norm(x, axis=1, keepdims=True) * 0.9).astype(np.float32)

        xb, xq = draw(A_NB), draw(A_N)
        cen = (xb[rs.choice(A_NB, A_NLIST, replace=False)] + rs.randn(A_NLIST, A_D) * 1e-3).astype(np.float32)
        _, a = pyoracle.knn(0, xb, cen, 1, nthreads=8)
        assign = a[:, 0].copy()
        # the reference's inner-product rule reads the max_topk-th entry of every list it probes: rows of the longest list move to
        # the lists shorter than that
        K = A_IP_CASE[0]
        for l in range(A_NLIST):
            short = K - int((assign == l).sum())
            if short > 0:
                big = int(np.bincount(assign, minlength=A_NLIST).argmax())
                assign[np.nonzero(assign == big)[0][-short:]] = l
        assert np.bincount(assign, minlength=A_NLIST).min() >= K
        out = dict(d=A_D, metric=0, xb=xb, cen=cen, assign=assign, traces=_traces(rs, A_NLIST))
    out.update(xq=np.ascontiguousarray(xq), req=req, variant=variant)
    _freeze(out["xb"], out["cen"], out["assign"], out["xq"], out["req"])
    return out


@functools.lru_cache(maxsize=None)
def coarse(variant):
    from oracle import pyoracle
    w = adaptive_world(variant)
    cd, ck = pyoracle.knn(w["metric"], w["xq"], w["cen"], A_NLIST, nthreads=8)
    _freeze(cd, ck)
    return cd, ck


@functools.lru_cache(maxsize=None)
def expected_adaptive(variant, K, query_topk):
    """the oracle's tune branch -> (D, I, stats, my_nprobe, t_recalls, gt_D); raises what the oracle raises"""
    from oracle import pyoracle
    w = adaptive_world(variant)
    lists = pyoracle.Lists(w["metric"], w["cen"], w["xb"], w["assign"])
    cd, ck = coarse(variant)
    gtD, _ = pyoracle.knn(w["metric"], w["xq"], w["xb"], K, nthreads=8)
    tun = pyoracle.Tuner(pyoracle.interdis(w["metric"], w["cen"]), w["traces"], K, A_N)
    stt = tun.struct(query_topk, w["req"], A_MULTIPLER, A_STD_M, gt_D=gtD, profile=False)
    D, I, st = pyoracle.search_preassigned(lists, w["xq"], K, ck, cd, tuner=stt, offset=0, nthreads=1)
    my_np, t_rec = tun.my_nprobe.astype(np.int64), tun.t_recalls.copy()
    _freeze(D, I, st, my_np, t_rec, gtD)
    return D, I, st, my_np, t_rec, gtD


@functools.lru_cache(maxsize=None)
def adaptive_edge_ties(variant, K, query_topk):
    """queries whose K-th and (K + 1)-th best candidates, among the lists they probed before they stopped, are bit-equal: a plain
    search of those lists (the rest of the ranking replaced by the reference's -1 padding) with one more entry"""
    from oracle import pyoracle
    w = adaptive_world(variant)
    my_np = expected_adaptive(variant, K, query_topk)[3]
    cd, ck = coarse(variant)
    keys = np.where(np.arange(A_NLIST)[None, :] < my_np[:, None], ck, -1)
    D, I, _ = pyoracle.search_preassigned(lists_of(w), w["xq"], K + 1, keys, cd)
    return int(((D[:, K - 1].view(np.uint32) == D[:, K].view(np.uint32)) & (I[:, K] >= 0)).sum())
