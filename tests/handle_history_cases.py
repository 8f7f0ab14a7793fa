"""Worlds, query sets and expected values of test_gpu_handle_history.py.  Every expected value comes from oracle.pyoracle over lists
built here; nothing is taken from the engine.

The world: 32 lists, sixteen "small" ones (0 .. 40 vectors, one of them empty) and sixteen "big" ones (1500 .. 4000 vectors, no
length a multiple of 64), ~45 000 vectors.  The small lists' centroids sit around one point and the big lists' around another, so
that a query drawn next to a small list also RANKS the small lists first under L2 (the ticket sequence lets the engine rank).  The
query sets of one world share n, k and nprobe -- the engine's hint signature -- and differ in the work a round plans for them."""
import functools

import numpy as np

NLIST, NSMALL, N, NPROBE, K = 32, 16, 160, 8, 10
SMALL_SIZES = [0, 1, 7, 40, 33, 12, 25, 3, 38, 17, 29, 9, 21, 36, 5, 14]
BIG_SIZES = [1537, 3999, 2050, 3333, 2817, 2921, 3601, 2499, 3075, 1666, 2945, 3777, 2111, 3201, 2689, 2493]
assert all(v % 64 for v in BIG_SIZES) and min(SMALL_SIZES) == 0 and 44000 < sum(SMALL_SIZES + BIG_SIZES) < 46000
KINDS = {"bytes": 2, "smallint": 1, "float": 0}  # kind: the arithmetic the list scan must choose (amd_ivf_scan_arith)
FLT_MAX = np.float32(3.4028234663852886e38)
WIDE_NPROBE = 72  # more probes a query than the keep-bit kernel's grid is sized for before any history (64)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _draw(rs, kind, centres, rows):
    """vectors around `centres[rows]` in the value range of the kind"""
    d = centres.shape[1]
    if kind == "bytes":
        return np.clip(centres[rows] + rs.randint(-25, 26, size=(len(rows), d)), 0, 255).astype(np.float32)
    if kind == "smallint":
        return (centres[rows] + rs.randint(-8, 9, size=(len(rows), d))).astype(np.float32)
    return (centres[rows] + 0.3 * rs.randn(len(rows), d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def world(kind, d, metric):
    rs = np.random.RandomState(9100 + 100 * sorted(KINDS).index(kind) + 2 * d + metric)
    sizes = np.array(SMALL_SIZES + BIG_SIZES)
    if kind == "bytes":
        cen = np.concatenate([rs.randint(35, 90, size=(NSMALL, d)), rs.randint(160, 215, size=(NLIST - NSMALL, d))]).astype(np.float32)
    elif kind == "smallint":
        cen = np.concatenate([rs.randint(-30, -9, size=(NSMALL, d)), rs.randint(10, 31, size=(NLIST - NSMALL, d))]).astype(np.float32)
    else:  # (random reals: no two coarse distances of a query are equal)
        cen = np.concatenate([-1.5 + rs.randn(NSMALL, d), 1.5 + rs.randn(NLIST - NSMALL, d)]).astype(np.float32)
    assign = np.repeat(np.arange(NLIST), sizes)
    assign = assign[rs.permutation(len(assign))]
    xb = _draw(rs, kind, cen, assign)
    _freeze(cen, assign, xb, sizes)
    return dict(kind=kind, d=d, metric=metric, cen=cen, assign=assign, xb=xb, sizes=sizes, arith=KINDS[kind])


def spread_lists(n):
    """(n, 2) list numbers, -1 where a query has no second one: no list is probed by more than 8 queries (n a multiple of 32, <= 256)"""
    assert n % NLIST == 0 and n // NLIST <= 8
    i = np.arange(n)
    second = np.where(i < (8 - n // NLIST) * NLIST, (7 * i + 3) % NLIST, -1)  # (6 i + 3 is odd: never the first list again)
    out = np.stack([i % NLIST, second], axis=1)
    counts = np.bincount(out[out >= 0], minlength=NLIST)
    assert counts.max() <= 8 and counts.min() >= 1
    return out


@functools.lru_cache(maxsize=None)
def query_set(kind, d, metric, name, n=N, nprobe=NPROBE):
    """-> (xq, keys, coarse_dis): the probed lists are chosen here (preassigned keys), ordered as the reference's ranking orders
    them, padded with -1 as its heap pads; the query rows lie next to one of the lists they probe"""
    from oracle import pyoracle
    w = world(kind, d, metric)
    rs = np.random.RandomState(9300 + sum(map(ord, name)) + n + 3 * d + metric)
    if name in ("light", "light2"):
        chosen = np.stack([rs.choice(NSMALL, NPROBE, replace=False) for _ in range(n)])
    elif name in ("heavy", "wide"):
        chosen = np.stack([NSMALL + rs.choice(NLIST - NSMALL, NPROBE, replace=False) for _ in range(n)])
    elif name == "spread":
        chosen = spread_lists(n)
    else:
        assert name == "crowd"
        chosen = np.tile(np.arange(NSMALL, NSMALL + NPROBE), (n, 1))
    xq = _draw(rs, kind, w["cen"], chosen[:, 0])
    rank_d, rank_k = pyoracle.knn(metric, xq, w["cen"], NLIST)
    width = WIDE_NPROBE if name == "wide" else nprobe
    keys = np.full((n, width), -1, np.int64)
    dis = np.full((n, width), FLT_MAX if metric == 1 else -FLT_MAX, np.float32)
    for i in range(n):
        m = np.isin(rank_k[i], chosen[i][chosen[i] >= 0])
        c = int(m.sum())
        keys[i, :c], dis[i, :c] = rank_k[i][m], rank_d[i][m]
    if metric == 1 and name in ("light", "light2", "heavy"):
        # the geometry the ticket sequence relies on: ranked by the engine, these queries probe small (big) lists only
        top = rank_k[:, :NPROBE]
        assert (top < NSMALL).all() if name != "heavy" else (top >= NSMALL).all()
    _freeze(xq, keys, dis)
    return xq, keys, dis


def oracle_lists(w, extra=None, member=None):
    """the oracle's lists of a world: `extra` = (rows, ids, list numbers) appended as amd_ivf_add appends them, `member` = a boolean
    per database vector (an id selector: the members of every list, in order)"""
    from oracle import pyoracle
    xb, assign, ids = w["xb"], w["assign"], np.arange(len(w["xb"]), dtype=np.int64)
    if member is not None:
        assign = np.where(member, assign, -1)
    if extra is not None:
        xb, ids, assign = np.concatenate([xb, extra[0]]), np.concatenate([ids, extra[1]]), np.concatenate([assign, extra[2]])
    return pyoracle.Lists(w["metric"], w["cen"], xb, assign, ids)


@functools.lru_cache(maxsize=None)
def expected(kind, d, metric, name, n=N, store_pairs=False, max_codes=0):
    """the oracle's (D, I, stats) of a query set over the world's lists"""
    from oracle import pyoracle
    xq, keys, dis = query_set(kind, d, metric, name, n)
    D, I, st = pyoracle.search_preassigned(oracle_lists(world(kind, d, metric)), xq, K, keys, dis, store_pairs=store_pairs, max_codes=max_codes)
    _freeze(D, I, st)
    return D, I, st


def selector_members(w, name):
    """a boolean per database vector: "sparse" keeps one id in fifty, "dense" nine in ten"""
    rs = np.random.RandomState(9500 + len(name))
    return rs.rand(len(w["xb"])) < (0.02 if name == "sparse" else 0.9)


@functools.lru_cache(maxsize=None)
def expected_selected(kind, d, metric, name, sel_name):
    from oracle import pyoracle
    w = world(kind, d, metric)
    xq, keys, dis = query_set(kind, d, metric, name)
    D, I, st = pyoracle.search_preassigned(oracle_lists(w, member=selector_members(w, sel_name)), xq, K, keys, dis)
    _freeze(D, I, st)
    return D, I, st


@functools.lru_cache(maxsize=None)
def growth(kind, d, metric):
    """rows that make every small list about fifty times as long: (rows, ids, list numbers), list by list"""
    w = world(kind, d, metric)
    rs = np.random.RandomState(9600 + d + metric)
    lists = np.repeat(np.arange(NSMALL), [1200 + 37 * l for l in range(NSMALL)])
    rows = _draw(rs, kind, w["cen"], lists)
    ids = 100000 + np.arange(len(lists), dtype=np.int64)
    _freeze(rows, ids, lists)
    return rows, ids, lists


@functools.lru_cache(maxsize=None)
def expected_grown(kind, d, metric, name):
    from oracle import pyoracle
    w = world(kind, d, metric)
    xq, keys, dis = query_set(kind, d, metric, name)
    D, I, st = pyoracle.search_preassigned(oracle_lists(w, extra=growth(kind, d, metric)), xq, K, keys, dis)
    _freeze(D, I, st)
    return D, I, st


@functools.lru_cache(maxsize=None)
def expected_ranked(kind, d, metric, names):
    """the ticket sequence: the query sets `names` one after the other as the resident set, ranked by the reference's coarse
    quantizer -> (all rows, [(D, I) of every set])"""
    from oracle import pyoracle
    w = world(kind, d, metric)
    xs = [query_set(kind, d, metric, nm)[0] for nm in names]
    out = []
    for x in xs:
        cd, ck = pyoracle.knn(metric, x, w["cen"], NPROBE)
        D, I, _ = pyoracle.search_preassigned(oracle_lists(w), x, K, ck, cd)
        _freeze(D, I)
        out.append((D, I))
    allx = np.concatenate(xs)
    _freeze(allx)
    return allx, out


# ---- the adaptive sequence ------------------------------------------------------------------------------------------------------------
A_NLIST, A_N, A_K, A_NB = 64, 160, 10, 12000


@functools.lru_cache(maxsize=None)
def adaptive_world(kind, d=32):
    """clustered data under L2, lists by the reference's assignment, a tuner as tests/test_gpu_random_adaptive.py draws it"""
    from oracle import pyoracle
    rs = np.random.RandomState(9700 + sorted(KINDS).index(kind))
    nblobs = A_NLIST // 2
    centres = rs.rand(nblobs, d) * 160.0

    def draw(n, sigma=1.0, between=False):
        c = centres[rs.randint(0, nblobs, n)]
        if between:  # half way between two clusters: many lists are about as near as the nearest
            c = 0.5 * (c + centres[rs.randint(0, nblobs, n)])
        if kind == "bytes":
            return np.floor(np.clip(c + rs.randn(n, d) * 30.0 * sigma, 0, 255)).astype(np.float32)
        return (c / 40.0 + rs.randn(n, d) * 0.8 * sigma).astype(np.float32)

    xb = draw(A_NB)
    cen = (xb[rs.choice(A_NB, A_NLIST, replace=False)] + rs.randn(A_NLIST, d) * 1e-3).astype(np.float32)  # no exact coarse ties
    _, a = pyoracle.knn(1, xb, cen, 1, nthreads=8)
    assign = a[:, 0].copy()
    ntr = 1
    while (1 << ntr) <= A_NLIST // 8:
        ntr += 1
    traces = []
    for _ in range(ntr):
        m = int(rs.randint(20, 60))
        x = np.sort(rs.rand(m) * 25.0).astype(np.float32)
        x += np.arange(m, dtype=np.float32) * 1e-3  # strictly ascending
        traces.append((x, (0.5 + rs.rand(m) * 2.5).astype(np.float32), (rs.rand(m) * 0.5).astype(np.float32)))
    easy = xb[rs.choice(A_NB, A_N, replace=False)].copy()
    easy2 = xb[rs.choice(A_NB, A_N, replace=False)].copy()
    hard = draw(A_N, between=True)
    xq = np.concatenate([easy, hard, easy2])
    req = np.concatenate([np.full(A_N, 0.5), np.full(A_N, 0.99), np.full(A_N, 0.5)]).astype(np.float32)
    _freeze(xb, cen, assign, xq, req)
    return dict(kind=kind, d=d, metric=1, xb=xb, cen=cen, assign=assign, traces=traces, xq=xq, req=req, arith=KINDS[kind])


A_QUERY_TOPK, A_MULTIPLER, A_STD_M = 10, 1.3, 1.0


@functools.lru_cache(maxsize=None)
def expected_adaptive(kind, step):
    """the oracle's tune branch over resident rows [step * A_N, (step + 1) * A_N) -> (D, I, stats, my_nprobe, t_recalls)"""
    from oracle import pyoracle
    w = adaptive_world(kind)
    lists = pyoracle.Lists(1, w["cen"], w["xb"], w["assign"])
    x = w["xq"][step * A_N:(step + 1) * A_N]
    cd, ck = pyoracle.knn(1, x, w["cen"], A_NLIST, nthreads=8)
    gtD, _ = pyoracle.knn(1, w["xq"], w["xb"], A_K, nthreads=8)
    tun = pyoracle.Tuner(pyoracle.interdis(1, w["cen"]), w["traces"], A_K, 3 * A_N)
    stt = tun.struct(A_QUERY_TOPK, w["req"], A_MULTIPLER, A_STD_M, gt_D=gtD, profile=False)
    D, I, st = pyoracle.search_preassigned(lists, x, A_K, ck, cd, tuner=stt, offset=step * A_N, nthreads=1)
    my_np = tun.my_nprobe[step * A_N:(step + 1) * A_N].astype(np.int64)
    t_rec = tun.t_recalls[step * A_N:(step + 1) * A_N].copy()
    _freeze(D, I, st, my_np, t_rec, gtD)
    return D, I, st, my_np, t_rec, gtD
