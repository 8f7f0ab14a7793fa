"""Case builders shared by test_gpu_shard_tickets.py (the engine's ticketed coarse ranking and preassigned search) and
test_shard_tickets_model_cpu.py (which checks, from the oracle and the goldens alone, that these inputs have the edges the GPU
tests rely on).  Every expected value here comes from the goldens or from oracle.pyoracle, never from the engine."""
import functools

import numpy as np

from util import load_case

FLT_MAX = np.float32(3.4028234663852886e38)

# ---- 1. golden shard cases -------------------------------------------------------------------------------------------------------
GOLDEN_SHARD_CASES = ["fixed_sift_l2", "fixed_gauss_l2_d96", "fixed_deep_ip_d96", "fixed_ragged", "fixed_dups"]
PIPELINED_CASES = ["fixed_sift_l2", "fixed_deep_ip_d96", "fixed_dups"]


def shares(nq, nshard):
    """(start, n) of every shard's share of nq queries: [r nq / N, (r + 1) nq / N), as sharding.run_pipelined's callers cut them"""
    return [(r * nq // nshard, (r + 1) * nq // nshard - r * nq // nshard) for r in range(nshard)]


def shard_assign(assign, nshard, s):
    """the assignment with every vector of a list that shard s does not own dropped: owner(l) = l % nshard, as the goldens were made"""
    a = np.asarray(assign, dtype=np.int64)
    return np.where((a >= 0) & (a % nshard == s), a, -1)


@functools.lru_cache(maxsize=None)
def golden_shard_tables(name):
    """{k: [(D, I) of shard s over the whole query set]} from the oracle over each shard's lists and the golden keys"""
    from oracle import pyoracle
    case, gold = load_case(name)
    out = {}
    for k in case["ks"]:
        tabs = []
        for s in range(case["nshard"]):
            sub = pyoracle.Lists(case["metric"], case["centroids"], case["xb"], shard_assign(gold["assign"], case["nshard"], s))
            D, I, _ = pyoracle.search_preassigned(sub, case["xq"], int(k), gold["coarse_keys_sse"], gold["coarse_dis_sse"])
            D.setflags(write=False), I.setflags(write=False)
            tabs.append((D, I))
        out[int(k)] = tabs
    return out


# ---- 3. slices and shapes --------------------------------------------------------------------------------------------------------
SYNTH_NQ, SYNTH_NLIST, SYNTH_NB = 130, 16, 3000
SYNTH_KINDS = {"bytes": (32, 2), "wideint": (30, 0), "gauss": (96, 0)}  # kind: (d, the arithmetic the list scan must choose)
RANGES = [(0, 1), (0, 130), (129, 1), (63, 2), (64, 66), (5, 0)]
NPROBES = [1, 5, 16, 19]
KS = [1, 10, 100, 200]
EMPTY_SHARD_NSHARD = 3  # shards 0 and 1 own the even and the odd lists, shard 2 owns none
EMPTY_SHARD_RANGE = (63, 2)  # two queries over three shards: one share is empty


def ticket_plan():
    """(start, n, nprobe, k) of every ticket pair (coarse ranking, search): every range with the smallest and the largest nprobe and
    k, every other value of nprobe and k at least once"""
    plan = []
    for start, n in RANGES:
        plan.append((start, n, NPROBES[0], KS[0]))
        plan.append((start, n, NPROBES[-1], KS[-1]))
    plan += [(0, 130, 1, 200), (0, 130, 19, 1), (0, 130, 5, 10), (0, 130, 16, 100), (64, 66, 5, 100), (63, 2, 16, 10), (129, 1, 5, 200),
             (64, 66, 16, 1)]
    return plan


def alternating(plan):
    """the plan ordered so that consecutive tickets alternate between the largest and the smallest shapes (n * nprobe * k)"""
    by_size = sorted(plan, key=lambda t: (t[1] * t[2] * t[3], t))
    out = []
    lo, hi = 0, len(by_size) - 1
    while lo <= hi:
        out.append(by_size[hi])
        if lo < hi:
            out.append(by_size[lo])
        lo, hi = lo + 1, hi - 1
    return out


@functools.lru_cache(maxsize=None)
def synth_case(kind, metric):
    d, arith = SYNTH_KINDS[kind]
    rs = np.random.RandomState(7000 + 10 * sorted(SYNTH_KINDS).index(kind) + metric)
    nb, nq, nlist = SYNTH_NB, SYNTH_NQ, SYNTH_NLIST
    if kind == "bytes":
        xb = rs.randint(0, 256, size=(nb, d)).astype(np.float32)
        xq = rs.randint(0, 256, size=(nq, d)).astype(np.float32)
    elif kind == "wideint":
        xb = rs.randint(-4000, 4001, size=(nb, d)).astype(np.float32)
        xq = rs.randint(-4000, 4001, size=(nq, d)).astype(np.float32)
    else:
        xb = rs.randn(nb, d).astype(np.float32)
        xq = rs.randn(nq, d).astype(np.float32)
    cen = xb[rs.choice(nb, size=nlist, replace=False)].copy()
    if kind == "gauss":
        cen += (rs.randn(*cen.shape) * 0.01).astype(np.float32)
    assign = rs.randint(0, nlist, size=nb)
    assign[assign == 1] = 0  # one list emptied into its neighbour
    for a in (xb, xq, cen, assign):
        a.setflags(write=False)
    return dict(kind=kind, d=d, nlist=nlist, metric=metric, xb=xb, xq=xq, cen=cen, assign=assign, arith=arith)


@functools.lru_cache(maxsize=None)
def synth_lists(kind, metric, nshard=0, shard=0):
    """the oracle's lists of the whole synthetic index (nshard = 0) or of one shard of EMPTY_SHARD_NSHARD"""
    from oracle import pyoracle
    c = synth_case(kind, metric)
    a = c["assign"] if nshard == 0 else empty_shard_assign(c["assign"], shard)
    return pyoracle.Lists(metric, c["cen"], c["xb"], a)


def empty_shard_assign(assign, shard):
    a = np.asarray(assign, dtype=np.int64)
    keep = (a % 2 == shard) if shard < 2 else np.zeros(a.shape, bool)
    return np.where(keep, a, -1)


@functools.lru_cache(maxsize=None)
def synth_coarse(kind, metric, nprobe):
    """the reference's coarse ranking of all resident queries: its heap of nprobe entries, -1 beyond nlist (Heap.h:317-320); a slice
    of the queries has the rows of that slice"""
    from oracle import pyoracle
    c = synth_case(kind, metric)
    dis, keys = pyoracle.knn(metric, c["xq"], c["cen"], nprobe)
    dis.setflags(write=False), keys.setflags(write=False)
    return dis, keys


@functools.lru_cache(maxsize=None)
def synth_search(kind, metric, nprobe, k, nshard=0, shard=0):
    """the oracle's search_preassigned of all resident queries over those keys -> (D, I, stats)"""
    from oracle import pyoracle
    c = synth_case(kind, metric)
    dis, keys = synth_coarse(kind, metric, nprobe)
    D, I, st = pyoracle.search_preassigned(synth_lists(kind, metric, nshard, shard), c["xq"], k, keys, dis)
    D.setflags(write=False), I.setflags(write=False)
    return D, I, st


# ---- 5. resident query sets of one shape ------------------------------------------------------------------------------------------
def byte_query_sets():
    """A and B: two byte-valued query sets of one shape, different in every row; C: a larger one"""
    rs = np.random.RandomState(7100)
    d = SYNTH_KINDS["bytes"][0]
    A = rs.randint(0, 256, size=(SYNTH_NQ, d)).astype(np.float32)
    B = rs.randint(0, 256, size=(SYNTH_NQ, d)).astype(np.float32)
    C = rs.randint(0, 256, size=(4 * SYNTH_NQ + 7, d)).astype(np.float32)
    return A, B, C
