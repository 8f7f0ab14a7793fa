"""The data of test_gpu_exact_wide_bytes.py (the byte list pass beyond 128 dimensions), made here so that
test_exact_wide_bytes_cpu.py can assert its preconditions without a GPU: the byte rule d m^2 <= 2^24 holds, the queries that tie are
the stated ones, and no query has more entries at or within its true k-th distance than candidate slots.  Every case has 16 lists: the
default seed of 16 lists then reads every list, so a query's threshold is its true k-th distance and its candidates are exactly the
entries numpy counts."""
import numpy as np

from test_gpu_exact import IP, L2, byte_case, ragged_assign
from test_gpu_wide_bytes import exact_table, limit_m

CAP = 1024  # the default candidate slots per query
NLIST = 16
NB = 4000
STAGE_D = [132, 192, 200, 384, 960, 1024]  # J = 5 (one padded stage), 6 (one stage), 7, 12 (two stages), 30, 32 (d m^2 = 2^24)
BATCHES = [(1, 100), (33, 65), (128, 10), (129, 64), (257, 1)]


def ties_within(metric, xb, xq, k):
    """(queries in whose best min(k + 1, ntotal) distances two neighbours are equal, entries at or within the true k-th distance), from
    exact integers"""
    E = exact_table(metric, xq, xb)
    dis = E if metric == L2 else -E
    w = min(k + 1, len(xb))
    best = np.sort(dis, axis=1)[:, :w]
    within = (dis <= best[:, min(k, len(xb)) - 1][:, None]).sum(1)
    return (best[:, 1:] == best[:, :-1]).any(axis=1), within


def top_of(d):
    return limit_m(d)


def stage_case(d, metric):
    """clustered byte rows 0 .. limit_m(d) over the ragged assignment; the largest value is met on both sides"""
    top = top_of(d)
    cen, assign, xb, xq = byte_case(d, NLIST, seed=1500 + d + metric, top=top, nq=257, nb=NB)
    xb[17, d - 1] = top
    xq[5, d - 1] = top
    # the batch of one query asks for k = 100: the first query is one whose best 101 distances are pairwise different
    tied, _ = ties_within(metric, xb, xq, 100)
    first = int(np.nonzero(~tied)[0][0])
    xq[[0, first]] = xq[[first, 0]]
    return cen, assign, xb, xq


TAIL_SIZES = [((100, 64, 0, 130, 50, 30), 16), ((100, 64, 0, 130, 50), 14), ((0, 0, 40, 0), 2)]


def tail_case(sizes, metric, d=200, nq=40):
    """lists of the given sizes around byte centroids far from each other; the queries lie around the LAST non-empty list's centroid"""
    rs = np.random.RandomState(1300 + len(sizes) + metric)
    nlist = len(sizes)
    cen = rs.randint(0, 256, size=(nlist, d)).astype(np.float32)
    last = max(l for l in range(nlist) if sizes[l])
    if metric == IP:
        cen[last] = np.clip(cen[last] + 100, 0, 255)  # (the inner product's neighbours are the rows of large values)
    assign = np.repeat(np.arange(nlist), sizes)
    xb = np.clip(cen[assign] + rs.randint(-12, 13, size=(len(assign), d)), 0, 255).astype(np.float32)
    xq = np.clip(cen[last] + rs.randint(-12, 13, size=(nq, d)), 0, 255).astype(np.float32)
    return cen, assign, xb, xq, last


def last_dims_case(d, metric):
    """every row of a list equals its centroid in all but the last eight dimensions and differs in those only; so do the queries"""
    nlist, nb, n = NLIST, 3000, 64
    rs = np.random.RandomState(77 + metric + d)
    cen = rs.randint(0, 256, size=(nlist, d)).astype(np.float32)
    cen[:, d - 8:] = 0
    assign = rs.randint(0, nlist, size=nb)
    xb = cen[assign].copy()
    xb[:, d - 8:] = rs.randint(0, 256, size=(nb, 8))
    xq = cen[rs.randint(0, nlist, size=n)].copy()
    xq[:, d - 8:] = rs.randint(0, 256, size=(n, 8))
    return cen, assign, xb.astype(np.float32), xq.astype(np.float32)


def small_range_case(metric, n=200, k=5, d=136, nb=6000):
    """values 0 .. 8: many equal distances.  The queries are the first n of 3 n whose entries at or within the true k-th distance fill
    at most half the slots"""
    rs = np.random.RandomState(8)
    assign = ragged_assign(NLIST, nb)
    cen = rs.randint(0, 9, size=(NLIST, d)).astype(np.float32)
    xb = rs.randint(0, 9, size=(nb, d)).astype(np.float32)
    xq = rs.randint(0, 9, size=(3 * n, d)).astype(np.float32)
    tied, within = ties_within(metric, xb, xq, k)
    pick = np.nonzero(within <= CAP // 2)[0][:n]
    return cen, assign, xb, xq[pick], tied[pick], within[pick]


def range_case(d, metric, nq=40):
    """uniform byte rows 0 .. limit_m(d); the queries are the nq of 3 nq whose squared norms lie nearest the median"""
    top = top_of(d)
    cen, assign, xb, xq = byte_case(d, NLIST, seed=560 + d + metric, top=top, clustered=False, nq=3 * nq, nb=NB)
    s = (xq * xq).sum(1)
    xq = xq[np.sort(np.argsort(np.abs(s - np.median(s)), kind="stable")[:nq])].copy()
    return cen, assign, xb, xq
