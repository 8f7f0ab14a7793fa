"""Data and a numpy model for the tests of the error bound that three list-side kernels drop candidates by: the fp16 list filter
(scan_filter_kernel<.., HALF> and scan_filter_wide_kernel<.., HALF>, ivf_filter.hip) and the fp16 exact pass (scan_all_f16_kernel,
ivf_exact.hip).  numpy only: the CPU test of the data's preconditions (test_filter_bound_cases_cpu.py) and the GPU test
(test_gpu_filter_bound.py) both read it; the engine is never imported here.

The data is coarse_pick_cases.coherent's: every query rounds down in the cast to fp16 and so does one half of the stored rows, the
other half rounds up, all by 0.49 steps of the fp16 grid.  The fp16 product of a query with a row that rounds down is then short of
the exact one by 0.5 .. 0.8 of 2^-10 |x| |y| -- Gaussian data reaches a few per cent of that -- and a keep test that leaves the
operands' rounding out of its constant drops true neighbours.

The model restates what the kernels promise, not how they compute it:
  approximate product    fp16(x sx) . fp16(y sy) / (sx sy), the dot product in float64 (the matrix cores' own accumulation differs
                         from that at 2^-24, four orders below the operands' rounding)
  keep                   exact_args.h: exact_float_keep over exact_float_bound and exact_float_slack, in fp32 as there --
                         L2: 2 p - (1 - C) |y|^2 >= (1 - C) |x|^2 - tau, IP: p + C |x| |y| >= tau
  C                      coarse_pick_cases.half_constant(d, False) = (2 d + 32) 2^-24 + 2^-10 + 2^-12: no matrix here is held exactly
  threshold              the k-th exact distance over the `s` lists ranked best by exact centroid distance (the exact pass's seed), or
                         over the lists a caller names (the filter's first round)
  candidates             the stored entries the keep test lets through; valid: those whose exact distance is at or within the threshold

What this data cannot see: a constant short by the 2^-12 term alone.  The observed error stays below 0.8 of 2^-10 |x| |y|, so
(2 d + 32) 2^-24 + 2^-10 loses nothing either; the data separates the real constant from the fp32 one ((2 d + 32) 2^-24, three orders
smaller) and from half of the real one, not from mutants within a quarter of it.
"""
import functools
from types import SimpleNamespace

import numpy as np

import coarse_pick_cases as cp

L2, IP = 1, 0
NB, N, NLIST, K = 4000, 256, 16, 10
CAP = 1024  # the exact pass's candidate slots per query (the default)

# (metric, d, W, mid, seed of the assignment): W = the spread of the grid points (coherent): 128 under the inner product; the whole grid
# under L2, where a narrow spread makes the distances tiny beside the norms and every entry a candidate.  mid = the seed depth at
# which the threshold sits a few ranks beyond the k-th: a dropped neighbour leaves k valid candidates and the result is wrong (at
# TIGHT it leaves fewer, and the query goes the general way, right again).  Under the inner product the best rows are the same few
# for most queries, so whether a depth is "mid" hangs on the lists those few fell into: at d = 32 no depth is under assignment 3
# (the fp32 constant loses 0 queries up to 11 lists and leaves all 256 short of k from 12 on), under assignment 4 eight lists are
EXACT_CASES = [(IP, 64, 128, 8, 3), (L2, 64, 1024, 12, 3), (IP, 100, 128, 12, 3), (L2, 100, 1024, 12, 3), (L2, 128, 1024, 12, 3),
               (IP, 32, 128, 8, 4)]
TIGHT = NLIST
# ... under a selector that keeps every second id the seed's nprobe doubles (exact_args.h: exact_selected_seed) and must stay below
# nlist: the option's values 7 and 6 make 14 lists, the deepest seed there is, and 12.  (metric, d, W, seed of the assignment); the
# inner product at d = 100: at d = 64 no assignment of 3 .. 15 has a depth at which the fp32 constant gives 32 wrong results
SELECTED_CASES = [(IP, 100, 128, 3), (L2, 64, 1024, 3)]
SELECTED_OPTION = (7, 6)


def selected_depth(option):
    """exact_selected_seed(option, NB, NB / 2)"""
    return 2 * option


# the filter in threshold rounds: list 0 holds DENSE of the rows and is every query's first probe
DENSE = 0.75
FILTER_D = [64, 96, 128, 136, 200]   # 4, 6, 8 register-resident pieces; the workgroup form beyond 128 dimensions
NARROW_D = [136]                     # ... and the one-wave form there
FILTER_SELECTED = (L2, 96)


def spread(metric):
    return 1024 if metric == L2 else 128


# ------------------------------------------------------------------------------------------ the data
def uniform_assign(seed):
    a = np.random.RandomState(seed).randint(0, NLIST, size=NB)
    a.setflags(write=False)
    return a


def dense_first_assign(seed, share=DENSE):
    """list 0 holds `share` of the rows, the other lists the rest, uniformly"""
    rs = np.random.RandomState(seed)
    a = np.where(rs.rand(NB) < share, 0, rs.randint(1, NLIST, size=NB))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=4)  # (a case carries its n x nb products once report() has run: few are kept)
def case(metric, d, W, layout="uniform", seed=3):
    cen, xq, xb = cp.coherent(d, NLIST, N, W, nb=NB)
    assign = uniform_assign(seed) if layout == "uniform" else dense_first_assign(seed)
    return SimpleNamespace(metric=metric, d=d, W=W, k=K, cen=cen, xq=xq, xb=xb, assign=assign, ids=np.arange(NB, dtype=np.int64))


def members(c, mask):
    """the case with the stored rows that `mask` keeps (the ids stay what they were)"""
    return SimpleNamespace(metric=c.metric, d=c.d, W=c.W, k=c.k, cen=c.cen, xq=c.xq, xb=c.xb[mask], assign=c.assign[mask], ids=c.ids[mask])


def every_second(c):
    return members(c, c.ids % 2 == 1)


# ------------------------------------------------------------------------------------------ the model
def approx_product(xq, xb):
    sx, sy = cp.half_scale(xq), cp.half_scale(xb)
    assert sx > 0 and sy > 0
    xh = (xq * np.float32(sx)).astype(np.float16).astype(np.float64)
    yh = (xb * np.float32(sy)).astype(np.float16).astype(np.float64)
    return (xh @ yh.T) / (sx * sy)


def norms(metric, m):
    """|row|^2 (L2) or |row| (IP), accumulated in double and rounded once"""
    sq = (m.astype(np.float64) ** 2).sum(1)
    return (sq if metric == L2 else np.sqrt(sq)).astype(np.float32)


def keep(metric, C, p, xn, yn, tau):
    """exact_float_keep(l2, C, p, yn, exact_float_bound(l2, C, xn, tau), exact_float_slack(l2, C, xn)) for every pair: p is n x nb,
    xn and tau have n entries, yn has nb.  fp32 throughout; the fused multiply-add as one rounding of the float64 value"""
    f = np.float32
    C, p = f(C), np.asarray(p, f)
    xn, yn, tau = np.asarray(xn, f)[:, None], np.asarray(yn, f)[None, :], np.asarray(tau, f)[:, None]
    one_c = f(1) - C
    if metric == L2:
        bound = one_c * xn - tau
        t = (2.0 * p.astype(np.float64) - (one_c * yn).astype(np.float64)).astype(f)
    else:
        bound = tau
        t = ((C * xn).astype(np.float64) * yn.astype(np.float64) + p.astype(np.float64)).astype(f)
    return t >= bound


def within(metric, exact, tau):
    """at or within the threshold: the entries a pass must not drop"""
    tau = np.asarray(tau)[:, None]
    return exact <= tau if metric == L2 else exact >= tau


def ranking(c):
    """the lists of every query, best first, by exact centroid distance"""
    return np.argsort(cp.order(c.metric, cp.exact_distances(c.metric, c.xq, c.cen)), axis=1, kind="stable")


def kth(c, exact, allowed):
    """the k-th best exact distance of every query among the entries `allowed` marks (n x nb)"""
    key = np.where(allowed, cp.order(c.metric, exact), np.inf)
    t = np.sort(key, axis=1)[:, c.k - 1]
    assert np.isfinite(t).all()
    return t if c.metric == L2 else -t


def seed_threshold(c, exact, seed_lists, rank=None):
    """the threshold of a seed over the best `seed_lists` lists of `rank` (default: the model's own ranking)"""
    rank = ranking(c) if rank is None else np.asarray(rank)
    probed = np.zeros((len(c.xq), NLIST), bool)
    np.put_along_axis(probed, rank[:, :seed_lists], True, axis=1)
    return kth(c, exact, probed[:, c.assign])


def products(c):
    """(exact distances, approximate products) of every pair of the case, computed once"""
    if not hasattr(c, "_products"):
        c._products = (cp.exact_distances(c.metric, c.xq, c.xb), approx_product(c.xq, c.xb))
    return c._products


def report(c, seed_lists, C, rank=None, tau=None, entries=None):
    """-> dict(lost, wrong, fallback, most) in queries, most in candidates.  The threshold is `tau` where the caller has one (the
    reference's seed), else the k-th exact distance over the best `seed_lists` lists of `rank` (the reference's ranking, or the
    model's).  lost: a true top-k entry is not kept; wrong: ... and k valid candidates remain, so the pass answers, wrongly;
    fallback: ... and fewer remain, so the query goes the general way; most: the largest candidate count of one query.
    entries: only these stored rows go through the keep test (the filter's later rounds); the others count as kept."""
    exact, approx = products(c)
    if tau is None:
        tau = seed_threshold(c, exact, seed_lists, rank)
    kept = keep(c.metric, C, approx, norms(c.metric, c.xq), norms(c.metric, c.xb), tau)
    if entries is not None:
        kept = kept | ~np.asarray(entries)[None, :]
    top = np.argsort(cp.order(c.metric, exact), axis=1, kind="stable")[:, :c.k]
    lost = ~np.take_along_axis(kept, top, axis=1).all(axis=1)
    valid = (kept & within(c.metric, exact, tau)).sum(1)
    return dict(lost=int(lost.sum()), wrong=int((lost & (valid >= c.k)).sum()), fallback=int((lost & (valid < c.k)).sum()),
                most=int(kept.sum(1).max()))


def dense_first_report(c, C):
    """the filter in threshold rounds over the dense-first layout: list 0 is scanned first, so whatever the schedule a later round's
    threshold is at or within the k-th distance over list 0 alone -- the loosest a round can hold.  An entry of lists 1 .. that the keep
    test drops at that threshold is dropped at every tighter one: lost counts the queries that CERTAINLY lose a final top-k entry"""
    exact, _ = products(c)
    tau = kth(c, exact, np.broadcast_to(c.assign == 0, exact.shape))
    return report(c, None, C, tau=tau, entries=c.assign != 0)


def err_over_bound(c):
    """the largest |approximate - exact| product of a pair over 2^-10 |x| |y|"""
    x, y = c.xq.astype(np.float64), c.xb.astype(np.float64)
    rel = np.abs(approx_product(c.xq, c.xb) - x @ y.T) / (np.sqrt((x * x).sum(1))[:, None] * np.sqrt((y * y).sum(1))[None, :]) / cp.U
    return float(rel.max())
