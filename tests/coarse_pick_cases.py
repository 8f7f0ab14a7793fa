"""Data and a numpy model for the tests of the matrix-core coarse ranking (coarse_gemm16_kernel -> coarse_pick_kernel -> the exact
re-run of the flagged rankings).  numpy only: the CPU test of the model's preconditions (test_coarse_pick_cases_cpu.py) and the GPU
test (test_gpu_coarse_pick_edges.py) both read it; the engine is never imported here.

The model restates what the kernels promise, not how they compute it:
  approximate distance   fp16(x sx) . fp16(c sy) / (sx sy), the dot product in float64 (the matrix cores' own accumulation differs
                         from that at 2^-24, four orders below the operands' rounding); L2 = |x|^2 + |c|^2 - 2 ip, clamped at 0
  eps                    C (|x|^2 + max |c|^2) (L2), C |x| max |c| (IP)
  candidates             approximate distances at or within a threshold widened by `widen` eps (the kernel: 2), the threshold being
                         any with nprobe .. nprobe + nprobe / 8 + 2 approximate distances under it (where its bisection stops)
  C                      (2 d + 32) 2^-24, + 2^-10 + 2^-12 unless every operand is an integer of magnitude <= 2048
                         (exact_float_constant); fp32_constant is what the fp32-operand form of the product uses -- too small by
                         three orders for fp16 operands
"""
import functools
import math

import numpy as np

PICK_CAP = 1024
U = 2.0 ** -10  # the fp16 grid's step in [1, 2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------ the model
def fp32_constant(d):
    return (2 * ((d + 3) & ~3) + 32) * 2.0 ** -24


def half_constant(d, operands_exact):
    C = (2 * d + 32) * 2.0 ** -24
    return C if operands_exact else C + 2.0 ** -10 + 2.0 ** -12


def held_exactly(m):
    with np.errstate(invalid="ignore"):
        return bool(np.all((m == np.trunc(m)) & (np.abs(m) <= 2048)))


def half_scale(m):
    """half_scale_of: the power of two that brings the largest magnitude into [2^14, 2^15); 1 for integers fp16 holds as they are;
    0 where one scale does not serve the matrix"""
    m = np.asarray(m, dtype=np.float32)
    amax = float(np.abs(m).max())
    if held_exactly(m) or amax == 0.0:
        return 1.0
    if not amax < math.inf:
        return 0.0
    e = math.frexp(amax)[1]
    if e > 24 or e < -24:
        return 0.0
    rows = np.abs(m).max(axis=1)
    if rows[rows > 0].min() < amax * 2.0 ** -12 * max(1.0, m.shape[1] / 1024.0):
        return 0.0
    return 2.0 ** (15 - e)


def order(metric, dist):
    """smaller = better, whatever the metric"""
    return dist if metric == 1 else -dist


def exact_distances(metric, xq, cen):
    x, c = xq.astype(np.float64), cen.astype(np.float64)
    ip = x @ c.T
    return (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2 * ip if metric == 1 else ip


def approx_distances(metric, xq, cen):
    sx, sy = half_scale(xq), half_scale(cen)
    assert sx > 0 and sy > 0
    xh = (xq * np.float32(sx)).astype(np.float16).astype(np.float64)
    ch = (cen * np.float32(sy)).astype(np.float16).astype(np.float64)
    ip = (xh @ ch.T) / (sx * sy)
    if metric == 0:
        return ip
    x, c = xq.astype(np.float64), cen.astype(np.float64)
    return np.maximum((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2 * ip, 0.0)


def eps_of(metric, C, xq, cen):
    xn = (xq.astype(np.float64) ** 2).sum(1)
    cmax = (cen.astype(np.float64) ** 2).sum(1).max() * (1.0 + 1e-6)
    return C * (xn + cmax) if metric == 1 else C * np.sqrt(xn) * math.sqrt(cmax)


def candidates(metric, approx, eps, nprobe, widen=2.0, loosest=True):
    """the mask of centroids at or within the widened threshold; loosest: the threshold is the (nprobe + nprobe / 8 + 2)-th approximate
    distance, the last the kernel's bisection may stop at, otherwise the nprobe-th, the first"""
    key = order(metric, approx)
    rank = nprobe + nprobe // 8 + 2 if loosest else nprobe
    T = np.sort(key, axis=1)[:, rank - 1]
    return key <= (T + widen * eps)[:, None]


def loses(mask, top):
    """per query: a member of its true top-nprobe (top: n x nprobe centroid numbers) is no candidate"""
    return ~np.take_along_axis(mask, top, axis=1).all(axis=1)


def true_top(metric, xq, cen, nprobe):
    return np.argsort(order(metric, exact_distances(metric, xq, cen)), axis=1, kind="stable")[:, :nprobe]


def bound_report(metric, xq, cen, nprobe, top=None):
    """what the tests of the bound require of their data, from the model alone (top: the reference's ranking where there is one)"""
    d = xq.shape[1]
    if top is None:
        top = true_top(metric, xq, cen, nprobe)
    approx = approx_distances(metric, xq, cen)
    C = half_constant(d, held_exactly(xq) and held_exactly(cen))
    eps = eps_of(metric, C, xq, cen)
    lost = lambda e, w: int(loses(candidates(metric, approx, e, nprobe, w), top).sum())
    return dict(n=len(xq),
                lost_fp32=lost(eps_of(metric, fp32_constant(d), xq, cen), 2.0),
                lost_unwidened=lost(eps, 0.0),
                lost_one_eps=lost(eps, 1.0),
                lost=lost(eps, 2.0),
                most=int(candidates(metric, approx, eps, nprobe).sum(1).max()),
                fewest_at_first_stop=int(candidates(metric, approx, eps, nprobe, loosest=False).sum(1).min()),
                err_over_eps=float((np.abs(approx - exact_distances(metric, xq, cen)) / eps[:, None]).max()))


def fewest_candidates_fp32_form(metric, xq, cen, nprobe):
    """the fp32-operand form of the product (coarse_pick = 1): approximate = exact at this model's precision, eps from fp32_constant;
    the fewest candidates of a query at the tightest threshold the kernel may stop at"""
    eps = eps_of(metric, fp32_constant(xq.shape[1]), xq, cen)
    return int(candidates(metric, exact_distances(metric, xq, cen), eps, nprobe, loosest=False).sum(1).min())


def distinct_counts(D):
    """(a, b) of a reference ranking D of nprobe + 1 entries a query: the queries whose nprobe + 1 best distances are finite and
    pairwise distinct -- the picked path must answer those -- and those whose nprobe best are -- it may answer no others"""
    D = np.asarray(D, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = lambda M: np.isfinite(M).all(axis=1) & (np.diff(M, axis=1) != 0).all(axis=1)
        return int(ok(D).sum()), int(ok(D[:, :-1]).sum())


# ------------------------------------------------------------------------------------------ the data
@functools.lru_cache(maxsize=None)
def near_centroids(kind, metric, nlist, n, d, seed=17):
    """queries near centroids: Gaussian floats (scaled to fp16) or byte-valued integers (scale 1, the exact-operand constant)"""
    rs = np.random.RandomState(seed)
    if kind == "bytes":
        cen = rs.randint(0, 256, size=(nlist, d)).astype(np.float32)
        xq = np.clip(cen[rs.randint(0, nlist, n)] + rs.randint(-40, 41, size=(n, d)), 0, 255).astype(np.float32)
    else:
        cen = rs.randn(nlist, d).astype(np.float32)
        xq = (cen[rs.randint(0, nlist, n)] + 0.7 * rs.randn(n, d)).astype(np.float32)
        if metric == 0:
            cen /= np.linalg.norm(cen, axis=1, keepdims=True)
            xq /= np.linalg.norm(xq, axis=1, keepdims=True)
    cen.setflags(write=False)
    xq.setflags(write=False)
    return cen, xq


def coherent_rows(rs, base, W, rows, up=None):
    """points of the fp16 grid of [1, 2) around `base`, displaced by 0.49 steps so that the cast to fp16 rounds every component of a
    row the same way: down, or up for the rows that up(rows) marks (drawn after the rows themselves)"""
    g = (1.0 + (base[None, :] + rs.randint(0, W, size=(rows, len(base)))) * U + 0.49 * U).astype(np.float32)
    if up is not None:
        g[up(rows)] -= np.float32(0.98 * U)
    return g


@functools.lru_cache(maxsize=None)
def coherent(d, nlist, n, W, seed=5, nb=0):
    """-> centroids (a random half rounds up, the others down), queries (all round down) and nb database vectors (half and half).
    The largest magnitude lies in [1, 2): the scale is 2^14 and every operand is off by 0.49 steps of the fp16 grid, so a query's
    approximate distances to the two families of centroids are displaced against each other by about 2^-10 |x| |c|."""
    rs = np.random.RandomState(seed)
    base = rs.randint(0, 1024 - W, size=d) if W < 1024 else np.zeros(d, dtype=np.int64)  # (W = 1024: the whole grid)
    half = lambda rows: rs.rand(rows) < 0.5
    cen = coherent_rows(rs, base, W, nlist, up=half)
    xq = coherent_rows(rs, base, W, n)
    xb = coherent_rows(rs, base, W, nb, up=half) if nb else None
    for m in (cen, xq, xb):
        if m is not None:
            m.setflags(write=False)
    return cen, xq, xb


# (metric, d, nlist, nprobe, W): IP where the candidates stay few with a narrow spread, L2 over the whole grid -- with a narrow one
# the L2 distances are tiny beside the norms and every centroid is a candidate (CAP_CASES)
BOUND_CASES = [(0, 64, 1024, 16, 128), (0, 64, 1024, 128, 128), (0, 64, 4096, 32, 128), (0, 100, 640, 32, 128),
               (1, 64, 1024, 16, 1024), (1, 100, 640, 32, 1024)]
BOUND_N = 256
# the candidate cap: (nlist, nprobe, n) on L2 data of W = 32, d = 64 -- beyond PICK_CAP, and exactly at it
CAP_D, CAP_W = 64, 32
CAP_OVER = (4096, 32, 259)
CAP_AT = (1024, 16, 256)
