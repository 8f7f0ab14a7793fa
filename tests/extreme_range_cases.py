"""Float data at the ends of the fp32 range for the matrix-core filter of threshold rounds (scan_filter_kernel and
scan_filter_wide_kernel, ivf_filter.hip): norms that overflow, products that overflow, NaN and infinite elements, distances in the
subnormal range.  numpy only: the CPU test of the data's preconditions (test_extreme_range_cases_cpu.py) and the GPU test
(test_gpu_extreme_range.py) both read it; the engine is never imported here.

Every world: nlist 16, 3000 stored rows, 64 queries, k 10, nprobe 8, built at d = 24 (the narrowest d at which d * (2^62)^2 passes
FLT_MAX), 128 (the widest register-resident form) and 200 (the workgroup form).  The centres come in four groups of four close
neighbours, so that a query's true neighbours lie in several of its probed lists: what a threshold round drops is missed.

  l2_norm_overflow    L2.  Elements s * 2^62 + 2^50 * noise, s the sign pattern of the list's group.  |x|^2 and |y|^2 are +inf in
                      fp32, distances inside a group are about d * 2^101, between the two groups of a pair 2^127 (two coordinates
                      differ in sign), between pairs d / 2 * 2^126 = +inf, which the reference never admits.
  ip_norm_overflow    Inner product.  Queries s * 2^60 (1 + noise), rows s * f * A (1 + noise): f = -1 on the first d / 2 coordinates
                      of the filter's accumulation order (filter_order: one fp32 chain over pieces of eight, elements 0 4 1 5 2 6 3 7
                      of a piece -- mfma_tile.h: filter_mac), + 1.4 on the others, and A such that the negative half sums to
                      - 1.5 * 2^128.  The filter's single chain reaches -inf after d / 2 steps and stays there; the reference's four
                      chains (elements 4 i + l) each hold an eighth of that, and its value for a pair of one group is about
                      0.6 * 2^128: finite, and the query's best.  So EVERY row of a query's own group is such a row, not one planted
                      one.  |x| |y| is about 1.2 * 1.5 * 2^129: +inf.  Planted per group: two rows of 8 A |f| s (the product overflows
                      to +inf: admitted as the best, as the reference does) and two of the opposite sign (-inf: never admitted).
  nonfinite_elements  Both metrics, Gaussian data.  In every list six planted rows, at positions 0, 31, 32, 63, 64 and last (block and
                      mask-word edges), of four kinds in turn: a NaN element, a +inf element, a -inf element, and a row whose
                      distance overflows (elements of 3e38).  Queries 5, 31 and 32 hold a NaN element, a +inf element, and zeros.
  subnormal           L2.  Elements 2^-76 * n, n an integer of magnitude <= 1024.  A squared difference is n^2 * 2^-152: below the
                      smallest normal number whenever |n| < 2^13, and not on the subnormal grid (2^-149) unless 8 divides n^2.
                      The first eight queries are copies of stored rows (distance zero).
  integers_2p62       l2_norm_overflow from another seed.  Every value there is an integer already (the grid at 2^62 is 2^39) that no
                      int holds: the host's integer-range detection (IntRange: the byte and fused decisions) meets them.

The model (keep_model) restates the two keep tests of filter_verdicts as they stood before they learnt about non-finite operands,
in float32: C = (2 d + 32) 2^-24; xn, yn accumulated in double and rounded once (|.|^2 under L2, |.| under the inner product); p
the fp32 chain in filter_order, one fused step an element; L2: kept iff fma(2, p, -(1 - C) yn) > (1 - C) xn - thr; inner product:
kept iff fma(C xn, yn, p) > thr; a NaN threshold makes the right side +inf.  The threshold is the query's k-th distance after the
dense first round (`first` probes: one where the filter is off, ceil(k / (0.03 * list length)) = 2 at these shapes where it is on).
"""
import functools

import numpy as np

IP, L2 = 0, 1
NLIST, NB, NQ, K, NPROBE = 16, 3000, 64, 10, 8
DS = (24, 128, 200)
GROUP = 4
FMAX = np.finfo(np.float32).max
TINY = np.finfo(np.float32).tiny  # 2^-126
POSITIONS = (0, 31, 32, 63, 64, -1)
KINDS = ("nan", "+inf", "-inf", "overflow")
Q_NAN, Q_INF, Q_ZERO = 5, 31, 32

# name -> (metric, generator); the (world, d) pairs the tests run
WORLDS = ("l2_norm_overflow", "ip_norm_overflow", "nonfinite_l2", "nonfinite_ip", "subnormal", "integers_2p62")
MODEL_WORLDS = ("l2_norm_overflow", "ip_norm_overflow")  # the parent's keep test loses neighbours here
SPREAD_WORLDS = ("l2_norm_overflow", "ip_norm_overflow", "subnormal", "integers_2p62")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ----------------------------------------------------------------------------------------------------------------- the data
def filter_order(d):
    """the order in which the fp32 filter's one accumulation chain takes the elements of a row"""
    out = []
    for j in range((d + 7) // 8):
        for i in range(4):
            out += [8 * j + i, 8 * j + 4 + i]
    return np.array([c for c in out if c < d])


def patterns(d):
    """sign patterns of the four groups: 0 / 1 and 2 / 3 differ in the last two coordinates, the pairs in every second one"""
    p = np.ones((4, d), np.float64)
    p[2:] = (-1.0) ** np.arange(d)
    p[1, -2:] *= -1
    p[3, -2:] *= -1
    return p


def _assign(rs):
    return rs.randint(0, NLIST, size=NB).astype(np.int64)


def _l2_overflow(d, seed):
    rs = np.random.RandomState(seed)
    pat = patterns(d)[np.arange(NLIST) // GROUP] * 2.0 ** 62
    cen = pat + 2.0 ** 48 * rs.randn(NLIST, d)
    assign = _assign(rs)
    xb = cen[assign] + 2.0 ** 50 * rs.randn(NB, d)
    xq = cen[rs.randint(0, NLIST, size=NQ)] + 2.0 ** 50 * rs.randn(NQ, d)
    return cen, assign, xb, xq, {}


def _ip_overflow(d, seed):
    rs = np.random.RandomState(seed)
    f = np.full(d, 1.4)
    f[filter_order(d)[:d // 2]] = -1.0
    A = 3.0 * 2.0 ** 68 / d  # (d / 2) * 2^60 * A = 1.5 * 2^128
    group = np.arange(NLIST) // GROUP
    pat = patterns(d)
    noise = lambda n, s: 1.0 + s * np.clip(rs.randn(n, d), -3.5, 3.5)  # noqa: E731
    cen = pat[group] * f * A * noise(NLIST, 0.03)
    assign = _assign(rs)
    xb = cen[assign] * noise(NB, 0.05)
    qlist = rs.randint(0, NLIST, size=NQ)
    xq = pat[group[qlist]] * 2.0 ** 60 * noise(NQ, 0.03)
    planted = {}
    for g in range(NLIST // GROUP):  # two rows a group whose product with the group's queries overflows to +inf, two to -inf
        rows = np.nonzero(group[assign] == g)[0]
        for j, sign in enumerate((1.0, 1.0, -1.0, -1.0)):
            r = int(rows[7 + 40 * j])
            xb[r] = sign * 8.0 * A * np.abs(f) * pat[g]
            planted[r] = "+inf" if sign > 0 else "-inf"
    return cen, assign, xb, xq, planted


def _nonfinite(d, seed):
    rs = np.random.RandomState(seed)
    centre = rs.randn(NLIST // GROUP, d)
    centre[:, :4] = (3.0, 3.0, -3.0, -3.0)  # every query and every ordinary row: positive in coordinates 0 and 1, negative in 2 and 3
    cen = centre[np.arange(NLIST) // GROUP] + 0.1 * rs.randn(NLIST, d)
    assign = _assign(rs)
    xb = cen[assign] + 0.5 * rs.randn(NB, d)
    xq = cen[rs.randint(0, NLIST, size=NQ)] + 0.5 * rs.randn(NQ, d)
    planted = {}
    for l in range(NLIST):
        rows = np.nonzero(assign == l)[0]  # (lists hold their rows in database order)
        assert len(rows) > 65
        # under the inner product an infinite element or an overflowing row gives -inf against every ordinary query (never admitted),
        # but for lists 0 and 8 (infinite elements) and 4 and 12 (overflowing rows), where it gives +inf: admitted as the best
        up_inf, up_over = l % 8 == 0, l % 8 == 4
        for j, pos in enumerate(POSITIONS):
            r, kind = int(rows[pos]), KINDS[(j + l) % 4]
            if kind == "nan":
                xb[r, int(rs.randint(0, d))] = np.nan
            elif kind == "+inf":
                xb[r, (j % 2) if up_inf else 2 + j % 2] = np.inf
            elif kind == "-inf":
                xb[r, 2 + j % 2 if up_inf else j % 2] = -np.inf
            else:
                xb[r, :4] = 3e38 * np.array([1.0, 1.0, -1.0, -1.0]) * (1.0 if up_over else -1.0)
            planted[r] = kind
    xq[Q_NAN, d // 2] = np.nan
    xq[Q_INF, 1] = np.inf
    xq[Q_ZERO] = 0.0
    return cen, assign, xb, xq, planted


def _subnormal(d, seed):
    rs = np.random.RandomState(seed)
    sigma = {24: 300.0, 128: 640.0, 200: 470.0}[d]
    centre = rs.randint(-300, 301, size=(NLIST // GROUP, d))
    cen = centre[np.arange(NLIST) // GROUP] + np.rint(0.25 * sigma * rs.randn(NLIST, d))
    assign = _assign(rs)
    xb = np.clip(cen[assign] + np.rint(sigma * rs.randn(NB, d)), -1024, 1024)
    xq = np.clip(cen[rs.randint(0, NLIST, size=NQ)] + np.rint(sigma * rs.randn(NQ, d)), -1024, 1024)
    xq[:8] = xb[rs.permutation(NB)[:8]]
    s = 2.0 ** -76
    return cen * s, assign, xb * s, xq * s, {}


SPECS = {
    "l2_norm_overflow": (L2, _l2_overflow, 100),
    "ip_norm_overflow": (IP, _ip_overflow, 200),
    "nonfinite_l2": (L2, _nonfinite, 300),
    "nonfinite_ip": (IP, _nonfinite, 300),
    "subnormal": (L2, _subnormal, 400),
    "integers_2p62": (L2, _l2_overflow, 500),
}


@functools.lru_cache(maxsize=None)
def world(name, d):
    metric, gen, seed = SPECS[name]
    with np.errstate(all="ignore"):
        cen, assign, xb, xq, planted = gen(d, seed + d)
        cen, xb, xq = (np.ascontiguousarray(a, dtype=np.float32) for a in (cen, xb, xq))
    freeze(cen, assign, xb, xq)
    clean = np.array([q for q in range(NQ) if not (name.startswith("nonfinite") and q in (Q_NAN, Q_INF, Q_ZERO))])
    return dict(name=name, metric=metric, d=d, nlist=NLIST, cen=cen, assign=assign, xb=xb, xq=xq, planted=planted, clean=clean)


def oracle_lists(w, members=None):
    """the world's lists for the oracle; members: a mask over the stored rows (the ids stay what they were)"""
    from oracle import pyoracle
    assign = w["assign"] if members is None else np.where(members, w["assign"], -1)
    return pyoracle.Lists(w["metric"], w["cen"], w["xb"], assign)


# ------------------------------------------------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def ranked(name, d, nprobe=NPROBE):
    """the oracle's coarse ranking of the world's queries -> (coarse distances, keys)"""
    from oracle import pyoracle
    w = world(name, d)
    with np.errstate(all="ignore"):
        cd, ck = pyoracle.knn(w["metric"], w["xq"], w["cen"], nprobe)
    freeze(cd, ck)
    return cd, ck


@functools.lru_cache(maxsize=None)
def expected(name, d, nprobe=NPROBE, queries="all"):
    """the oracle's (D, I, stats) over the first `nprobe` lists of its own ranking; queries: "all" or "clean" """
    from oracle import pyoracle
    w = world(name, d)
    cd, ck = ranked(name, d)
    sel = np.arange(NQ) if queries == "all" else w["clean"]
    with np.errstate(all="ignore"):
        D, I, st = pyoracle.search_preassigned(oracle_lists(w), w["xq"][sel], K, ck[sel, :nprobe], cd[sel, :nprobe])
    freeze(D, I, st)
    return D, I, st


def identity_keys(n):
    return np.tile(np.arange(NLIST, dtype=np.int64), (n, 1))


@functools.lru_cache(maxsize=None)
def expected_exact(name, d, selected=False):
    """the oracle over every list in list-number order (what the exact calls equal); selected: over the ids with id % 3 == 0"""
    from oracle import pyoracle
    w = world(name, d)
    members = np.arange(NB) % 3 == 0 if selected else None
    keys = identity_keys(NQ)
    with np.errstate(all="ignore"):
        D, I, st = pyoracle.search_preassigned(oracle_lists(w, members), w["xq"], K, keys, np.zeros(keys.shape, np.float32))
    freeze(D, I, st)
    return D, I, st


@functools.lru_cache(maxsize=None)
def exact_radius(name, d):
    """between the 5th and 6th true distance of the median query (the clean queries, ordered by their 5th distance); where infinities
    lead a result (the inner product over planted rows) the 5th and 6th of the finite ones: the infinities are inside any radius"""
    from oracle import pyoracle
    w = world(name, d)
    keys = identity_keys(NQ)
    with np.errstate(all="ignore"):
        D = pyoracle.search_preassigned(oracle_lists(w), w["xq"], 4 * K, keys, np.zeros(keys.shape, np.float32))[0][w["clean"]]
    pairs = []
    for row in D:
        fin = row[np.isfinite(row)]
        if len(fin) >= 6 and fin[4] != fin[5]:
            pairs.append((fin[4], fin[5]))
    a, b = sorted(pairs)[len(pairs) // 2]
    r = np.float32(0.5 * (np.float64(a) + np.float64(b)))
    if not min(a, b) < r < max(a, b):  # (neighbouring floats: the reference keeps dis < radius / dis > radius)
        r = max(a, b)
    return float(r)


# ---------------------------------------------------------------------------------------------------------------- the model
def norms(metric, m):
    """|row|^2 (L2) or |row| (inner product), accumulated in double and rounded once"""
    with np.errstate(all="ignore"):
        sq = (m.astype(np.float64) ** 2).sum(1)
        return (sq if metric == L2 else np.sqrt(sq)).astype(np.float32)


def chain_product(xq, xb):
    """(nq, nb) x . y as the fp32 filter accumulates it: one chain in filter_order, a fused step an element"""
    acc = np.zeros((xq.shape[0], xb.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for c in filter_order(xq.shape[1]):
            acc = (acc.astype(np.float64) + xq[:, c].astype(np.float64)[:, None] * xb[:, c].astype(np.float64)[None, :]).astype(np.float32)
    return acc


def keep_model(metric, d, p, xn, yn, thr):
    """the keep tests of filter_verdicts before non-finite operands were kept: (nq, nb) bool"""
    f = np.float32
    C = f((2 * d + 32) * 2.0 ** -24)
    xn, yn, thr = np.asarray(xn, f)[:, None], np.asarray(yn, f)[None, :], np.asarray(thr, f)[:, None]
    with np.errstate(all="ignore"):
        if metric == L2:
            u = (f(1) - C) * xn - thr
            t = (2.0 * p.astype(np.float64) - ((f(1) - C) * yn).astype(np.float64)).astype(f)
        else:
            u = thr
            t = ((C * xn).astype(np.float64) * yn.astype(np.float64) + p.astype(np.float64)).astype(f)
        u = np.where(np.isnan(thr), f(np.inf), u)
        return t > u


def lost_by_model(name, d, first):
    """queries in which the model drops a true neighbour: an entry of the oracle's result over NPROBE lists that lies in a list
    ranked behind the `first` dense ones and fails the keep test at the threshold those leave -> (n lost queries, n lost entries)"""
    w = world(name, d)
    _, ck = ranked(name, d)
    D, I, _ = expected(name, d)
    D1, I1, _ = expected(name, d, nprobe=first)
    thr = np.where(I1[:, K - 1] >= 0, D1[:, K - 1], np.float32(FMAX if w["metric"] == L2 else -FMAX))
    kept = keep_model(w["metric"], d, chain_product(w["xq"], w["xb"]), norms(w["metric"], w["xq"]), norms(w["metric"], w["xb"]), thr)
    lost_q = lost_e = 0
    for q in range(NQ):
        ids = I[q][I[q] >= 0]
        later = ~np.isin(w["assign"][ids], ck[q, :first])
        n = int((later & ~kept[q, ids]).sum())
        lost_q += n > 0
        lost_e += n
    return lost_q, lost_e


def spread(name, d):
    """per query: how many of the oracle's top k lie in lists ranked second or later"""
    w = world(name, d)
    _, ck = ranked(name, d)
    _, I, _ = expected(name, d)
    return np.array([int((w["assign"][I[q][I[q] >= 0]] != ck[q, 0]).sum()) for q in range(NQ)])
