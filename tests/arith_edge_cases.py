"""Cases and a CPU model for the edges of the scan's arithmetic choice (IntRange in ivf_engine.hip); no GPU here.

Every fp32 list scan and the exact coarse ranking pick, per call, from the value ranges of the two operand sets:
  2  byte codes on the i8 matrix cores: both sides integers 0 .. 255 and d * m^2 <= 2^24 (m the largest value on either side);
  1  fused fma(t, t, acc): all operands integers with |v| <= 4095, and under L2 the spread hi - lo over BOTH sides <= 4096;
  0  the reference's order acc += t * t: anything else.
Arithmetic 1 equals the reference only while every product t * t (or x * y) is an fp32 number: |t| <= 4096 gives t^2 <= 2^24,
while 4097^2 = 2^24 + 8193 is odd above 2^24 and is rounded before the reference adds it.  So the rule's edge is spread 4096
(inside) against 4097 (one step outside), and +-4095 against +-4097 under the inner product (4097 * 4095 is still exact).

The model restates the scan's sum in numpy: four lane accumulators over 4-wide steps (a zero-padded tail, as the reference's masked
tail and the engine's padded rows), then (s0 + s1) + (s2 + s3).  Unfused: float32(acc + float32(a * b)).  Fused:
float32(float64(acc) + float64(a) * float64(b)) -- one rounding; float64 holds product and sum exactly at these magnitudes (a
48-bit product under an accumulator below 2^34).  tests/test_arith_edge_cases_cpu.py pins the unfused model to the oracle on every
case (odd tails included: d = 30 agrees, so the model is not kept to d % 4 == 0) and shows that the fused model differs from it on
returned pairs of every teeth case: a wrongly fused call there returns wrong bits.

Data: half of all coordinates sit at the extremes of the side's range (that is what makes partial sums pass 2^24 and the two
roundings part); query 0 and the single row of list 1 are made of the extremes alone, in all four combinations
(coordinate c % 4: (q hi, row hi), (q hi, row lo), (q lo, row hi), (q lo, row lo)), and query 0 probes list 1 -- so the joint
extreme |t| (4096 inside the rule) is summed in a probed pair, and every call (query 0 is in each) has the case's full query range.
Shapes: nlist 8, list lengths 0, 1, 63, 64, 65, 129, 700 (129 twice), nprobe 4, calls of the first 3, 70 and 300 queries (each
work-item shape of the scan), every third query probing the three shortest lists only (all their rows are returned at k = 100)."""
import functools

import numpy as np

IP, L2 = 0, 1
NLIST, NPROBE = 8, 4
LENGTHS = (0, 1, 63, 64, 65, 129, 700, 129)
CALLS = (3, 70, 300)
KS = (1, 10, 100)
NQ = max(CALLS)
EDGE = 4096          # the largest |t| whose square fp32 holds for every integer t up to it
MAG = 4095           # the largest operand magnitude IntRange accepts
BYTE_LIMIT = 1 << 24

# name: metric, d, list range, query range, centroid range (None: the lists'), pokes (side, row, column, value), expected scan
# arithmetic, teeth (the fused model must differ from the oracle on a returned pair), coarse teeth (... on a coarse distance).
# Rows of pokes: "q" a query (1: in every call), "b" a database row given as (list, offset), "c" a centroid.
SPECS = {
    # inside the rule: spread exactly 4096 / magnitude exactly 4095
    "l2_lo_m1":        (L2, 16,  (-1, 4095),     (-1, 4095),    None, (), 1, False, False),
    "l2_hi_p1":        (L2, 30,  (-4095, 1),     (-4095, 1),    None, (), 1, False, False),
    "l2_sym_negzero":  (L2, 128, (-2048, 2048),  (-2048, 2048), None, "negzero", 1, False, False),
    "ip_full":         (IP, 100, (-4095, 4095),  (-4095, 4095), None, (), 1, False, False),
    "l2_halves":       (L2, 100, (-2048, 0),     (0, 2048),     (-2048, 0), (), 1, False, False),
    "ip_halves":       (IP, 16,  (-4095, 0),     (0, 4095),     (-4095, 0), (), 1, False, False),
    # one step outside
    "l2_list_4097":    (L2, 16,  (-2, 4095),     (-1, 4095),    (-1, 4095), (), 0, True, False),
    "l2_query_4097":   (L2, 128, (-1, 4095),     (-2, 4095),    None, (), 0, True, False),
    "l2_joint_4097":   (L2, 30,  (-2049, -1000), (1000, 2048),  (-2048, -1000), (), 0, True, False),
    "l2_centred_4097": (L2, 100, (-2049, 2048),  (-2049, 2048), None, (), 0, True, False),
    "ip_4097":         (IP, 16,  (-4097, 4097),  (-4097, 4097), (-4095, 4095), (), 0, True, False),
    "l2_value_4096":   (L2, 100, (0, 4095),      (0, 4095),     None, (("b", (6, 11), 5, 4096.0),), 0, False, False),
    "l2_half_list":    (L2, 16,  (-1, 4095),     (-1, 4095),    None, (("b", (2, 3), 7, 0.5),), 0, False, False),
    "l2_half_query":   (L2, 128, (-1, 4095),     (-1, 4095),    None, (("q", 1, 9, 0.5),), 0, False, False),
    "ip_half_query":   (IP, 30,  (-4095, 4095),  (-4095, 4095), None, (("q", 1, 9, 0.5),), 0, False, False),
    # the byte rule's neighbours
    "bytes":           (L2, 128, (0, 255),       (0, 255),      None, (), 2, False, False),
    "bytes_query_m1":  (L2, 128, (0, 255),       (0, 255),      None, (("q", 1, 9, -1.0),), 1, False, False),
    "bytes_list_256":  (IP, 16,  (0, 255),       (0, 255),      None, (("b", (6, 11), 5, 256.0),), 1, False, False),
    "bytes_query_256": (L2, 30,  (0, 255),       (0, 255),      None, (("q", 1, 9, 256.0),), 1, False, False),
    "bytes_255_5":     (L2, 100, (0, 255),       (0, 255),      None, (("q", 1, 9, 255.5),), 0, False, False),
    # the coarse side by itself: scan_arith() speaks of the list scan alone, the coarse ranking is judged by its bits
    "coarse_out":      (L2, 16,  (-1, 4095),     (-1, 4095),    (-2, 4095), (), 1, False, True),
    "coarse_in":       (L2, 128, (-2, 4095),     (-1, 4095),    (-1, 4095), (), 0, True, False),
    # (4097 * 4095 is exact; against queries inside the rule the first centroid value with an inexact product is 8193)
    "coarse_out_ip":   (IP, 100, (-4095, 4095),  (-4095, 4095), (-8193, 8193), (), 1, False, True),
}
NAMES = tuple(SPECS)
TEETH = tuple(n for n in NAMES if SPECS[n][7])
COARSE_TEETH = tuple(n for n in NAMES if SPECS[n][8])
INSIDE = tuple(n for n in NAMES if SPECS[n][6] == 1 and not SPECS[n][8] and not n.startswith("bytes"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ------------------------------------------------------------------------------------------------------------------ the rule
def rule_arith(metric, d, a, b):
    """the arithmetic a scan of operand sets a and b must choose -- written from the table above, not taken from the engine"""
    v = np.concatenate([np.ravel(a), np.ravel(b)]).astype(np.float64)
    if not (np.isfinite(v).all() and (v == np.trunc(v)).all()):
        return 0
    lo, hi = v.min(), v.max()
    if lo >= 0 and hi <= 255 and d * hi * hi <= BYTE_LIMIT:
        return 2
    if max(-lo, hi) > MAG:
        return 0
    if metric == L2 and hi - lo > EDGE:
        return 0
    return 1


def rule_fused(metric, d, a, b):
    """whether fp32 sums over a and b may be fused (the coarse ranking has no byte form: its arithmetic 2 is 1)"""
    return rule_arith(metric, d, a, b) >= 1


# ----------------------------------------------------------------------------------------------------------------- the model
def model_dist(metric, xq, xb, fused):
    """(nq, nb) float32 distances in the scan's summation order, fused or not"""
    xq, xb = np.asarray(xq, np.float32), np.asarray(xb, np.float32)
    d = xq.shape[1]
    pad = -d % 4
    if pad:
        xq = np.concatenate([xq, np.zeros((xq.shape[0], pad), np.float32)], axis=1)
        xb = np.concatenate([xb, np.zeros((xb.shape[0], pad), np.float32)], axis=1)
    acc = np.zeros((xq.shape[0], xb.shape[0], 4), np.float32)
    for s in range(0, d + pad, 4):
        q, y = xq[:, None, s:s + 4], xb[None, :, s:s + 4]
        if metric == L2:
            a = b = (q - y).astype(np.float32)  # (one rounding, as the reference's subtraction)
        else:
            a, b = np.broadcast_arrays(q, y)
        if fused:
            acc = (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
        else:
            acc = acc + (a * b).astype(np.float32)
    return (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])


def oracle_table(metric, xq, xb):
    """(nq, nb) distances of the pinned oracle (its per-pair kernel), by database row"""
    from oracle import pyoracle
    D, I = pyoracle.knn(metric, xq, xb, xb.shape[0])
    out = np.empty_like(D)
    np.put_along_axis(out, I, D, axis=1)
    return out


# ----------------------------------------------------------------------------------------------------------------- the cases
def draw(rs, n, d, lo, hi):
    """integers lo .. hi, half of the coordinates at lo or hi"""
    v = rs.randint(lo, hi + 1, size=(n, d))
    ext = rs.rand(n, d) < 0.5
    v[ext] = np.where(rs.rand(int(ext.sum())) < 0.5, lo, hi)
    return v.astype(np.float32)


def corners(d, q_range, b_range):
    """query 0 and the row of list 1: the four combinations of the two sides' extremes, coordinate by coordinate"""
    c = np.arange(d) % 4
    q = np.where(c < 2, q_range[1], q_range[0]).astype(np.float32)
    y = np.where(c % 2 == 0, b_range[1], b_range[0]).astype(np.float32)
    return q, y


def base_keys(rs, nq):
    """(nq, NPROBE): four lists a query in random order; query 0 probes list 1; every third query the three shortest lists and -1"""
    keys = np.stack([rs.permutation(NLIST)[:NPROBE] for _ in range(nq)]).astype(np.int64)
    keys[0] = [1, 0, 6, 2]
    for q in range(1, nq, 3):
        keys[q] = list(rs.permutation([0, 1, 2])) + [-1]
    return keys


def row_of(assign, l, offset):
    """the database row at `offset` of list l (lists hold their rows in database order)"""
    return int(np.nonzero(assign == l)[0][offset])


@functools.lru_cache(maxsize=None)
def case(name):
    metric, d, b_range, q_range, c_range, pokes, arith, teeth, coarse_teeth = SPECS[name]
    rs = np.random.RandomState(4096 + 17 * NAMES.index(name))
    assign = rs.permutation(np.repeat(np.arange(NLIST), LENGTHS)).astype(np.int64)
    xb = draw(rs, len(assign), d, *b_range)
    xq = draw(rs, NQ, d, *q_range)
    cen = draw(rs, NLIST, d, *(c_range or b_range))
    if pokes == "negzero":  # zeros of either sign are the same operand: -0.0 sprinkled over all three sets
        for a in (xb, xq, cen):
            a[rs.rand(*a.shape) < 0.05] = -0.0
        xb[row_of(assign, 6, 0), :4] = -0.0
        pokes = ()
    xq[0], xb[row_of(assign, 1, 0)] = corners(d, q_range, b_range)
    for side, row, col, value in pokes:
        if side == "q":
            xq[row, col] = value
        elif side == "c":
            cen[row, col] = value
        else:
            xb[row_of(assign, *row), col] = value
    keys = base_keys(rs, NQ)
    freeze(assign, xb, xq, cen, keys)
    return dict(name=name, metric=metric, d=d, nlist=NLIST, assign=assign, xb=xb, xq=xq, cen=cen, keys=keys, arith=arith, teeth=teeth,
                coarse_teeth=coarse_teeth, b_range=b_range, q_range=q_range)


def oracle_lists(c, xb=None, assign=None, ids=None):
    from oracle import pyoracle
    return pyoracle.Lists(c["metric"], c["cen"], c["xb"] if xb is None else xb, c["assign"] if assign is None else assign, ids)


@functools.lru_cache(maxsize=None)
def expected(name, nq, k, store_pairs=False):
    """the oracle's (D, I, stats) of the case's first nq queries under its keys"""
    from oracle import pyoracle
    c = case(name)
    D, I, st = pyoracle.search_preassigned(oracle_lists(c), c["xq"][:nq], k, c["keys"][:nq], np.zeros((nq, NPROBE), np.float32),
                                           store_pairs=store_pairs)
    freeze(D, I, st)
    return D, I, st


@functools.lru_cache(maxsize=None)
def expected_ranked(name, nq, k, nprobe=NPROBE):
    """... under the oracle's own coarse ranking -> (coarse_dis, keys, D, I, stats)"""
    from oracle import pyoracle
    c = case(name)
    cd, ck = pyoracle.knn(c["metric"], c["xq"][:nq], c["cen"], nprobe)
    D, I, st = pyoracle.search_preassigned(oracle_lists(c), c["xq"][:nq], k, ck, cd)
    freeze(cd, ck, D, I, st)
    return cd, ck, D, I, st


def returned_pairs_that_differ(c, D, I, table):
    """how many returned (query, id) of an oracle result (ids = database rows) carry other bits in `table` (a model's distances)"""
    ok = I >= 0
    q = np.nonzero(ok)[0]
    return int((bits(table[q, I[ok]]) != bits(D[ok])).sum())


# ---------------------------------------------------------------------------------------- ranges over the handle's life
# An inside-rule index (the case below) and one row that widens the spread to 4097: half of its coordinates at -2 or 4095.  It
# goes to list 1 by add(), or over entry 5 of list 2 by update_lists(); the queries that probe the three shortest lists only
# return every row of them at k = 100, this one included.
LIFE_CASE, LIFE_K, LIFE_ID, LIFE_LIST, LIFE_OVERWRITE = "l2_lo_m1", 100, 900000, 1, (2, 5)


@functools.lru_cache(maxsize=None)
def life():
    c = case(LIFE_CASE)
    rs = np.random.RandomState(777)
    w = draw(rs, 1, c["d"], -2, 4095)
    w[0, :2] = [-2, 4095]
    # add(): the row behind the others, in list 1
    xb_add = np.concatenate([c["xb"], w])
    assign_add = np.concatenate([c["assign"], [LIFE_LIST]]).astype(np.int64)
    ids_add = np.concatenate([np.arange(len(c["xb"])), [LIFE_ID]]).astype(np.int64)
    # update_lists(): the row over an entry of list 2, under that entry's id
    over = row_of(c["assign"], *LIFE_OVERWRITE)
    xb_upd = c["xb"].copy()
    xb_upd[over] = w[0]
    freeze(w, xb_add, assign_add, ids_add, xb_upd)
    return dict(w=w, xb_add=xb_add, assign_add=assign_add, ids_add=ids_add, over=over, xb_upd=xb_upd)


@functools.lru_cache(maxsize=None)
def life_expected(state, nq=NQ, k=LIFE_K):
    """the oracle's (D, I, stats) over the lists in `state`: "base", "added" (the widening row in list 1), "updated" (over an
    entry of list 2)"""
    from oracle import pyoracle
    c, f = case(LIFE_CASE), life()
    if state == "added":
        lists = oracle_lists(c, f["xb_add"], f["assign_add"], f["ids_add"])
    elif state == "updated":
        lists = oracle_lists(c, f["xb_upd"])
    else:
        lists = oracle_lists(c)
    D, I, st = pyoracle.search_preassigned(lists, c["xq"][:nq], k, c["keys"][:nq], np.zeros((nq, NPROBE), np.float32))
    freeze(D, I, st)
    return D, I, st


# ---------------------------------------------------------------------------------------------------------- resident queries
@functools.lru_cache(maxsize=None)
def resident_rows():
    """the queries of LIFE_CASE and, behind them, one row that alone breaks the rule (a -2: spread 4097 against the lists' 4095)"""
    c = case(LIFE_CASE)
    last = draw(np.random.RandomState(778), 1, c["d"], -2, 4095)
    last[0, :2] = [-2, 4095]
    x = np.concatenate([c["xq"], last])
    freeze(x)
    return x


# ------------------------------------------------------------------------------------------------------- radii on teeth pairs
def probed_mask(assign, keys):
    """(nq, nb) bool: the rows a query scans under `keys`"""
    hit = np.zeros((keys.shape[0], NLIST), bool)
    q, p = np.nonzero(keys >= 0)
    hit[q, keys[q, p]] = True
    return hit[:, assign]


@functools.lru_cache(maxsize=None)
def model_tables(name, nq):
    """(oracle table, fused model) of the case's first nq queries against its rows"""
    c = case(name)
    want, fused = oracle_table(c["metric"], c["xq"][:nq], c["xb"]), model_dist(c["metric"], c["xq"][:nq], c["xb"], True)
    freeze(want, fused)
    return want, fused


def radius_on_teeth(metric, want, fused):
    """A radius over candidate pairs (their oracle distances and fused sums) and whether a fused sum would change the result.  The
    reference keeps dis < radius (L2) / dis > radius (inner product).  Of the pairs whose fused sum has other bits, the one nearest
    the median distance (a result of about half the candidates) gives the radius: the larger of its two values under L2, the
    smaller under the inner product -- so the pair is kept at one of the two values and left out at the other.  Without such a
    pair (no teeth) the radius is the median."""
    differ = np.nonzero(bits(want) != bits(fused))[0]
    med = float(np.median(want))
    if len(differ) == 0:
        return float(np.float32(med)), False
    j = differ[np.argmin(np.abs(want[differ].astype(np.float64) - med))]
    return float(max(want[j], fused[j]) if metric == L2 else min(want[j], fused[j])), True


def flipping_radius(name, nq, keys):
    """radius_on_teeth over the pairs the case's first nq queries probe under `keys`"""
    c = case(name)
    want, fused = model_tables(name, nq)
    pm = probed_mask(c["assign"], keys)
    return radius_on_teeth(c["metric"], want[pm], fused[pm])
