"""Data, round schedules and a numpy model for the tests of the adaptive search over float lists through many filter rounds
(test_gpu_adaptive_filter.py; the preconditions are asserted without a GPU by test_adaptive_filter_cases_cpu.py).  numpy only; the
oracle is passed in by the caller and the engine is never imported here.

The round schedule.  In a tuned search over float lists with the filter on, run_rounds_device does not take the options alone:
  first round   filter_first_probes(index, K, 64, 0.015) = clamp(ceil(K / (0.015 sum(len^2) / sum(len))), 1, 16) probes, whatever
                "round_first" says; AUNCEL_AMD_FILTER_FIRST (read per call) is the only way to set it
  later rounds  plan_counts_query: an unfired query at stage s goes to max(floor((s + 1) multipler), floor(s max(multipler, grow)),
                s + inc), grow = "round_grow" (6 where unset), inc = "round_inc" (12 where unset)
  the reference a query fires at a stage t <= nlist / 8 and stops at floor(t multipler): with multipler = 1 it stops where it fires,
                my_nprobe <= nlist / 8, and an unfired query's target is s + 1 at the least
So the options force one probe a round only with multipler = 1 and the first round set through the environment; every schedule
here does both and sets "round_first" to the same value.  Under the default rule the shapes of these tests (K = 20 over lists of
~ 100) would scan 14 probes densely, more than the nlist / 8 = 8 a query can run: no filter round at all.  stages() restates the
schedule in effect; a query that the oracle stops at probe p takes part in the rounds up to the first whose stage reaches p, so a
call needs at least rounds_floor() planning passes, and all but the first (dense) round go through the filter."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import coarse_pick_cases as cp
import filter_bound_cases as fb

L2, IP = 1, 0
TOTAL_FIRST = 64  # the nprobe filter_first_probes is called with in a tuned search

# name -> (AUNCEL_AMD_FILTER_FIRST and "round_first", "round_grow", "round_inc"); None: unset (the engine's own rule)
SCHEDULES = {"default": (None, None, None), "one_probe": (1, 1, 1), "three_two": (3, 2, 1), "one_round": (64, 1, 1)}


def default_first(K, sizes):
    """filter_first_probes(index, K, 64, 0.015)"""
    s = np.asarray(sizes, dtype=np.float64)
    probed = max(1.0, float((s * s).sum() / s.sum()))
    return max(1, min(int(math.ceil(K / (0.015 * probed))), max(1, TOTAL_FIRST // 4)))


def stages(schedule, K, sizes, nlist):
    """the stage an unfired query stands at after every round (multipler = 1)"""
    first, grow, inc = SCHEDULES[schedule]
    first = default_first(K, sizes) if first is None else min(first, TOTAL_FIRST)
    grow = 6.0 if grow is None else float(grow)
    inc = 12 if inc is None else inc
    out, s = [], 0
    while s < nlist:
        s = min(nlist, max(s + 1, int(s * max(1.0, grow)), s + (first if s == 0 else inc)))
        out.append(s)
    return out


def rounds_floor(schedule, K, sizes, nlist, my_nprobe):
    """the rounds the query that stops last takes part in"""
    last = int(np.max(my_nprobe))
    assert 1 <= last <= nlist // 8  # (multipler = 1)
    return 1 + next(i for i, s in enumerate(stages(schedule, K, sizes, nlist)) if s >= last)


# ------------------------------------------------------------------------------------------ traces
def ntraces(nlist):
    n = 1
    while (1 << n) <= nlist // 8:
        n += 1
    return n


def random_traces(rs, nlist):
    """as test_gpu_random_adaptive.py draws them: predicted recalls on both sides of the bounds a call mixes"""
    traces = []
    for _ in range(ntraces(nlist)):
        n = int(rs.randint(3, 60))
        x = np.sort(rs.rand(n) * 25.0).astype(np.float32)
        x += np.arange(n, dtype=np.float32) * 1e-3  # strictly ascending
        traces.append((x, (0.5 + rs.rand(n) * 2.5).astype(np.float32), (rs.rand(n) * 0.5).astype(np.float32)))
    return traces


def stepped_traces(nlist, recalls=(0.55, 0.65, 0.75, 0.85, 0.85, 0.85)):
    """trace i predicts a k-scaling of 1 / recalls[i] at every angle.  The rule reads trace ceil(log2(stage)) and, at query_topk = 10,
    makes of it a recall of floor(10 recalls[i] + 1) / 10: 0.6 at stage 1, 0.7 at 2, 0.8 at 3 and 4, 0.9 from 5 on.  A query fires at
    the first stage whose recall reaches its bound, so a call that mixes bounds from 0.5 to 0.99 stops its queries at 1, 2, 3 and 5
    probes and, the bounds above 0.9, at nlist / 8 (or where their k-th distance has stood for floor(12 bound) probes).  At
    query_topk = 1 the prediction is 0 and every query runs that far."""
    x = (np.arange(8, dtype=np.float32) + 1) * 3
    return [(x, np.full(8, 1.0 / recalls[i], np.float32), np.zeros(8, np.float32)) for i in range(ntraces(nlist))]


def steep_traces(nlist):
    """a k-scaling of 3 at every angle: the predicted recall stays near 1 / 3, below every bound, and no query fires before
    stage nlist / 8 (the rule's other way to fire, a k-th distance unchanged for floor(12 bound) probes, needs 6 at the least)"""
    x = (np.arange(8, dtype=np.float32) + 1) * 3
    return [(x, np.full(8, 3.0, np.float32), np.zeros(8, np.float32)) for _ in range(ntraces(nlist))]


def case(metric, cen, assign, xb, xq, K, traces, req, std_m=0.0):
    for a in (cen, assign, xb, xq, req):
        a.setflags(write=False)
    return SimpleNamespace(metric=metric, nlist=cen.shape[0], d=cen.shape[1], K=K, cen=cen, assign=assign, xb=xb, xq=xq, traces=traces,
                           req=req, multipler=1.0, std_m=std_m, sizes=np.bincount(assign, minlength=cen.shape[0]))


def mixed_bounds(rs, nq):
    return rs.choice([0.5, 0.8, 0.9, 0.95, 0.99], size=nq).astype(np.float32)


# ------------------------------------------------------------------------------------------ 1. every filter kernel form
FORM_D = [20, 64, 96, 128, 136, 200, 520]  # 4, 8, 12, 16 register-resident pieces; the workgroup form beyond 128 dimensions
FORM_NARROW_D = [136]                      # ... and the one-wave form there
FORM_K, FORM_NLIST, FORM_NB = 20, 64, 6000
# (queries, centres they are drawn around): ~ 19, ~ 37 and ~ 130 queries meet on a list -> 1, 2 and 4 (+ 1) query blocks an item
FORM_LAYOUTS = ((150, 8), (150, 4), (260, 2))


def clustered(rs, nb, nq, d, nlist, few, spread=0.35, stray=0.3):
    """test_gpu_filter.py's data, the queries around the first `few` of the centres that hold vectors; a share `stray` of the vectors
    is stored in a list drawn at random instead of its blob's, so that the probes behind the first hold true neighbours and what the
    later rounds rescore enters the results (in many dimensions Gaussian blobs do not overlap, however wide)"""
    cen = rs.randn(nlist, d).astype(np.float32)
    assign = rs.randint(0, nlist, size=nb)
    assign[assign == 1] = 0          # an empty list and a long one
    xb = (cen[assign] + spread * rs.randn(nb, d)).astype(np.float32)
    away = (rs.rand(nb) < stray) & (assign != 0)  # (list 0 stays the long one)
    assign = np.where(away, rs.randint(2, nlist, size=nb), assign)
    near = np.array([l for l in range(nlist) if l != 1][:few])
    xq = (cen[near[rs.randint(0, few, size=nq)]] + spread * rs.randn(nq, d)).astype(np.float32)
    return cen, assign, xb, xq


@functools.lru_cache(maxsize=4)
def form_case(d, layout):
    nq, few = FORM_LAYOUTS[layout]
    rs = np.random.RandomState(8000 + 10 * d + layout)
    cen, assign, xb, xq = clustered(rs, FORM_NB, nq, d, FORM_NLIST, few)
    return case(L2, cen, assign, xb, xq, FORM_K, stepped_traces(FORM_NLIST), mixed_bounds(rs, nq), std_m=1.0)


# ------------------------------------------------------------------------------------------ 2. schedule invariance, 6. inner product
def unit_blobs(rs, nb, nq, d, nlist, short=None):
    """unit-norm blobs scaled by 0.9 (test_gpu_random_adaptive.py's "unit" kind), a list per blob; short = (list, length): that list
    keeps `length` vectors"""
    centres = rs.rand(nlist, d)

    def draw(which):
        x = centres[which] - 0.5 + rs.randn(len(which), d) * 0.15
        return (x / np.linalg.norm(x, axis=1, keepdims=True) * 0.9).astype(np.float32)
    assign = rs.randint(0, nlist, size=nb)
    if short is not None:
        extra = np.nonzero(assign == short[0])[0][short[1]:]
        assign[extra] = (short[0] + 1) % nlist
    xb = draw(assign)
    qlist = rs.randint(0, nlist, size=nq)
    if short is not None:
        qlist[0] = short[0]
    xq = draw(qlist)
    c = centres - 0.5
    cen = (c / np.linalg.norm(c, axis=1, keepdims=True) * 0.9 + rs.randn(nlist, d) * 1e-3).astype(np.float32)  # no exact coarse ties
    return cen, assign, xb, xq


IP_CASES = [(64, 5), (64, 10), (96, 5), (96, 10)]  # (d, K)
IP_NLIST, IP_NB, IP_NQ = 64, 8000, 150


@functools.lru_cache(maxsize=4)
def ip_case(d, K, short=False):
    rs = np.random.RandomState(8300 + d + K)
    cen, assign, xb, xq = unit_blobs(rs, IP_NB, IP_NQ, d, IP_NLIST, short=(7, K - 1) if short else None)
    return case(IP, cen, assign, xb, xq, K, stepped_traces(IP_NLIST), mixed_bounds(rs, IP_NQ), std_m=1.0)


SCHEDULE_NLIST = {L2: 256, IP: 64}


@functools.lru_cache(maxsize=2)
def schedule_case(metric):
    if metric == IP:
        return ip_case(64, 10)
    rs = np.random.RandomState(8200)
    nlist, nb, nq, d = SCHEDULE_NLIST[L2], 12000, 150, 64
    cen = rs.randn(nlist, d).astype(np.float32)
    assign = rs.randint(0, nlist, size=nb)
    xb = (cen[assign] + 0.35 * rs.randn(nb, d)).astype(np.float32)
    xq = (cen[rs.randint(0, nlist, size=nq)] + 0.35 * rs.randn(nq, d)).astype(np.float32)
    return case(L2, cen, assign, xb, xq, 10, steep_traces(nlist), np.full(nq, 0.99, np.float32))


# ------------------------------------------------------------------------------------------ 3. queries that stop at different rounds
MIXED_NLIST = 64


@functools.lru_cache(maxsize=1)
def mixed_case():
    rs = np.random.RandomState(8400)
    nlist, nb, nq, d = MIXED_NLIST, 6000, 200, 32
    cen = rs.randn(nlist, d).astype(np.float32)
    assign = rs.randint(0, nlist, size=nb)
    xb = (cen[assign] + 1.0 * rs.randn(nb, d)).astype(np.float32)  # (blobs that overlap: a stop after one probe misses neighbours)
    xq = (cen[rs.randint(0, nlist, size=nq)] + 1.0 * rs.randn(nq, d)).astype(np.float32)
    req = np.linspace(0.5, 0.99, nq).astype(np.float32)[rs.permutation(nq)]
    return case(L2, cen, assign, xb, xq, 10, stepped_traces(nlist), req, std_m=1.0)


# ------------------------------------------------------------------------------------------ 4. thresholds that shrink onto candidates
COPIES_D = [32, 96, 200]
COPIES_NLIST, COPIES_K = 64, 12


@functools.lru_cache(maxsize=3)
def copies_case(d):
    """test_gpu_filter.py's test_candidates_on_and_next_to_the_threshold over 64 lists (a tuned search reads nlist / 8 + 20 entries
    of a ranking, more than 16 lists have): every vector three times and four times more with one coordinate moved by an ulp, the
    copies spread over the lists, so that every round meets candidates on, or an ulp from, the query's current k-th distance.  L2
    only: the reference's inner-product rule needs arccos of the distances, and these rows are no unit vectors."""
    rs = np.random.RandomState(8500 + d)
    nlist, nq = COPIES_NLIST, 160
    cen = rs.randn(nlist, d).astype(np.float32)
    seeds = (cen[rs.randint(0, nlist, size=300)] + 0.3 * rs.randn(300, d)).astype(np.float32)
    rows = []
    for v in seeds:
        for _ in range(3):
            rows.append(v)
        for _ in range(4):
            w = v.copy()
            c = rs.randint(0, d)
            w[c] = np.nextafter(w[c], np.float32(np.inf if rs.rand() < 0.5 else -np.inf), dtype=np.float32)
            rows.append(w)
    xb = np.stack(rows).astype(np.float32)
    xb = xb[rs.permutation(len(xb))]
    assign = rs.randint(0, nlist, size=len(xb))
    xq = (seeds[rs.randint(0, len(seeds), size=nq)] + 0.05 * rs.randn(nq, d)).astype(np.float32)
    return case(L2, cen, assign, xb, xq, COPIES_K, steep_traces(nlist), np.full(nq, 0.99, np.float32))


# ------------------------------------------------------------------------------------------ 5. the bound under shrinking thresholds
BOUND_D = [64, 128, 136]
BOUND_NLIST, BOUND_N, BOUND_NB, BOUND_K = 64, 256, 4000, 10
# queries that lose an entry their heap would admit, in some round, under the fp32 form's constant: what the model gives is at
# least this for every d: 246, 251 and 252 of 256 at d = 64, 128, 136 (test_adaptive_filter_cases_cpu.py prints the figures)
BOUND_FP32_LOSES = 240


@functools.lru_cache(maxsize=3)
def bound_case(d):
    """coarse_pick_cases.coherent's rows (every query rounds down in the cast to fp16, half of the stored rows too) over 64 lists,
    uniformly; no query fires before stage 8"""
    cen, xq, xb = cp.coherent(d, BOUND_NLIST, BOUND_N, 1024, nb=BOUND_NB)
    assign = np.random.RandomState(8600 + d).randint(0, BOUND_NLIST, size=BOUND_NB)
    return case(L2, cen.copy(), assign, xb.copy(), xq.copy(), BOUND_K, steep_traces(BOUND_NLIST), np.full(BOUND_N, 0.99, np.float32))


def bound_report(oracle, c, ref):
    """The keep rule per round, one probe a round: round r (1 ..) filters the list of probe r with the k-th distance of the oracle's
    heap after probes 0 .. r - 1.  -> (entries within the threshold that the real constant drops, queries that lose such an entry in
    some round under the fp32 form's constant, the rounds in which one does)"""
    C, F = cp.half_constant(c.d, False), cp.fp32_constant(c.d)
    exact = cp.exact_distances(c.metric, c.xq, c.xb)
    approx = fb.approx_product(c.xq, c.xb)
    xn, yn = fb.norms(c.metric, c.xq), fb.norms(c.metric, c.xb)
    lists = oracle.Lists(c.metric, c.cen, c.xb, c.assign)
    lost_real, loses, rounds = 0, np.zeros(len(c.xq), bool), set()
    for r in range(1, int(ref.my_nprobe.max())):
        D, I, _ = oracle.search_preassigned(lists, c.xq, c.K, ref.ck[:, :r], ref.cd[:, :r])
        assert (I[:, c.K - 1] >= 0).all()
        tau = D[:, c.K - 1]
        met = (c.assign[None, :] == ref.ck[:, r][:, None]) & (ref.my_nprobe > r)[:, None] & fb.within(c.metric, exact, tau)
        lost_real += int((met & ~fb.keep(c.metric, C, approx, xn, yn, tau)).sum())
        bad = (met & ~fb.keep(c.metric, F, approx, xn, yn, tau)).any(axis=1)
        loses |= bad
        if bad.any():
            rounds.add(r)
    return lost_real, int(loses.sum()), sorted(rounds)


# ------------------------------------------------------------------------------------------ 7. entry points, 8. scale edge
@functools.lru_cache(maxsize=1)
def entry_case():
    return form_case(96, 1)


@functools.lru_cache(maxsize=1)
def scale_case():
    """one query row scaled by 2^50 (test_gpu_filter.py's test_fp16_form_without_a_usable_scale): the queries have no usable fp16 scale"""
    rs = np.random.RandomState(8800)
    cen, assign, xb, xq = clustered(rs, 4000, 150, 64, 64, 8)
    xq[17] *= np.float32(2.0 ** 50)
    return case(L2, cen, assign, xb, xq, 10, steep_traces(64), np.full(150, 0.99, np.float32))


# ------------------------------------------------------------------------------------------ the oracle's answer
_REFERENCE = {}


def reference(oracle, arcos, key, c, query_topk, profile=False):
    """the oracle's answer to one adaptive call over its own coarse ranking, computed once per (case, query_topk, profile) and
    left unchanged.  Raises what the oracle raises."""
    key = (key, query_topk, profile)
    if key not in _REFERENCE:
        nq = len(c.xq)
        lists = oracle.Lists(c.metric, c.cen, c.xb, c.assign)
        cd, ck = oracle.knn(c.metric, c.xq, c.cen, c.nlist, nthreads=8)
        gtD, _ = oracle.knn(c.metric, c.xq, c.xb, c.K, nthreads=8)
        tun = oracle.Tuner(oracle.interdis(c.metric, c.cen), c.traces, c.K, nq, arcos=arcos)
        stt = tun.struct(query_topk, c.req, c.multipler, c.std_m, gt_D=gtD, profile=profile)
        D, I, st = oracle.search_preassigned(lists, c.xq, c.K, ck, cd, tuner=stt, offset=0, nthreads=1)
        out = SimpleNamespace(D=D, I=I, stats=[int(v) for v in st], my_nprobe=tun.my_nprobe.astype(np.int64).copy(),
                              t_recalls=tun.t_recalls.copy(), ck=ck, cd=cd, gtD=gtD)
        for a in (out.D, out.I, out.my_nprobe, out.t_recalls, out.ck, out.cd, out.gtD):
            a.setflags(write=False)
        if len(_REFERENCE) >= 12:
            _REFERENCE.clear()
        _REFERENCE[key] = out
    return _REFERENCE[key]
