"""The `_dev` entry points where the cores leave their common path ("Where the results are stored").
tests/test_gpu_device_io.py stays, at 16 or 32 lists and nprobe = 4, on the one path where the selection kernel stores straight into
the caller's tensors; here every other place of ivf_engine.hip that writes (D, I) under amd_ivf::dev_out is reached, and every test
holds a witness that it was: a comparison in which nothing unusual happened proves nothing.

The comparison is always the same: (D, I) of the `_dev` call, copied back, are the host-pointer call's on the same handle with the
same options, byte for byte -- and so are scan_arith, last_exact, last_exact_detail, my_nprobe, the bits of t_recalls, the statistics
(reset before each side), last_tie_redone and last_tie_patched.  The host call is pinned against the CPU oracle by
test_gpu_coarse_ties.py, test_gpu_exact*.py, test_gpu_budget_cut.py and test_gpu_select_forms.py; the adaptive calls are compared with
the oracle here as well.

1. adaptive search above 128 lists (integer grid data, 20000 vectors, nlist 136 / 256, K 10 / 100): calls of 1, 5 and 19 queries that
   are repeated with the heap's tie order (and one of 1 query that is not), calls of 20 and 60 under coarse_ties 2 / 1 / 0 -- searched
   again (nlist 136: the one case in which result bytes cross the bus) and patched in flight (nlist 256);
2. the exact call: flagged queries in more than one run (byte values 0 .. 15, d = 20; tests/golden/fixed_dups), candidate overflow
   (a child under AUNCEL_AMD_EXACT_CAP=16), two slices (8193 queries), an empty index, the optional list passes;
3. fixed nprobe off the single dense round (the ragged and tie-heavy worlds of test_gpu_budget_cut.py, 1024 queries, every list):
   two rounds, heap selection, eager and final tie fix, and the planner's cut in children under its knobs;
4. subset, joined, updated and cloned handles; 5. search_dev of the class mirror (tests/cpp/device_io_driver.cpp).

Measured on an MI355X: the module's 49 cases take 12 s, of which the four children take 7 s (1.3 s without a knob, 2.3 s and 2.4 s under
the planner's knobs, 1.2 s under the exact call's) -- and 20 s more where it is the first module to build the class mirror."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from test_gpu_budget_cut import FATAL, build_cases
from test_gpu_coarse_ties import grid_points
from test_gpu_device_io import FMAX, IP, L2, bits, new_handle, same, to_gpu, world
from test_gpu_exact import exact_ties
from util import load_case

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "device_io_paths_child.py")
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "device_io_driver.cpp")
SENT_D, SENT_I = 12345.5, -777


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def snapshot(h):
    """what a call leaves on its handle besides (D, I)"""
    return dict(arith=h.scan_arith(), exact=h.last_exact(), detail=h.last_exact_detail(), stats=h.stats(), redone=h.last_tie_redone(),
                patched=h.last_tie_patched())


def framed(torch, n, k):
    """n result rows inside larger tensors; the rows themselves hold the sentinel too: a row that no pass wrote is seen"""
    bigD = torch.full((n + 6, k), SENT_D, dtype=torch.float32, device="cuda")
    bigI = torch.full((n + 6, k), SENT_I, dtype=torch.int64, device="cuda")
    return bigD, bigI, (bigD[3:3 + n], bigI[3:3 + n])


def frame_untouched(bigD, bigI, n, tag):
    for part in (bigD[:3], bigD[3 + n:]):
        assert bool((part == SENT_D).all()), tag
    for part in (bigI[:3], bigI[3 + n:]):
        assert bool((part == SENT_I).all()), tag


def runs_of(flags):
    f = np.asarray(flags, dtype=bool)
    return int(f[0]) + int((f[1:] & ~f[:-1]).sum()) if len(f) else 0


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the adaptive call above 128 lists
# ------------------------------------------------------------------------------------------------------------------------------
NQ_AD = 60
# query of each world that reads into no run of equal coarse distances under (query_topk 10, multipler 1, std_m 0), found with the
# oracle alone (first run at or past 2 my_nprobe + 14, and 2 my_nprobe + 15 below what the first pass ranks); query 0 of every world
# reads into one
NO_RUN = {(136, 10): 2, (136, 100): 1, (256, 10): 3, (256, 100): 21}
_AD = {}


def adaptive_world(oracle, capi, nlist, K):
    """the data recipe of test_gpu_coarse_ties.py's adaptive test: made once per shape and never changed"""
    if (nlist, K) not in _AD:
        rs = np.random.RandomState(9300 + nlist + K)
        d, nb = 16, 20000
        xb, xq = grid_points(rs, nb, d, 12), grid_points(rs, NQ_AD, d, 12)
        cen = xb[rs.choice(nb, nlist, replace=False)].copy()
        ntr = 1
        while (1 << ntr) <= nlist // 8:
            ntr += 1
        traces = []
        for _ in range(ntr):
            n = int(rs.randint(3, 60))
            x = np.sort(rs.rand(n) * 25.0).astype(np.float32)
            x += np.arange(n, dtype=np.float32) * 1e-3
            traces.append((x, (0.5 + rs.rand(n) * 2.5).astype(np.float32), (rs.rand(n) * 0.5).astype(np.float32)))
        req = rs.choice([0.8, 0.9, 0.95, 0.99], size=NQ_AD).astype(np.float32)
        _, a = oracle.knn(1, xb, cen, 1, nthreads=8)
        cd, ck = oracle.knn(1, xq, cen, nlist, nthreads=8)
        gtD, _ = oracle.knn(1, xq, xb, K, nthreads=8)
        eq = cd[:, 1:] == cd[:, :-1]
        first = np.where(eq.any(axis=1), eq.argmax(axis=1), nlist)  # where a query's first run of equal coarse distances starts
        w = dict(nlist=nlist, K=K, d=d, xb=xb, xq=xq, cen=cen, traces=traces, req=req, assign=a[:, 0].copy(), cd=cd, ck=ck, gtD=gtD,
                 first=first, lists=oracle.Lists(1, cen, xb, a[:, 0]), interdis=oracle.interdis(1, cen), arcos=capi.arcos_table())
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _AD[(nlist, K)] = w
    return _AD[(nlist, K)]


def adaptive_handle(capi, w):
    h = capi.Handle(w["d"], w["nlist"], 1, 0)
    h.set_centroids(w["cen"])
    h.set_lists_from_assign(w["xb"], w["assign"])
    h.set_interdis(None)
    h.set_tuner(w["K"], w["traces"], w["arcos"])
    return h


def oracle_adaptive(oracle, w, start, n, qk, mult, sm, profile):
    """the reference's result for queries start .. start + n as a call of their own, or the text it throws"""
    s = slice(start, start + n)
    tun = oracle.Tuner(w["interdis"], w["traces"], w["K"], n, arcos=w["arcos"])
    stt = tun.struct(qk, w["req"][s].copy(), mult, sm, gt_D=w["gtD"][s].copy(), profile=profile)
    try:
        eD, eI, est = oracle.search_preassigned(w["lists"], w["xq"][s], w["K"], w["ck"][s], w["cd"][s], tuner=stt, offset=0, nthreads=1)
    except RuntimeError:
        return None
    return eD, eI, list(est), tun.my_nprobe.astype(np.int64).copy()


def adaptive_pair(capi, torch, oracle, h, w, start, n, qk, mult, sm, profile=False, with_oracle=True):
    """the host call, then the `_dev` call into framed rows; everything equal.  Returns (my_nprobe of the call's queries, rise of
    coarse_tie_rows during the host call, last_dev_io), or None where the reference refuses the draw (both forms the same text)"""
    K, tag = w["K"], (w["nlist"], w["K"], start, n, qk, mult, sm, profile)
    np0, tr0 = np.zeros(NQ_AD, np.uint64), np.zeros(NQ_AD, np.float32)
    np1, tr1 = np.zeros(NQ_AD, np.uint64), np.zeros(NQ_AD, np.float32)
    h.set_queries(w["xq"])
    h.stats(reset=True)
    before = h.coarse_tie_rows()
    try:
        want, err = h.search_adaptive(start, n, qk, mult, sm, w["req"], np0, tr0, gt_D=w["gtD"], profile=profile), None
    except capi.EngineError as e:
        want, err = None, str(e)
    rose = h.coarse_tie_rows() - before
    snap = snapshot(h)
    h.set_queries(w["xq"][:1] * 0.5)  # (what the host call left resident must not be what the device call searches)
    h.set_queries_dev(to_gpu(torch, w["xq"]))
    bigD, bigI, out = framed(torch, n, K)
    h.stats(reset=True)
    if err is not None:
        with pytest.raises(capi.EngineError) as got:
            h.search_adaptive_dev(start, n, qk, mult, sm, w["req"], np1, tr1, gt_D=w["gtD"], profile=profile, out=out)
        assert str(got.value) == err, tag
        return None
    h.search_adaptive_dev(start, n, qk, mult, sm, w["req"], np1, tr1, gt_D=w["gtD"], profile=profile, out=out)
    io = h.last_dev_io()
    print(tag, "tie rows +", rose, "redone", h.last_tie_redone(), "patched", h.last_tie_patched(), "dev_io", io)
    same(out, want, tag)
    frame_untouched(bigD, bigI, n, tag)
    assert np.array_equal(np1, np0) and np.array_equal(bits(tr1), bits(tr0)), tag
    assert snapshot(h) == snap, (tag, snapshot(h), snap)
    assert io[0] == 0, (tag, io)
    if with_oracle:
        ref = oracle_adaptive(oracle, w, start, n, qk, mult, sm, profile)
        if ref is not None:
            assert np.array_equal(want[1], ref[1]) and np.array_equal(bits(want[0]), bits(ref[0])), tag
            assert np.array_equal(np0[start:start + n].astype(np.int64), ref[3]), tag
            assert [snap["stats"]["nlist"], snap["stats"]["ndis"], snap["stats"]["nheap_updates"]] == ref[2], tag
    return np0[start:start + n].astype(np.int64), rose, io


@gpu
@pytest.mark.parametrize("K", [10, 100])
@pytest.mark.parametrize("nlist", [136, 256])
def test_adaptive_small_call_taken_twice(capi, torch, oracle, monkeypatch, nlist, K):
    """n < 20: the call runs with centroid-number tie order and, where a query reads into a run of equal coarse distances, again
    with the heap's order over the same device buffers.  Witness: the run lies below 2 my_nprobe + 14 for a query of the call
    (from the oracle's ranking, on the CPU) and the host call re-ran rankings through the heap (coarse_tie_rows rose).  One draw
    per world reads into no run: one pass, nothing re-run."""
    monkeypatch.delenv("AUNCEL_AMD_COARSE_TIES", raising=False)
    w = adaptive_world(oracle, capi, nlist, K)
    h = adaptive_handle(capi, w)
    assert h.get_option("coarse_ties") == -1
    taken_twice = 0
    for start, n, expect_run in ((0, 1, True), (NO_RUN[(nlist, K)], 1, False), (0, 5, True), (0, 19, True), (41, 19, None)):
        got = adaptive_pair(capi, torch, oracle, h, w, start, n, 10, 1.0, 0.0)
        assert got is not None or expect_run is None, (start, n, "the reference refuses a draw picked for its witness")
        if got is None:
            continue
        my_np, rose, io = got
        reads = w["first"][start:start + n] < 2 * my_np + 14
        assert io[1] == 0 and io[3] == 1, io
        if expect_run is True:
            assert reads.any() and rose > 0, (start, n, reads, rose)
            taken_twice += 1
        elif expect_run is False:
            assert not reads.any() and rose == 0, (start, n, reads, rose)
    assert taken_twice == 3
    # the same under gt_D and profile on, and with the other tuner arguments
    adaptive_pair(capi, torch, oracle, h, w, 0, 19, 10, 1.0, 0.0, profile=True)
    adaptive_pair(capi, torch, oracle, h, w, 3, 5, 1, 2.0, 1.0)
    h.close()


@gpu
@pytest.mark.parametrize("K", [10, 100])
@pytest.mark.parametrize("nlist", [136, 256])
def test_adaptive_redo_searched_again_or_patched(capi, torch, oracle, monkeypatch, nlist, K):
    """n >= 20 under coarse_ties = 2: nlist 136 (no power of two) searches a few queries again with dev_out switched off and sends
    each row to its place host to device -- the one case in which result bytes cross the bus, 12 bytes an entry; nlist 256 patches
    the pass in flight.  coarse_ties 1 and 0 for the same calls besides."""
    monkeypatch.delenv("AUNCEL_AMD_COARSE_TIES", raising=False)
    w = adaptive_world(oracle, capi, nlist, K)
    h = adaptive_handle(capi, w)
    again = patched = 0
    for ties in (2, 1, 0):
        h.set_option("coarse_ties", ties)
        assert h.get_option("coarse_ties") == ties
        for n in (20, 60):
            for qk, mult, sm, profile in ((10, 1.0, 0.0, False), (1, 2.0, 1.0, False), (10, 1.0, 0.0, True)):
                if profile and (n != 60 or ties != 2):
                    continue
                # (centroid-number order, ties = 0, is the engine's own: the oracle restates the reference's heap)
                got = adaptive_pair(capi, torch, oracle, h, w, 0, n, qk, mult, sm, profile=profile, with_oracle=ties != 0)
                if got is None:
                    continue
                io = got[2]
                if ties != 2:
                    assert io[1] == 0 and io[3] == 1, io
                    continue
                redone, fixed = h.last_tie_redone(), h.last_tie_patched()
                assert io[1] == redone * K * 12, (io, redone)
                if nlist & (nlist - 1):
                    assert fixed == 0 and redone > 0, (n, qk, redone, fixed)
                    again += 1
                else:
                    assert fixed > 0, (n, qk, redone, fixed)
                    patched += 1
    assert (again if nlist & (nlist - 1) else patched) >= 4
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the exact call's second ways
# ------------------------------------------------------------------------------------------------------------------------------
_TIES = {}


def tie_world(metric):
    """byte values 0 .. 15 at d = 20, 3000 vectors in 16 lists: with k = 10 about half of 257 queries meet equal distances among
    their best k + 1, with k = 1 a handful -- in more than one run of consecutive queries either way (asserted where it is used)"""
    if metric not in _TIES:
        rs = np.random.RandomState(4100 + 15 + metric)
        nb, d, nlist, nq = 3000, 20, 16, 257
        xb = rs.randint(0, 16, size=(nb, d)).astype(np.float32)
        xq = rs.randint(0, 16, size=(nq, d)).astype(np.float32)
        cen = xb[rs.choice(nb, nlist, replace=False)].copy()
        assign = rs.randint(0, nlist, size=nb).astype(np.int64)
        for a in (xb, xq, cen, assign):
            a.setflags(write=False)
        _TIES[metric] = dict(d=d, nlist=nlist, metric=metric, xb=xb, xq=xq, cen=cen, assign=assign)
    return _TIES[metric]


def exact_pair(torch, h, xq, k, tag, out=None):
    """search_exact, then search_exact_dev; everything equal.  Returns (last_exact, last_exact_detail, last_dev_io)"""
    h.stats(reset=True)
    want = h.search_exact(xq, k)
    snap = snapshot(h)
    h.stats(reset=True)
    got = h.search_exact_dev(to_gpu(torch, xq), k, out=out)
    io = h.last_dev_io()
    print(tag, "last_exact", snap["exact"], "detail", snap["detail"], "dev_io", io)
    same(got, want, tag)
    assert snapshot(h) == snap, (tag, snapshot(h), snap)
    assert io[0] == 0 and io[1] == 0, (tag, io)
    return snap["exact"], snap["detail"], io, want


@gpu
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("metric", [L2, IP])
def test_exact_flagged_queries_in_several_runs(capi, torch, metric, k):
    """the queries in which equal distances meet leave the list pass and are searched the general way: under dev_out their rows come
    from w_ex_D / w_ex_I by one device copy per run of consecutive queries.  Which queries those are is known here from exact integer
    arithmetic (test_gpu_exact.py holds that the engine flags exactly these): more than one run, and not every query"""
    w = tie_world(metric)
    h = new_handle(capi, w)
    n = 257
    tied, within = exact_ties(metric, w["xb"], w["xq"], k)
    assert within.max() < 512 and 0 < tied.sum() < n and runs_of(tied) >= 2, (int(tied.sum()), runs_of(tied))
    bigD, bigI, out = framed(torch, n, k)
    last, det, io, want = exact_pair(torch, h, w["xq"], k, (metric, k), out=out)
    frame_untouched(bigD, bigI, n, (metric, k))
    assert last[1] == int(tied.sum()) and last[2] == 0 and last[0] == n - last[1], (last, int(tied.sum()))
    assert 0 < last[1] + last[2] < n and io[3] == 2, (last, io)
    assert det[0] == 1, det
    # the rows of the flagged queries are the general way's: search_preassigned over every list
    keys = np.tile(np.arange(w["nlist"], dtype=np.int64), (n, 1))
    pD, pI = h.search_preassigned(w["xq"], k, keys)
    assert np.array_equal(pI, want[1]) and np.array_equal(bits(pD), bits(want[0]))
    h.close()


@gpu
@pytest.mark.parametrize("k", [1, 10])
def test_exact_over_exact_duplicates(capi, torch, k):
    """tests/golden/fixed_dups: every stored vector has about sixteen copies, so every one of the 48 queries is flagged -- one run
    of all the call's rows"""
    case, gold = load_case("fixed_dups")
    h = capi.Handle(case["d"], case["nlist"], case["metric"], 0)
    h.set_centroids(case["centroids"])
    h.set_lists_from_assign(case["xb"], gold["assign"])
    n = len(case["xq"])
    tied, _ = exact_ties(case["metric"], case["xb"], case["xq"], k)
    last, det, io, _ = exact_pair(torch, h, case["xq"], k, ("dups", k))
    assert last[1] + last[2] == int(tied.sum()) == n and io[3] == 2, (last, io)
    h.close()


@gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_exact_two_slices(capi, torch, metric):
    """8193 queries: exact_core takes two slices, the second of one query, whose rows lie at D + 8192 k of a device pointer"""
    w = tie_world(metric)
    h = new_handle(capi, w)
    n = 8193
    xq = np.tile(w["xq"], (n // len(w["xq"]) + 1, 1))[:n].copy()
    bigD, bigI, out = framed(torch, n, 1)
    last, det, io, want = exact_pair(torch, h, xq, 1, (metric, "two slices"), out=out)
    frame_untouched(bigD, bigI, n, metric)
    assert sum(last[:3]) == n and 0 < last[1] + last[2] < n and io[3] == 2, (last, io)
    lastD, lastI = out[0][n - 1].cpu().numpy(), out[1][n - 1].cpu().numpy()
    assert np.array_equal(lastI, want[1][n - 1]) and np.array_equal(bits(lastD), bits(want[0][n - 1])) and lastI[0] >= 0
    # row 8192 is query 8192 % 257 of the world once more
    j = (n - 1) % len(w["xq"])
    assert np.array_equal(want[1][n - 1], want[1][j]) and np.array_equal(bits(want[0][n - 1]), bits(want[0][j]))
    h.close()


@gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_exact_empty_index(capi, torch, metric):
    """no stored vector: the reference's padding, -1 and +-FLT_MAX, set on the device inside the frame"""
    d, n, k = 20, 65, 10
    h = capi.Handle(d, 16, metric, 0)
    h.set_centroids(np.zeros((16, d), np.float32))
    xq = world(d, metric, "float")["xq"][:n]
    bigD, bigI, out = framed(torch, n, k)
    last, det, io, want = exact_pair(torch, h, xq, k, (metric, "empty"), out=out)
    frame_untouched(bigD, bigI, n, metric)
    assert last == (0, 0, n, 0) and io[3] == 2, (last, io)
    gD, gI = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert (gI == -1).all() and np.array_equal(bits(gD), bits(np.full((n, k), FMAX if metric == L2 else -FMAX, np.float32)))
    h.close()


@gpu
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("kind,d,data,options", [(2, 20, "float", ("exact_float",)), (3, 132, "float", ("exact_float", "exact_wide")),
                                                 (4, 132, "bytes", ("exact_wide_bytes",))])
def test_exact_optional_passes(capi, torch, kind, d, data, options, metric, k):
    """the list passes that are off by default; last_exact_detail says which one ran"""
    w = world(d, metric, data)
    h = new_handle(capi, w)
    for key in options:
        h.set_option(key, 1)
        assert h.get_option(key) == 1
    for n in (65, 257):
        last, det, io, _ = exact_pair(torch, h, w["xq"][:n], k, (kind, metric, k, n))
        assert det[0] == kind and last[0] > 0 and sum(last[:3]) == n and io[3] == 2, (last, det, io)
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. fixed nprobe off the single dense round
# ------------------------------------------------------------------------------------------------------------------------------
FIXED_WORLDS = ("B_bytes_l2", "B_float_l2", "D")
N_FIXED = 1024


@pytest.fixture(scope="module")
def cut_worlds(oracle):
    """the ragged (B) and tie-heavy (D) indexes of test_gpu_budget_cut.py, from its own builder; 1024 queries each (D's 64, tiled)"""
    c = build_cases(oracle)
    specs = {s["name"]: s for s in c.indexes}
    out = {}
    for name in FIXED_WORLDS:
        xq = c.arrays[name + "/xq_b"] if name != "D" else np.tile(c.arrays["D/xq"], (N_FIXED // 64, 1))
        assert xq.shape[0] == N_FIXED
        out[name] = dict(d=specs[name]["d"], nlist=specs[name]["nlist"], metric=specs[name]["metric"], cen=c.arrays[name + "/cen"],
                         xb=c.arrays[name + "/xb"], assign=c.arrays[name + "/assign"], xq=np.ascontiguousarray(xq))
    return out


def fixed_pair(torch, h, entry, xq, x, k, nprobe, keys, tag):
    h.stats(reset=True)
    if entry == "search":
        want = h.search(xq, k, nprobe)
    elif entry == "preassigned":
        want = h.search_preassigned(xq, k, keys)
    else:
        h.set_queries(xq)
        want = h.search_resident(0, len(xq), k, nprobe)
    snap, fixed, rounds = snapshot(h), h.last_tie_fixed(), h.last_timing()["rounds"]
    h.stats(reset=True)
    if entry == "search":
        got = h.search_dev(x, k, nprobe)
    elif entry == "preassigned":
        got = h.search_preassigned_dev(x, k, to_gpu(torch, keys))
    else:
        h.set_queries(xq[:1] * 0.5)
        h.set_queries_dev(x)
        got = h.search_resident_dev(0, len(xq), k, nprobe)
    io = h.last_dev_io()
    same(got, want, tag)
    assert snapshot(h) == snap, (tag, snapshot(h), snap)
    assert h.last_tie_fixed() == fixed and h.last_timing()["rounds"] == rounds, tag
    assert io[0] == 0 and io[1] == 0 and io[3] == 1, (tag, io)
    return fixed, rounds


@gpu
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("name", FIXED_WORLDS)
def test_fixed_nprobe_rounds_selection_and_tie_fix(capi, torch, cut_worlds, monkeypatch, name, k):
    """1024 queries over every list (16; the tie-heavy index has 7): one and two rounds, sorted and heap selection, final and eager
    tie fix, from each of the three entry points.  Witnesses: two rounds take more planning passes than one; get_option echoes the
    selection; on the tie-heavy index the sorted selection hands queries to tie_fix_kernel, which stores into the caller's rows"""
    for key in ("AUNCEL_AMD_FIXED_ROUNDS", "AUNCEL_AMD_SELECT", "AUNCEL_AMD_TIE_FIX"):
        monkeypatch.delenv(key, raising=False)
    w = cut_worlds[name]
    h = new_handle(capi, w)
    nprobe = min(16, w["nlist"])
    xq = w["xq"]
    x = to_gpu(torch, xq)
    keys = h.coarse(xq, nprobe)[1]
    for select in (1, 0):
        for tie_fix in (0, 1):
            for entry in ("search", "preassigned", "resident"):
                seen = {}
                for fixed_rounds in (1, 2):
                    for key, v in (("select", select), ("tie_fix", tie_fix), ("fixed_rounds", fixed_rounds)):
                        h.set_option(key, v)
                        assert h.get_option(key) == v
                    tag = (name, k, select, tie_fix, entry, fixed_rounds)
                    fixed, rounds = fixed_pair(torch, h, entry, xq, x, k, nprobe, keys, tag)
                    print(tag, "tie_fixed", fixed, "rounds", rounds)
                    seen[fixed_rounds] = rounds
                    if name == "D" and select == 1:
                        assert fixed > 0, tag
                assert seen[1] >= 1 and seen[2] > seen[1], (name, k, select, tie_fix, entry, seen)
    h.close()


def child_manifest(cut_worlds):
    """the fixed-nprobe calls of the children (the ragged byte index and the tie-heavy one) and the exact call that overflows"""
    arrays, indexes, calls = {}, [], []
    for name in ("B_bytes_l2", "D"):
        w = cut_worlds[name]
        indexes.append(dict(name=name, d=w["d"], nlist=w["nlist"], metric=w["metric"]))
        for f in ("cen", "xb", "assign"):
            arrays[f"{name}/{f}"] = w[f]
        arrays[name + "/xq"] = w["xq"]
        for k in (10, 100):
            for fixed_rounds in (1, 2):
                for select in (1, 0):
                    for entry in ("search", "preassigned", "resident"):
                        calls.append(dict(name=f"{name}_k{k}_r{fixed_rounds}_s{select}_{entry}", index=name, op=entry, xq=name + "/xq", k=k,
                                          nprobe=min(16, w["nlist"]), options=dict(fixed_rounds=fixed_rounds, select=select)))
    for metric, mname in ((L2, "l2"), (IP, "ip")):
        w = world(20, metric, "bytes")
        name = "X_" + mname
        indexes.append(dict(name=name, d=w["d"], nlist=w["nlist"], metric=metric))
        for f in ("cen", "xb", "assign"):
            arrays[f"{name}/{f}"] = w[f]
        arrays[name + "/xq"] = w["xq"]
        calls.append(dict(name=name + "_exact", index=name, op="exact", xq=name + "/xq", k=10, options=dict(exact_seed_nprobe=4)))
    return arrays, indexes, calls


CHILDREN = {"baseline": {}, "budget": {"AUNCEL_AMD_DIST_BUDGET_MB": "1"}, "pairs": {"AUNCEL_AMD_SEG_CAP_PAIRS": "256"},
            "exact_cap": {"AUNCEL_AMD_EXACT_CAP": "16"}}
# fields of a side's "state" array (device_io_paths_child.py)
ST_ARITH, ST_EXACT, ST_DETAIL, ST_STATS, ST_TIE_FIXED, ST_ROUNDS = 0, slice(1, 5), slice(5, 9), slice(9, 13), 13, 14


@pytest.fixture(scope="module")
def children(cut_worlds, tmp_path_factory):
    """the four children have run, one after the other, each under a time limit of its own; at the first that ends with a fatal
    status no further child is started"""
    tmp = tmp_path_factory.mktemp("device_io_paths")
    arrays, indexes, calls = child_manifest(cut_worlds)
    inp = str(tmp / "input.npz")
    np.savez(inp, manifest=np.array(json.dumps(dict(indexes=indexes, calls=calls))), **arrays)
    out = {"calls": calls}
    for name, knobs in CHILDREN.items():
        env = dict(os.environ)
        for key in ("AUNCEL_AMD_FIXED_ROUNDS", "AUNCEL_AMD_SELECT", "AUNCEL_AMD_TIE_FIX", "AUNCEL_AMD_EXACT_SEED"):
            env.pop(key, None)
        env.update(knobs)
        outdir = str(tmp / name)
        t0 = time.time()
        try:
            # (a child takes a few seconds, most of them the start of the interpreter, torch and the HIP runtime; a machine that other
            # work shares starts processes slowly, so the limit is generous)
            p = subprocess.run([sys.executable, CHILD, inp, outdir], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            rc, log = p.returncode, p.stdout
        except subprocess.TimeoutExpired as e:
            rc, log = "timeout", (e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else e.stdout or "")
        print(f"child {name}: exit {rc}, {time.time() - t0:.1f} s\n{log[-2000:]}")
        if rc == "timeout" or rc in FATAL:
            pytest.fail(f"child {name} ended with {rc}; no further child is started\n{log[-3000:]}")
        assert rc == 0, (name, rc, log[-3000:])
        out[name] = dict(np.load(os.path.join(outdir, "out.npz")))
    return out


def child_sides_equal(got, call):
    for f in ("I", "D", "state"):
        a, b = got[f"{call}/host_{f}"], got[f"{call}/dev_{f}"]
        if f == "D":
            a, b = bits(a), bits(b)
        assert np.array_equal(a, b), (call, f)


@gpu
@pytest.mark.parametrize("child", ["baseline", "budget", "pairs"])
def test_budget_cut_deferred_queries_get_their_rows(children, child):
    """under the planner's knobs the deferred queries get their rows in a later pass, stored into the caller's device rows like the
    first pass's.  Witness, as test_gpu_budget_cut.py holds it: the `_dev` call took more planning passes than the same call of the
    child without a knob.  Every result is also the no-knob child's"""
    got, base = children[child], children["baseline"]
    for c in children["calls"]:
        call = c["name"]
        if c["op"] == "exact":
            continue
        child_sides_equal(got, call)
        io = got[call + "/dev_io"]
        assert io[0] == 0 and io[1] == 0 and io[3] == 1, (call, io)
        assert np.array_equal(got[call + "/dev_I"], base[call + "/dev_I"]) and np.array_equal(bits(got[call + "/dev_D"]), bits(base[call + "/dev_D"])), call
        rounds, rounds0 = int(got[call + "/dev_state"][ST_ROUNDS]), int(base[call + "/dev_state"][ST_ROUNDS])
        print(call, child, "planning passes", rounds, "without a knob", rounds0)
        if child == "baseline":
            assert rounds >= 1, call
        else:
            assert rounds > rounds0, (call, child, "no query was deferred", rounds, rounds0)


@gpu
@pytest.mark.parametrize("mname", ["l2", "ip"])
def test_exact_candidate_overflow_in_a_child(children, mname):
    """AUNCEL_AMD_EXACT_CAP=16 with k = 10 and a seed of four lists: queries whose candidates pass their 16 slots are searched the
    general way -- some, not all -- and the result is the default capacity's"""
    call = f"X_{mname}_exact"
    got, base = children["exact_cap"], children["baseline"]
    child_sides_equal(got, call)
    n = got[call + "/dev_I"].shape[0]
    last, io = got[call + "/dev_state"][ST_EXACT], got[call + "/dev_io"]
    print(call, "last_exact", last, "without the knob", base[call + "/dev_state"][ST_EXACT], "dev_io", io)
    assert last[2] > 0 and 0 < last[1] + last[2] < n and int(last[:3].sum()) == n, last
    assert io[0] == 0 and io[1] == 0 and io[3] == 2, io
    assert last[1] + last[2] > base[call + "/dev_state"][ST_EXACT][1:3].sum()
    # more than one run of flagged queries: the rows the two capacities' passes disagree on cannot be told apart (the results are
    # equal by design), so the count is the witness
    child_sides_equal(base, call)
    assert np.array_equal(got[call + "/dev_I"], base[call + "/dev_I"]) and np.array_equal(bits(got[call + "/dev_D"]), bits(base[call + "/dev_D"]))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. handles that are not a plain owner
# ------------------------------------------------------------------------------------------------------------------------------
def handle_pairs(torch, h, xq, tag, resident_dev=None):
    """search_dev, search_exact_dev and set_queries_dev + search_resident_dev equal the handle's own host calls"""
    n = len(xq)
    x = to_gpu(torch, xq)
    for k in (1, 10):
        for entry in ("search", "resident"):
            fixed_pair(torch, h, entry, xq, x, k, 4, None, tag + (entry, k))
        exact_pair(torch, h, xq, k, tag + ("exact", k))
    return x


@gpu
@pytest.mark.parametrize("kind", ["float", "bytes"])
@pytest.mark.parametrize("metric", [L2, IP])
def test_subset_and_joined_handles(capi, torch, metric, kind):
    """a subset by id range, a join of two halves with id offsets, and a clone of each"""
    w = world(30, metric, kind)
    h = new_handle(capi, w)
    nb, nlist = len(w["xb"]), w["nlist"]
    xq = w["xq"]
    sub = h.subset(capi.SUBSET_ID_RANGE, 500, 1500)
    looked, kept, h2d, d2h = sub.last_subset()
    assert (looked, kept) == (nb, 1000) and h2d <= 16 * (nlist + 1) + 65536 and d2h <= 16 * (nlist + 1) + 65536, sub.last_subset()
    a, b = h.subset(capi.SUBSET_ID_RANGE, 0, nb // 2), h.subset(capi.SUBSET_ID_RANGE, nb // 2, nb)
    joined = capi.Handle.concat([(a, None, None, 0), (b, None, None, 100000)])
    taken, nparts, h2d, d2h = joined.last_concat()
    assert (taken, nparts) == (nb, 2) and h2d <= (2 * 2 + 2) * 8 * (nlist + 1) + 65536 and d2h <= 65536, joined.last_concat()
    for name, g in (("subset", sub), ("joined", joined)):
        handle_pairs(torch, g, xq, (metric, kind, name))
        cl = g.clone()
        handle_pairs(torch, cl, xq, (metric, kind, name, "clone"))
        same(cl.search_dev(to_gpu(torch, xq), 10, 4), g.search(xq, 10, 4), (name, "clone against its index"))
        cl.close()
    I = sub.search_dev(to_gpu(torch, xq), 10, 16)[1].cpu().numpy()
    assert ((I >= 500) & (I < 1500)).all()
    I = joined.search_dev(to_gpu(torch, xq), 10, 16)[1].cpu().numpy()
    assert ((I >= 0) & (I < nb // 2) | (I >= 100000 + nb // 2) & (I < 100000 + nb)).all() and (I >= 100000).any()
    for g in (joined, a, b, sub, h):
        g.close()


@gpu
@pytest.mark.parametrize("kind", ["float", "bytes"])
def test_handle_after_add_and_remove(capi, torch, kind):
    """add of 100 rows, then remove_ids of 50: the `_dev` call right after each change finds the journal pending and sees the new
    lists; the resident set put there by set_queries_dev before the change is still served; a clone follows"""
    w = world(30, L2, kind)
    h = new_handle(capi, w)
    xq = w["xq"]
    n = len(xq)
    x = to_gpu(torch, xq)
    h.search(xq[:1], 1, 1)  # (the lists are on the device: what follows is a change in place)
    h.set_queries_dev(x)
    rs = np.random.RandomState(30)
    new = w["xb"][rs.choice(len(w["xb"]), 100, replace=False)].copy()
    new[:, 1:] = np.minimum(new[:, 1:] + 1.0, 255.0) if kind == "bytes" else new[:, 1:] + 0.25
    new[:, 0] = np.arange(100) % 7 + (300.0 if kind == "float" else 0.0)  # (no row of the world looks like these)
    new_ids = np.arange(5000, 5100, dtype=np.int64)
    h.add(new, new_ids)
    # the journal is pending: this call applies it, and every new row is found by its own vector
    D, I = h.search_dev(to_gpu(torch, new), 1, w["nlist"])
    assert h.last_update()[0] == 1, h.last_update()
    assert np.array_equal(I.cpu().numpy()[:, 0], new_ids)
    same((D, I), h.search(new, 1, w["nlist"]), (kind, "add"))
    # the resident set of before the change, over the new lists
    want = h.search(xq, 10, 4)
    same(h.search_resident_dev(0, n, 10, 4), want, (kind, "resident across add"))
    assert h.last_dev_io()[2] == 0
    handle_pairs(torch, h, xq, (kind, "after add"))
    # remove 50 ids that the queries find
    found = h.search(xq, 1, w["nlist"])[1][:, 0]
    gone = np.unique(found)[:50]
    assert len(gone) == 50
    h.set_queries_dev(x)
    assert h.remove_ids(gone) == 50
    D, I = h.search_dev(x, 10, w["nlist"])
    assert h.last_update()[0] == 1, h.last_update()
    assert not np.isin(I.cpu().numpy(), gone).any()
    same((D, I), h.search(xq, 10, w["nlist"]), (kind, "remove"))
    got = h.search_resident_dev(0, n, 10, w["nlist"])
    same(got, h.search(xq, 10, w["nlist"]), (kind, "resident across remove"))
    assert not np.isin(h.search_exact_dev(x, 10)[1].cpu().numpy(), gone).any()
    handle_pairs(torch, h, xq, (kind, "after remove"))
    cl = h.clone()
    handle_pairs(torch, cl, xq, (kind, "clone after the changes"))
    I = cl.search_dev(x, 10, w["nlist"])[1].cpu().numpy()
    assert not np.isin(I, gone).any()
    assert np.array_equal(cl.search_dev(to_gpu(torch, new), 1, w["nlist"])[1].cpu().numpy()[:, 0], new_ids)
    cl.close()
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the class mirror
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from auncel_amd import build
    build.build_host()
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))))
    exe = str(tmp_path_factory.mktemp("drv") / "device_io_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), DRIVER_SRC, "-o", exe,
                    "-L" + build.LIBDIR, "-lfaiss_amd", "-launcel_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                    "-Wl,-rpath," + build.LIBDIR, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-pthread"], check=True)
    return exe


@gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_the_class_mirror_search_dev(driver, tmp_path, metric):
    """IndexIVFFlat::search_dev and IndexIVFFlatSubset::search_dev return search()'s bytes into rows of a larger device buffer"""
    from oracle import tbundle
    rs = np.random.RandomState(16)
    nlist, d, nb, nq, k = 16, 30, 2500, 65, 10
    cen = rs.randn(nlist, d).astype(np.float32)
    xb = (cen[rs.randint(0, nlist, size=nb)] + 0.3 * rs.randn(nb, d)).astype(np.float32)
    xq = (cen[rs.randint(0, nlist, size=nq)] + 0.3 * rs.randn(nq, d)).astype(np.float32)
    t = {"d": d, "nlist": nlist, "nprobe": 6, "k": k, "metric": metric, "centroids": cen, "xb": xb, "xq": xq,
         "range_lo": np.int64(nb // 3), "range_hi": np.int64(2 * nb // 3)}
    fin, fout = str(tmp_path / "in.tb"), str(tmp_path / "out.tb")
    tbundle.save(fin, t)
    r = subprocess.run([driver, fin, fout], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    out = tbundle.load(fout)
    for p in ("flat_", "subset_"):
        assert np.array_equal(out[p + "dev_I"], out[p + "host_I"]), p
        assert np.array_equal(bits(out[p + "dev_D"]), bits(out[p + "host_D"])), p
        assert int(out[p + "guards_ok"][0]) == 1, p
        io = [int(v) for v in out[p + "dev_io"]]
        assert io[0] == 0 and io[1] == 0 and io[2] == 2 and io[3] == 1, (p, io)
        assert (out[p + "host_I"] >= 0).all()
    assert int(out["subset_ntotal"][0]) == 2 * nb // 3 - nb // 3
    sI = out["subset_dev_I"]
    assert ((sI >= nb // 3) & (sI < 2 * nb // 3)).all() and not np.array_equal(sI, out["flat_dev_I"])
