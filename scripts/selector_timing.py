"""Cost of a search under an id selector against a subset index: on the 10M x 128 byte-valued index of
auncel_amd/synth.py, IVF4096, 1000 queries at nprobe 32, for id % 100 == 7, id % 10 == 3, id % 2 == 1 and a tenth of the id range,
with byte codes and on the fp32 path: amd_ivf_selector_create and the first and the steady amd_ivf_search_selected; amd_ivf_subset
and its first and steady search; the unfiltered search of the parent; the device bytes either route holds.  Then three rows per
selector: amd_ivf_selector_combine of it with id % 2 == 0 (AND) and of it alone (NOT); amd_ivf_range_search_selected beside the
subset's amd_ivf_range_search at the median 10th-neighbour distance of the selected search; and amd_ivf_search_resident_selected as
tickets at asynchronous depths 1 / 2 / 4 beside the synchronous call (queries per second over --reps batches).  Steady: the median of
--reps calls after a warm-up, as wall time and as the engine's own HIP-event time (amd_ivf_last_timing).  One JSON line per row.
usage: python3 scripts/selector_timing.py [--nb N] [--reps R] [--unfiltered-only]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auncel_amd import capi, synth  # noqa: E402

args = sys.argv[1:]
NB = int(args[args.index("--nb") + 1]) if "--nb" in args else 10_000_000
REPS = int(args[args.index("--reps") + 1]) if "--reps" in args else 20
UNFILTERED_ONLY = "--unfiltered-only" in args  # (what also runs on a commit without the selector entry points)
NQ, NLIST, D, K, NPROBE = 1000, 4096, 128, 10, 32
xb, xq = synth.sift_like(NB, NQ, d=D)
cen = synth.sample_centroids(xb, NLIST)
h = capi.Handle(D, NLIST, capi.METRIC_L2, 0)
h.set_centroids(cen)
t0 = time.time()
h.add(xb)
h.search(xq, K, NPROBE)
print(json.dumps({"nb": NB, "build_s": round(time.time() - t0, 1)}), flush=True)
del xb


def steady(handle, call):
    """median wall and HIP-event ms of REPS calls after two warm-up calls"""
    call()
    call()
    wall, dev = [], []
    for _ in range(REPS):
        t = time.time()
        call()
        wall.append((time.time() - t) * 1e3)
        dev.append(handle.last_timing()["total_ms"])
    return round(float(np.median(wall)), 3), round(float(np.median(dev)), 3)


def timed(f):
    t = time.time()
    r = f()
    return r, round((time.time() - t) * 1e3, 3)


def in_flight(handle, s, depth):
    """queries per second of REPS selected batches as tickets, `depth` searches at a time (the depth is fixed by the first submit:
    the pool is given back before and after)"""
    handle.set_async_depth(0)
    handle.set_async_depth(depth)
    for t in [handle.submit_search_resident_selected(s, 0, NQ, K, NPROBE) for _ in range(2 * depth)]:
        handle.wait(t)
    t0 = time.time()
    for t in [handle.submit_search_resident_selected(s, 0, NQ, K, NPROBE) for _ in range(REPS)]:
        handle.wait(t)
    qps = REPS * NQ / (time.time() - t0)
    handle.set_async_depth(0)
    return round(qps)


SELECTORS = [("mod_100 (1 %)", capi.SUBSET_ID_MOD, 100, 7), ("mod_10 (10 %)", capi.SUBSET_ID_MOD, 10, 3), ("mod_2 (50 %)", capi.SUBSET_ID_MOD, 2, 1),
             ("range (10 %)", capi.SUBSET_ID_RANGE, NB // 2, NB // 2 + NB // 10)]
for byte in (1, 0):
    h.set_byte_codes(byte)
    path = "bytes" if byte else "fp32"
    w, d = steady(h, lambda: h.search(xq, K, NPROBE))
    print(json.dumps({"path": path, "selector": "none (parent)", "steady_wall_ms": w, "steady_event_ms": d, "scan_arith": h.scan_arith()}), flush=True)
    if UNFILTERED_ONLY:
        continue
    for name, kind, a1, a2 in SELECTORS:
        row = {"path": path, "selector": name}
        s, row["selector_create_ms"] = timed(lambda: h.selector(kind, a1, a2))
        s.close()
        s, row["selector_create_again_ms"] = timed(lambda: h.selector(kind, a1, a2))  # (allocations of the first are back in the pool)
        (D0, I0), row["selected_first_ms"] = timed(lambda: h.search_selected(s, xq, K, NPROBE))
        row["selected_steady_wall_ms"], row["selected_steady_event_ms"] = steady(h, lambda: h.search_selected(s, xq, K, NPROBE))
        row["selector_info"] = s.info()
        sub, row["subset_ms"] = timed(lambda: h.subset(kind, a1, a2))
        sub.set_byte_codes(byte)
        (D1, I1), row["subset_first_ms"] = timed(lambda: sub.search(xq, K, NPROBE))
        row["subset_steady_wall_ms"], row["subset_steady_event_ms"] = steady(sub, lambda: sub.search(xq, K, NPROBE))
        nt, dpad = sub.ntotal, (D + 3) // 4 * 4
        row["subset_rows_bytes"] = nt * (4 * dpad + 8)  # (rows and ids alone: the derived copies of its searches come on top)
        row["same_results"] = bool(np.array_equal(I0, I1) and np.array_equal(D0.view(np.uint32), D1.view(np.uint32)))
        print(json.dumps(row), flush=True)
        # ---- combine: with a second selector (AND) and alone (NOT); the first call of each pays the allocations
        row = {"path": path, "selector": name, "row": "combine"}
        even = h.selector(capi.SUBSET_ID_MOD, 2, 0)
        for what, f in (("and", lambda: s & even), ("not", lambda: ~s)):
            c, row["combine_%s_first_ms" % what] = timed(f)
            c.close()
            times = []
            for _ in range(REPS):
                c, ms = timed(f)
                times.append(ms)
                row["combine_%s_info" % what] = c.info()
                c.close()
            row["combine_%s_steady_ms" % what] = round(float(np.median(times)), 3)
        even.close()
        print(json.dumps(row), flush=True)
        # ---- range search: under the selector and on the subset, at the median distance of the selected search's 10th neighbour
        row = {"path": path, "selector": name, "row": "range"}
        kth = D0[:, -1][np.isfinite(D0[:, -1]) & (np.abs(D0[:, -1]) < 1e37)]
        radius = float(np.median(kth)) if kth.size else 1.0
        row["radius"] = radius
        r0 = h.range_search_selected(s, xq, radius, NPROBE)
        r1 = sub.range_search(xq, radius, NPROBE)
        row["results"] = int(r0[0][-1])
        row["selected_range_steady_wall_ms"], row["selected_range_steady_event_ms"] = steady(h, lambda: h.range_search_selected(s, xq, radius, NPROBE))
        row["subset_range_steady_wall_ms"], row["subset_range_steady_event_ms"] = steady(sub, lambda: sub.range_search(xq, radius, NPROBE))
        row["same_results"] = bool(np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1]) and np.array_equal(r0[2].view(np.uint32), r1[2].view(np.uint32)))
        sub.close()
        print(json.dumps(row), flush=True)
        # ---- in flight: tickets at depths 1 / 2 / 4 beside the synchronous resident call
        row = {"path": path, "selector": name, "row": "in_flight"}
        h.set_queries(xq)
        w, _ = steady(h, lambda: h.search_resident_selected(s, 0, NQ, K, NPROBE))
        row["synchronous_qps"] = round(NQ / (w * 1e-3))
        for depth in (1, 2, 4):
            row["depth_%d_qps" % depth] = in_flight(h, s, depth)
        s.close()
        print(json.dumps(row), flush=True)
h.close()
