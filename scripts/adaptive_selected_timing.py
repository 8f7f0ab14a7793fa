"""Cost of the adaptive search under an id selector against the subset index and against the parent's unselected adaptive search
("The adaptive rule under a selector"): on the 10M x 128 byte-valued index of auncel_amd/synth.py, IVF4096, 5000
resident queries at the bench's error bound (0.95, query_topk 10), under id % 100 == 7 (1 %), id % 10 == 3 (10 %) and id % 2 == 1
(50 %).  The traces are trained once, on the parent, from TRAIN further queries and the exact ground truth
(amd_ivf_search_exact_resident), multipler 1 and std_m 1 -- one set of traces for every row, as the contract has it: the subset
copies them, the selected call reads them from the handle.  Per selector: amd_ivf_search_adaptive_selected with the planner's skip on
and off, the subset's amd_ivf_search_adaptive, and once the parent's unselected amd_ivf_search_adaptive; medians of --reps
synchronising calls after two warm-up calls (wall time and the engine's HIP-event time), the mean my_nprobe, and the call's scan bytes
(amd_ivf_last_timing, a count).  One JSON line per row; ONE run, short windows: differences of a tenth of a millisecond are inside
what a second run may move.  --out FILE also writes the lines there (profiles/adaptive_selected_timing.txt is where a run belongs).
usage: python3 scripts/adaptive_selected_timing.py [--nb N] [--reps R] [--out FILE]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from auncel_amd import capi, synth  # noqa: E402

args = sys.argv[1:]
NB = int(args[args.index("--nb") + 1]) if "--nb" in args else 10_000_000
REPS = int(args[args.index("--reps") + 1]) if "--reps" in args else 10
OUT = args[args.index("--out") + 1] if "--out" in args else None
NQ, TRAIN, NLIST, D, K, TOPK, BOUND, MULT, STD_M = 5000, 2000, 4096, 128, 100, 10, 0.95, 1.0, 1.0
lines = []


def say(row):
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)


xb, xq = synth.sift_like(NB, NQ + TRAIN, d=D)
cen = synth.sample_centroids(xb, NLIST)
h = capi.Handle(D, NLIST, capi.METRIC_L2, 0)
h.set_centroids(cen)
t0 = time.time()
h.add(xb)
del xb
h.set_interdis(None)
h.set_queries(xq)
h.set_option("coarse_ties", 2)  # (the bench's regime)
ntr = 0
while (1 << ntr) <= NLIST // 8:
    ntr += 1
gtD, _ = h.search_exact_resident(NQ, TRAIN, K)
gt_all = np.zeros((NQ + TRAIN, K), np.float32)
gt_all[NQ:] = gtD
raw = [np.full(((NQ + TRAIN) * (K // 4), 2), -1, dtype=np.float32) for _ in range(ntr)]
h.train_samples(NQ, TRAIN, K, gt_all, NQ + TRAIN, raw)
traces = [capi.trace_sb(r[NQ * (K // 4):]) for r in raw]
h.set_tuner(K, traces, capi.arcos_table())
say({"nb": NB, "build_and_training_s": round(time.time() - t0, 1), "reps": REPS, "bound": BOUND, "bins_per_trace": [len(t[0]) for t in traces]})
req = np.full(NQ + TRAIN, BOUND, np.float32)


def steady(handle, f):
    """f(my_nprobe, t_recalls) is one synchronising call: -> median wall ms, median HIP-event ms, mean my_nprobe, scan bytes"""
    wall, dev = [], []
    for i in range(REPS + 2):
        my_np = np.zeros(NQ + TRAIN, np.uint64)
        t_rec = np.zeros(NQ + TRAIN, np.float32)
        t = time.time()
        f(my_np, t_rec)
        if i >= 2:
            wall.append((time.time() - t) * 1e3)
            dev.append(handle.last_timing()["total_ms"])
    return {"wall_ms": round(float(np.median(wall)), 3), "event_ms": round(float(np.median(dev)), 3),
            "mean_my_nprobe": round(float(my_np[:NQ].mean()), 2), "scan_bytes": handle.last_timing()["scan_bytes"]}


say({"call": "parent, unselected", **steady(h, lambda p, t: h.search_adaptive(0, NQ, TOPK, MULT, STD_M, req, p, t))})
for name, m, r in (("1 %", 100, 7), ("10 %", 10, 3), ("50 %", 2, 1)):
    with h.selector(capi.SUBSET_ID_MOD, m, r) as s:
        for skip in (1, 0):
            h.set_option("selected_skip_empty", skip)
            say({"call": "search_adaptive_selected", "selector": name, "skip_empty": skip,
                 **steady(h, lambda p, t: h.search_adaptive_selected(s, 0, NQ, TOPK, MULT, STD_M, req, p, t))})
        h.set_option("selected_skip_empty", None)
    sub = h.subset(capi.SUBSET_ID_MOD, m, r)
    sub.set_queries(xq)
    sub.set_option("coarse_ties", 2)
    say({"call": "subset's search_adaptive", "selector": name, **steady(sub, lambda p, t: sub.search_adaptive(0, NQ, TOPK, MULT, STD_M, req, p, t))})
    sub.close()
if OUT:
    with open(OUT, "w") as f:
        f.write("# adaptive_selected_timing: nb %d, nlist %d, d %d, %d queries, medians of %d synchronising calls, ONE run on one MI355X\n" % (NB, NLIST, D, NQ, REPS))
        f.write("\n".join(lines) + "\n")
h.close()
