"""Cost of cutting a subset of the headline index: on the 10M x 128 byte-valued index of auncel_amd/synth.py,
IVF4096, for ID_MOD with 1 / 10 / 50 % kept and ID_RANGE with 10 % kept, time (a) amd_ivf_subset + the first search of 1000 queries at
nprobe 32 and (b) the route without it: the same rows filtered on the host, sent with amd_ivf_set_lists into a fresh handle, + its
first search.  Prints one JSON line per selector, with amd_ivf_last_subset's counters.
usage: python3 scripts/subset_timing.py [--nb N] [--device-only]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auncel_amd import capi, synth  # noqa: E402

args = sys.argv[1:]
NB = int(args[args.index("--nb") + 1]) if "--nb" in args else 10_000_000
DEVICE_ONLY = "--device-only" in args
NQ, NLIST, D = 1000, 4096, 128
xb, xq = synth.sift_like(NB, NQ, d=D)
cen = synth.sample_centroids(xb, NLIST)
h = capi.Handle(D, NLIST, capi.METRIC_L2, 0)
h.set_centroids(cen)
t0 = time.time()
h.add(xb)
h.search(xq, 10, 32)
print(json.dumps({"nb": NB, "build_s": round(time.time() - t0, 1)}), flush=True)
del xb
codes, ids = [], []
if not DEVICE_ONLY:  # the host's copy of the lists, which the route without amd_ivf_subset filters
    for l in range(NLIST):
        c, i = h.get_list(l)
        codes.append(c)
        ids.append(i)

SELECTORS = [("mod_100 (1 %)", capi.SUBSET_ID_MOD, 100, 7, lambda i: i % 100 == 7), ("mod_10 (10 %)", capi.SUBSET_ID_MOD, 10, 3, lambda i: i % 10 == 3),
             ("mod_2 (50 %)", capi.SUBSET_ID_MOD, 2, 1, lambda i: i % 2 == 1),
             ("range (10 %)", capi.SUBSET_ID_RANGE, NB // 2, NB // 2 + NB // 10, lambda i: (i >= NB // 2) & (i < NB // 2 + NB // 10))]
for name, kind, a1, a2, rule in SELECTORS:
    row = {"selector": name}
    for rep in range(2):  # (the second cut: allocations of the first are back in the runtime's pool)
        t0 = time.time()
        sub = h.subset(kind, a1, a2)
        t1 = time.time()
        D0, I0 = sub.search(xq, 10, 32)
        t2 = time.time()
        row.update({"subset_ms": round((t1 - t0) * 1e3, 2), "first_search_ms": round((t2 - t1) * 1e3, 2), "last_subset": sub.last_subset(),
                    "scan_arith": sub.scan_arith()})
        sub.close()
    if not DEVICE_ONLY:
        t0 = time.time()
        keep = [rule(i) for i in ids]
        fc, fi = [c[k] for c, k in zip(codes, keep)], [i[k] for i, k in zip(ids, keep)]
        t1 = time.time()
        g = capi.Handle(D, NLIST, capi.METRIC_L2, 0)
        g.set_centroids(cen)
        t2 = time.time()
        g.set_lists([len(i) for i in fi], fc, fi)
        t3 = time.time()
        D1, I1 = g.search(xq, 10, 32)
        t4 = time.time()
        row.update({"host_filter_ms": round((t1 - t0) * 1e3, 2), "host_set_lists_ms": round((t3 - t2) * 1e3, 2),
                    "host_first_search_ms": round((t4 - t3) * 1e3, 2), "host_last_update": g.last_update(),
                    "same_results": bool(np.array_equal(I0, I1) and np.array_equal(D0.view(np.uint32), D1.view(np.uint32)))})
        g.close()
        del fc, fi, keep
    print(json.dumps(row), flush=True)
h.close()
