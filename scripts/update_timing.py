"""Cost of changing the headline index in place: on the 10M x 128 byte-valued index of auncel_amd/synth.py, IVF4096,
time an add of 10000 vectors and a removal of 10000 ids, each with the search after it, with option "incremental" 1 and 0.
Prints one JSON line per mode, with amd_ivf_last_update's counters.  usage: python3 scripts/update_timing.py [1|0 ...]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auncel_amd import capi, synth  # noqa: E402

NB, NQ, NLIST, D = 10_000_000, 1000, 4096, 128
xb, xq = synth.sift_like(NB + 10000, NQ, d=D)
extra, xb = xb[NB:], xb[:NB]
cen = synth.sample_centroids(xb, NLIST)
res = {}
for inc in [int(a) for a in sys.argv[1:]] or [1, 0]:
    h = capi.Handle(D, NLIST, capi.METRIC_L2, 0)
    h.set_option("incremental", inc)
    h.set_centroids(cen)
    t0 = time.time()
    h.add(xb)
    h.search(xq, 10, 32)
    build_s = time.time() - t0
    for _ in range(3):
        t0 = time.time()
        h.search(xq, 10, 32)
        steady = time.time() - t0
    t0 = time.time()
    h.add(extra, xids=np.arange(NB, NB + 10000, dtype=np.int64))
    t1 = time.time()
    h.search(xq, 10, 32)
    t2 = time.time()
    add_lu = h.last_update()
    rm = np.random.RandomState(1).choice(NB, 10000, replace=False).astype(np.int64)
    t3 = time.time()
    n = h.remove_ids(rm)
    t4 = time.time()
    h.search(xq, 10, 32)
    t5 = time.time()
    rm_lu = h.last_update()
    res[f"incremental={inc}"] = {"build_s": round(build_s, 1), "steady_search_ms": round(steady * 1e3, 2),
                                 "add_call_ms": round((t1 - t0) * 1e3, 2), "first_search_after_add_ms": round((t2 - t1) * 1e3, 2),
                                 "add_last_update": add_lu, "remove_call_ms": round((t4 - t3) * 1e3, 2), "removed": n,
                                 "search_after_remove_ms": round((t5 - t4) * 1e3, 2), "remove_last_update": rm_lu}
    print(json.dumps({f"incremental={inc}": res[f"incremental={inc}"]}), flush=True)
    h.close()
    del h
