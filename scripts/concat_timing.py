"""Cost of joining resident indexes: on the 10M x 128 byte-valued index of auncel_amd/synth.py, IVF4096, (1) a merge
of two halves and (2) a window of four slices that steps -- drops a quarter of every list's front, takes a quarter -- each through
amd_ivf_concat and through the route without it: amd_ivf_get_list of every list, a numpy concatenation, amd_ivf_set_lists into a fresh
handle.  Every time includes the first search of 1000 queries at nprobe 32.  Prints one JSON line per case, with amd_ivf_last_concat's
counters.  The parts are amd_ivf_subset cuts of one index by id (a quarter each: id % 4).
usage: python3 scripts/concat_timing.py [--nb N] [--device-only]"""
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
quarters = [h.subset(capi.SUBSET_ID_MOD, 4, r) for r in range(4)]
halves = [h.subset(capi.SUBSET_ID_MOD, 2, r) for r in range(2)]
h.close()
window = capi.Handle.concat(quarters)  # the window before the step: four slices
oldest = np.array([quarters[0].list_size(l) for l in range(NLIST)], np.uint64)  # what the oldest slice gave every list
CASES = [("merge of two halves", lambda: [halves[0], halves[1]]),
         ("window step: drop a quarter, take a quarter", lambda: [(window, oldest, None, 0), (quarters[0], None, None, NB)])]


def host_route(parts):
    """the parent commit's only route: every list back over PCIe, joined on the host, sent again"""
    t0 = time.time()
    codes, ids = [], []
    for l in range(NLIST):
        cs, js = [], []
        for p in parts:
            hp, b, e, add = (tuple(p) + (None, None, 0))[:4] if isinstance(p, tuple) else (p, None, None, 0)
            c, i = hp.get_list(l)
            lo, hi = (0 if b is None else int(b[l])), (len(i) if e is None else int(e[l]))
            cs.append(c[lo:hi])
            js.append(i[lo:hi] + add)
        codes.append(np.concatenate(cs))
        ids.append(np.concatenate(js))
    t1 = time.time()
    g = capi.Handle(D, NLIST, capi.METRIC_L2, 0)
    g.set_centroids(cen)
    g.set_lists([len(i) for i in ids], codes, ids)
    t2 = time.time()
    D1, I1 = g.search(xq, 10, 32)
    t3 = time.time()
    g.close()
    return {"host_get_and_join_ms": round((t1 - t0) * 1e3, 2), "host_set_lists_ms": round((t2 - t1) * 1e3, 2),
            "host_first_search_ms": round((t3 - t2) * 1e3, 2), "host_total_ms": round((t3 - t0) * 1e3, 2)}, D1, I1


for name, make in CASES:
    row = {"case": name}
    for rep in range(2):  # (the second join: allocations of the first are back in the runtime's pool)
        t0 = time.time()
        j = capi.Handle.concat(make())
        t1 = time.time()
        D0, I0 = j.search(xq, 10, 32)
        t2 = time.time()
        row.update({"concat_ms": round((t1 - t0) * 1e3, 2), "first_search_ms": round((t2 - t1) * 1e3, 2),
                    "device_total_ms": round((t2 - t0) * 1e3, 2), "last_concat": j.last_concat(), "scan_arith": j.scan_arith()})
        j.close()
    if not DEVICE_ONLY:
        host, D1, I1 = host_route(make())
        row.update(host)
        row["same_results"] = bool(np.array_equal(I0, I1) and np.array_equal(D0.view(np.uint32), D1.view(np.uint32)))
    print(json.dumps(row), flush=True)
for x in quarters + halves + [window]:
    x.close()
