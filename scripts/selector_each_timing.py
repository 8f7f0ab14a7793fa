"""One batch under a selector per query against the same queries issued as one call per selector: on the 10M x 128
byte-valued index of scripts/selector_timing.py (auncel_amd/synth.py, IVF4096, nprobe 32), 5000 queries spread evenly over 1, 8 and
64 selectors (id % nsel == j: each keeps 1 / nsel of the entries), with byte codes and on the fp32 path.  Medians of --reps
synchronising calls after two warm-up calls, wall time, of
  (a) the one amd_ivf_search_selected_each call;
  (b) the same queries grouped by selector and issued as nsel amd_ivf_search_selected calls (the yardstick: code that the per-query
      form does not touch);
  (c) the unfiltered search of the 5000 queries.
One JSON line per row; same_results says whether (a) and (b) returned the same bits.  --trace: nothing is timed; four calls each of
amd_ivf_search_selected and of the _each form at nsel 1 on either path, for a kernel trace to compare keep_rows_kernel with
keep_rows_each_kernel (rocprofv3 --kernel-trace --stats -- python3 scripts/selector_each_timing.py --trace).
usage: python3 scripts/selector_each_timing.py [--nb N] [--reps R] [--trace]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auncel_amd import capi, synth  # noqa: E402

args = sys.argv[1:]
NB = int(args[args.index("--nb") + 1]) if "--nb" in args else 10_000_000
REPS = int(args[args.index("--reps") + 1]) if "--reps" in args else 10
TRACE = "--trace" in args
NQ, NLIST, D, K, NPROBE = 5000, 4096, 128, 10, 32
xb, xq = synth.sift_like(NB, NQ, d=D)
cen = synth.sample_centroids(xb, NLIST)
h = capi.Handle(D, NLIST, capi.METRIC_L2, 0)
h.set_centroids(cen)
t0 = time.time()
h.add(xb)
h.search(xq, K, NPROBE)
print(json.dumps({"nb": NB, "nq": NQ, "build_s": round(time.time() - t0, 1)}), flush=True)
del xb


def steady(call):
    """median wall ms of REPS calls after two warm-up calls"""
    call()
    call()
    wall = []
    for _ in range(REPS):
        t = time.time()
        call()
        wall.append((time.time() - t) * 1e3)
    return round(float(np.median(wall)), 3)


if TRACE:
    s = h.selector(capi.SUBSET_ID_MOD, 2, 1)
    zeros = np.zeros(NQ, np.uint32)
    for byte in (1, 0):
        h.set_byte_codes(byte)
        for _ in range(4):
            h.search_selected_each([s], zeros, xq, K, NPROBE)
            h.search_selected(s, xq, K, NPROBE)
    s.close()
    h.close()
    sys.exit(0)

for byte in (1, 0):
    h.set_byte_codes(byte)
    path = "bytes" if byte else "fp32"
    print(json.dumps({"path": path, "row": "unfiltered", "c_ms": steady(lambda: h.search(xq, K, NPROBE)), "scan_arith": h.scan_arith()}), flush=True)
    for nsel in (1, 8, 64):
        sels = [h.selector(capi.SUBSET_ID_MOD, nsel, j) for j in range(nsel)]
        sel_of = (np.arange(NQ) % nsel).astype(np.uint32)  # (neighbouring queries under different selectors)
        groups = [np.nonzero(sel_of == j)[0] for j in range(nsel)]
        xg = [np.ascontiguousarray(xq[g]) for g in groups]

        def grouped():
            return [h.search_selected(sels[j], xg[j], K, NPROBE) for j in range(nsel)]

        Da, Ia = h.search_selected_each(sels, sel_of, xq, K, NPROBE)
        same = all(np.array_equal(Ia[g], I) and np.array_equal(Da[g].view(np.uint32), D_.view(np.uint32)) for g, (D_, I) in zip(groups, grouped()))
        row = {"path": path, "nsel": nsel, "queries_per_selector": NQ // nsel}
        row["a_each_ms"] = steady(lambda: h.search_selected_each(sels, sel_of, xq, K, NPROBE))
        row["b_grouped_ms"] = steady(grouped)
        row["b_over_a"] = round(row["b_grouped_ms"] / row["a_each_ms"], 2)
        row["same_results"] = bool(same)
        print(json.dumps(row), flush=True)
        for s in sels:
            s.close()
h.close()
