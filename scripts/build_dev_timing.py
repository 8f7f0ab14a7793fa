"""Cost of building an index from rows that are in GPU memory: the 10M-row SIFT-like (d = 128, L2, byte-valued) and
DEEP-like (d = 96, inner product) sets of auncel_amd/synth.py, IVF4096, as a torch tensor on the device.  (1) amd_ivf_build_dev plus the
first search; (2) the route without it: the tensor to the host, amd_ivf_add into an empty owner, the first search (which uploads the
lists).  1000 queries at nprobe 32; the second of two repetitions is reported.  Prints one JSON line per case, with amd_ivf_last_build's
counters and whether both routes return the same bits.
usage: python3 scripts/build_dev_timing.py [--nb N] [--case sift|deep] [--device-only]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auncel_amd import capi, synth  # noqa: E402

args = sys.argv[1:]
NB = int(args[args.index("--nb") + 1]) if "--nb" in args else 10_000_000
ONLY = args[args.index("--case") + 1] if "--case" in args else None
DEVICE_ONLY = "--device-only" in args
NQ, NLIST = 1000, 4096
CASES = [("sift", synth.sift_like, 128, capi.METRIC_L2), ("deep", synth.deep_like, 96, capi.METRIC_IP)]

for name, make, d, metric in CASES:
    if ONLY and name != ONLY:
        continue
    xb, xq = make(NB, NQ, d=d)
    q = capi.Handle(d, NLIST, metric, 0)
    q.set_centroids(synth.sample_centroids(xb, NLIST))
    x = torch.from_numpy(xb).cuda()
    del xb
    row = {"case": name, "nb": NB, "d": d}
    for rep in range(2):  # (the second build: allocations of the first are back in the runtime's pool)
        torch.cuda.synchronize()
        t0 = time.time()
        b = q.build_dev(x)
        t1 = time.time()
        D0, I0 = b.search(xq, 10, 32)
        t2 = time.time()
        row.update({"build_dev_ms": round((t1 - t0) * 1e3, 2), "first_search_ms": round((t2 - t1) * 1e3, 2),
                    "device_total_ms": round((t2 - t0) * 1e3, 2), "last_build": b.last_build(), "scan_arith": b.scan_arith()})
        b.close()
    if not DEVICE_ONLY:
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.time()
            host = x.cpu().numpy()
            t1 = time.time()
            g = capi.Handle(d, NLIST, metric, 0)
            g.set_centroids(synth.sample_centroids(host, NLIST))
            t2 = time.time()
            g.add(host)
            t3 = time.time()
            D1, I1 = g.search(xq, 10, 32)
            t4 = time.time()
            g.close()
            del host
        row.update({"host_copy_down_ms": round((t1 - t0) * 1e3, 2), "host_add_ms": round((t3 - t2) * 1e3, 2),
                    "host_first_search_ms": round((t4 - t3) * 1e3, 2), "host_total_ms": round((t1 - t0 + t4 - t2) * 1e3, 2),
                    "same_results": bool(np.array_equal(I0, I1) and np.array_equal(D0.view(np.uint32), D1.view(np.uint32)))})
    print(json.dumps(row), flush=True)
    q.close()
    del x
