"""amd_ivf_kmeans_dev against amd_ivf_kmeans on the same rows: 1M x 128 (SIFT-like) and 1M x 960 (GIST-like) of
auncel_amd/synth.py, k = 4096, 5 iterations, max_points_per_centroid = 256, AUNCEL_AMD_ASSIGN_FUSED = AUNCEL_AMD_ASSIGN_WIDE = 1 for
both.  In one process the two calls alternate; medians and ranges of REPS calls after one warm-up call each, host clocks around
calls that return after the engine's stream has finished, set-up included (the host call: its finite check, sub-sampling and
upload from numpy; the device call: its finite check and sampling kernels from a tensor that is on the device already).  The
centroids and objectives of the two must be equal by bits.  One JSON line per case.  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats` with --reps 1: the figures of interest are update_kernel + order_kernel + place_kernel + the
build_* kernels against kmeans_sums_kernel + the DeviceRadixSort kernels, and objective_kernel.
usage: python3 scripts/kmeans_dev_timing.py [--case sift|gist] [--reps R] [--n N]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

os.environ["AUNCEL_AMD_ASSIGN_FUSED"] = "1"
os.environ["AUNCEL_AMD_ASSIGN_WIDE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auncel_amd import capi, synth  # noqa: E402

args = sys.argv[1:]
N = int(args[args.index("--n") + 1]) if "--n" in args else 1_000_000
REPS = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
ONLY = args[args.index("--case") + 1] if "--case" in args else None
K, NITER, MAX_PTS = 4096, 5, 256


def timed(f):
    torch.cuda.synchronize()
    t0 = time.time()
    r = f()
    torch.cuda.synchronize()
    return (time.time() - t0) * 1e3, r


for name, make, d in (("sift", synth.sift_like, 128), ("gist", synth.gist_like, 960)):
    if ONLY and name != ONLY:
        continue
    xb, _ = make(N, 1, d=d)
    x = torch.from_numpy(xb).cuda()
    ms, out, last = {"host": [], "dev": []}, {}, {}
    for rep in range(REPS + 1):  # (the first round warms both up and is dropped)
        t, out["host"] = timed(lambda: capi.kmeans(capi.METRIC_L2, xb, K, NITER, 1234, MAX_PTS))
        last["host"] = capi.kmeans_last_assign()
        if rep:
            ms["host"].append(t)
        t, out["dev"] = timed(lambda: capi.kmeans_dev(capi.METRIC_L2, x, K, NITER, 1234, MAX_PTS))
        last["dev"] = capi.kmeans_last_assign()
        if rep:
            ms["dev"].append(t)
    nx = min(N, K * MAX_PTS)
    same = bool(np.array_equal(out["host"][0].view(np.uint32), out["dev"][0].cpu().numpy().view(np.uint32))
                and np.array_equal(out["host"][1].view(np.uint32), out["dev"][1].view(np.uint32)))
    print(json.dumps({"case": name, "n": N, "nx": nx, "d": d, "k": K, "niter": NITER, "reps": REPS,
                      "kmeans_ms": round(statistics.median(ms["host"]), 1), "kmeans_dev_ms": round(statistics.median(ms["dev"]), 1),
                      "kmeans_ms_range": [round(min(ms["host"]), 1), round(max(ms["host"]), 1)],
                      "kmeans_dev_ms_range": [round(min(ms["dev"]), 1), round(max(ms["dev"]), 1)],
                      "same_bits": same, "last_assign": last,
                      # what the loops themselves move across the bus an iteration (the assignment pass's own 16-byte read-backs and
                      # the rows it sends the general way come on top, the same in both)
                      "loop_bus_bytes_per_iteration_host": nx * 4 + 2 * (K + 1) * 4 + 2 * K * d * 4,
                      "loop_bus_bytes_per_iteration_dev": 24}), flush=True)
    del x, xb
