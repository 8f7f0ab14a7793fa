"""Cost of the nearest-centroid assignment with option "assign_fused" 0 (the general path) and 1 (the fused
matrix-core pass of ivf_assign.hip): the 10M-row SIFT-like (d = 128, L2) and DEEP-like (d = 96, inner product) sets of
auncel_amd/synth.py, IVF4096, as a torch tensor on the device.  Per case, in one process, the two forms alternating, medians of
REPS calls after one warm-up call each: amd_ivf_build_dev with the option 0 and 1, and amd_ivf_assign_dev alone (always the fused
pass; its assignment is compared with the option-0 build's list sizes).  Then amd_ivf_kmeans (1M x 128, k = 4096, 5 iterations),
AUNCEL_AMD_ASSIGN_FUSED unset and set, alternating (its handle is its own: the environment is what reaches it).  Host clocks
around calls that return after the engine's stream has finished.  Case "gist": the GIST-like set (1M x 960, L2), "assign_fused" and
"assign_wide" both 0 against both 1 in build_dev, assign_dev and amd_ivf_kmeans (section 18.1).  One JSON line per case.
usage: python3 scripts/assign_timing.py [--nb N] [--case sift|deep|gist|kmeans] [--reps R] [--nk N] [--ng N]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auncel_amd import capi, synth  # noqa: E402

args = sys.argv[1:]
NB = int(args[args.index("--nb") + 1]) if "--nb" in args else 10_000_000
NK = int(args[args.index("--nk") + 1]) if "--nk" in args else 1_000_000
NG = int(args[args.index("--ng") + 1]) if "--ng" in args else 1_000_000
REPS = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
ONLY = args[args.index("--case") + 1] if "--case" in args else None
NLIST = 4096
CASES = [("sift", synth.sift_like, 128, capi.METRIC_L2), ("deep", synth.deep_like, 96, capi.METRIC_IP)]


def timed(f):
    torch.cuda.synchronize()
    t0 = time.time()
    r = f()
    torch.cuda.synchronize()
    return (time.time() - t0) * 1e3, r


def med(v):
    return round(statistics.median(v), 2)


for name, make, d, metric in CASES:
    if ONLY and name != ONLY:
        continue
    xb, _ = make(NB, 1, d=d)
    q = capi.Handle(d, NLIST, metric, 0)
    q.set_centroids(synth.sample_centroids(xb, NLIST))
    x = torch.from_numpy(xb).cuda()
    del xb
    ms = {0: [], 1: [], "assign": []}
    digest, last = {}, {}
    for rep in range(REPS + 1):  # (the first round warms every form up and is dropped)
        for fused in (0, 1):
            q.set_option("assign_fused", fused)
            t, b = timed(lambda: q.build_dev(x))
            digest[fused], last[fused] = b.layout_digest(), q.last_assign()
            b.close()
            if rep:
                ms[fused].append(t)
        t, (a, _) = timed(lambda: q.assign_dev(x))
        last["assign"] = q.last_assign()
        if rep:
            ms["assign"].append(t)
    # what the kernels of the fused pass need at the least: 2 sweeps x 2 n nlist 16 JP flops on the matrix cores, and every
    # workgroup's 2 reads of the table from L2 into LDS
    jp = (((d + 15) // 16) + 1) & ~1
    flops = 2 * 2.0 * NB * NLIST * 16 * jp
    lds_fill = 2.0 * ((NB + 255) // 256) * ((NLIST + 31) // 32) * (jp * 1024 + 128)
    print(json.dumps({"case": name, "nb": NB, "d": d, "nlist": NLIST, "reps": REPS, "build_dev_ms_fused0": med(ms[0]), "build_dev_ms_fused1": med(ms[1]),
                      "assign_dev_ms": med(ms["assign"]), "all_ms": {str(k): [round(t, 1) for t in v] for k, v in ms.items()},
                      "same_layout": digest[0] == digest[1], "last_assign_build_fused1": last[1], "last_assign_assign_dev": last["assign"],
                      "fused_mfma_flops": flops, "fused_table_bytes_into_lds": lds_fill}), flush=True)
    q.close()
    del x, a

if not ONLY or ONLY == "gist":
    # beyond 128 dimensions: "assign_fused" and "assign_wide" both 0 (the general path: what every such call
    # launched before the wide pass existed) against both 1, alternating -- build_dev, assign_dev alone, then amd_ivf_kmeans under the
    # two environment variables
    d = 960
    xb, _ = synth.gist_like(NG, 1, d=d)
    q = capi.Handle(d, NLIST, capi.METRIC_L2, 0)
    q.set_centroids(synth.sample_centroids(xb, NLIST))
    x = torch.from_numpy(xb).cuda()
    ms = {(w, on): [] for w in ("build", "assign", "kmeans") for on in (0, 1)}
    digest, got, last, cen = {}, {}, {}, {}
    for rep in range(REPS + 1):
        for on in (0, 1):
            q.set_option("assign_fused", on)
            q.set_option("assign_wide", on)
            t, b = timed(lambda: q.build_dev(x))
            digest[on], last["build", on] = b.layout_digest(), q.last_assign()
            b.close()
            t2, (got[on], _) = timed(lambda: q.assign_dev(x))
            last["assign", on] = q.last_assign()
            for k in ("AUNCEL_AMD_ASSIGN_FUSED", "AUNCEL_AMD_ASSIGN_WIDE"):
                os.environ.pop(k, None)
                if on:
                    os.environ[k] = "1"
            t3, (cen[on], _) = timed(lambda: capi.kmeans(capi.METRIC_L2, xb, NLIST, niter=5))
            last["kmeans", on] = capi.kmeans_last_assign()
            if rep:
                ms["build", on].append(t), ms["assign", on].append(t2), ms["kmeans", on].append(t3)
    jp = (((d + 15) // 16) + 1) & ~1
    print(json.dumps({"case": "gist", "nb": NG, "d": d, "nlist": NLIST, "reps": REPS, **{f"{w}_ms_{'on' if on else 'off'}": med(v) for (w, on), v in ms.items()},
                      "all_ms": {f"{w}_{on}": [round(t, 1) for t in v] for (w, on), v in ms.items()}, "same_layout": digest[0] == digest[1],
                      "same_assignment": bool(torch.equal(got[0], got[1])), "same_centroids": bool(np.array_equal(cen[0].view(np.uint32), cen[1].view(np.uint32))),
                      "last_assign_on": {w: last[w, 1] for w in ("build", "assign", "kmeans")}, "wide_mfma_flops": 2 * 2.0 * NG * NLIST * 16 * jp,
                      "wide_bytes_from_l2_per_sweep": 1.0 * ((NG + 127) // 128) * ((NLIST + 127) // 128) * 2 * 128 * jp * 32}), flush=True)
    q.close()
    del x, xb, got
    for k in ("AUNCEL_AMD_ASSIGN_FUSED", "AUNCEL_AMD_ASSIGN_WIDE"):
        os.environ.pop(k, None)

if not ONLY or ONLY == "kmeans":
    xk, _ = synth.sift_like(NK, 1, d=128)
    ms, cen = {None: [], "1": []}, {}
    for rep in range(REPS + 1):
        for fused in (None, "1"):
            os.environ.pop("AUNCEL_AMD_ASSIGN_FUSED", None)
            if fused:
                os.environ["AUNCEL_AMD_ASSIGN_FUSED"] = fused
            t, (cen[fused], _) = timed(lambda: capi.kmeans(capi.METRIC_L2, xk, NLIST, niter=5))
            if rep:
                ms[fused].append(t)
    print(json.dumps({"case": "kmeans", "n": NK, "d": 128, "k": NLIST, "niter": 5, "reps": REPS, "kmeans_ms_unset": med(ms[None]), "kmeans_ms_set": med(ms["1"]),
                      "all_ms": {str(k): [round(t, 1) for t in v] for k, v in ms.items()}, "last_assign_set": capi.kmeans_last_assign(),
                      "same_centroids": bool(np.array_equal(cen[None].view(np.uint32), cen["1"].view(np.uint32)))}), flush=True)
