"""Time of the exact search over the whole index: 1M x 128 SIFT-like bytes (auncel_amd/synth.py), IVF1024, batches of
100 / 1000 / 5000 queries at k = 10 and 100.  At each point the median of 10 synchronising calls of (a) search_exact at
exact_seed_nprobe 1, 4, 16 and 64, with last_exact's four counts, the largest per-point candidate count per query and the list pass's
and the selection's own time (AUNCEL_AMD_EXACT_TIMING), (b) the general way on the same build: search_preassigned with identity
keys, (c) bench.ground_truth (torch matmul + topk).  Every step is a child process of its own under its own time limit; the first
step that fails ends the run.  One JSON line per point, appended to profiles/exact_timing.txt.
usage: python3 scripts/exact_timing.py [--nb N] [--out FILE]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = sys.argv[1:]
NB = int(args[args.index("--nb") + 1]) if "--nb" in args else 1_000_000
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "exact_timing.txt")
NLIST, D, REPS = 1024, 128, 10
POINTS = [(n, k) for n in (100, 1000, 5000) for k in (10, 100)]


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def median_ms(f):
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def step(what):
    import numpy as np
    from auncel_amd import capi, synth
    xb, xq = synth.sift_like(NB, 5000, d=D)
    if what == "torch":
        import torch
        import bench
        dev = torch.device("cuda")
        tb, tq = torch.from_numpy(xb).to(dev), torch.from_numpy(xq).to(dev)
        for n, k in POINTS:
            bench.ground_truth(torch, tb, tq[:n], k)
            emit({"what": "bench.ground_truth", "n": n, "k": k, "ms": median_ms(lambda: bench.ground_truth(torch, tb, tq[:n], k))})
        return
    cen = synth.sample_centroids(xb, NLIST)
    h = capi.Handle(D, NLIST, capi.METRIC_L2, 0)
    h.set_centroids(cen)
    h.add(xb)
    keys = np.tile(np.arange(NLIST, dtype=np.int64), (5000, 1))
    for n, k in POINTS:
        if what == "general":
            h.search_preassigned(xq[:n], k, keys[:n])
            emit({"what": "general (search_preassigned, identity keys)", "n": n, "k": k,
                  "ms": median_ms(lambda: h.search_preassigned(xq[:n], k, keys[:n]))})
        else:
            h.set_option("exact_seed_nprobe", int(what))
            h.search_exact(xq[:n], k)
            ms = median_ms(lambda: h.search_exact(xq[:n], k))
            last = h.last_exact()
            seed_ms = median_ms(lambda: h.search(xq[:n], k, int(what), coarse_mode=-1))
            emit({"what": "search_exact", "seed_nprobe": int(what), "n": n, "k": k, "ms": ms, "last_exact": last,
                  "candidates_per_served_query": round(last[3] / max(1, n), 1), "seed_search_alone_ms": seed_ms})
    h.close()


if __name__ == "__main__":
    if "--step" in args:
        step(args[args.index("--step") + 1])
        sys.exit(0)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(f"# exact_timing: nb {NB}, nlist {NLIST}, d {D}, medians of {REPS} synchronising calls, ONE run on one MI355X\n")
    env = dict(os.environ, AUNCEL_AMD_EXACT_TIMING="1")
    for what in ("16", "1", "4", "64", "general", "torch"):
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--step", what, "--nb", str(NB), "--out", OUT]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        stages = [l for l in p.stderr.splitlines() if l.startswith("[exact]")]
        last = {l.split(":")[0]: l for l in stages}  # the stages' own times of the last call at every point (HIP events)
        with open(OUT, "a") as f:
            for l in last.values():
                f.write("# " + l + "\n")
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit(f"step {what} ended with status {p.returncode}: nothing further is started")
