"""Time of the exact range search over the whole index: 1M x 128 SIFT-like bytes under L2 and 1M x 96 DEEP-like
floats under the inner product (auncel_amd/synth.py; option exact_float = 1), IVF1024, batches of 100 / 1000 / 5000 queries at two
radii that give about 10 and about 100 results a query (the medians of the 10th and the 100th distance of search_exact over 200
queries).  At each point the median of 10 synchronising calls of (a) range_search_exact, with last_range_exact, the mean result
count and the list pass's and the collect's own time by HIP events (AUNCEL_AMD_EXACT_TIMING; "rest" is what remains of the call:
fill, copies, host work, the general way for queries beyond the slots), (b) the baseline on the same handle in the same run:
range_search with nprobe = nlist and identity keys (amd_ivf_range_search_preassigned).  Every data set is a child process of its own
under its own time limit; the first that fails ends the run.  One JSON line per point, appended to profiles/exact_range_timing.txt.
usage: python3 scripts/exact_range_timing.py [--nb N] [--out FILE] [--limit SECONDS]"""
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
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "exact_range_timing.txt")
LIMIT = int(args[args.index("--limit") + 1]) if "--limit" in args else 400
NLIST, REPS = 1024, 10
BATCHES = (100, 1000, 5000)


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
    if what == "sift":
        d, metric = 128, capi.METRIC_L2
        xb, xq = synth.sift_like(NB, 5000, d=d)
    else:
        d, metric = 96, capi.METRIC_IP
        xb, xq = synth.deep_like(NB, 5000, d=d)[:2]
    cen = synth.sample_centroids(xb, NLIST)
    h = capi.Handle(d, NLIST, metric, 0)
    h.set_centroids(cen)
    h.add(xb)
    h.set_option("exact_float", 1)
    keys = np.tile(np.arange(NLIST, dtype=np.int64), (5000, 1))
    D, _ = h.search_exact(xq[:200], 100)
    for about, col in ((10, 9), (100, 99)):
        radius = float(np.median(D[:, col]))
        for n in BATCHES:
            sys.stderr.write(f"[point] {what} about {about} n {n}\n")
            sys.stderr.flush()
            lims, _, _ = h.range_search_exact(xq[:n], radius)
            ms = median_ms(lambda: h.range_search_exact(xq[:n], radius))
            last = h.last_range_exact()
            base = median_ms(lambda: h.range_search(xq[:n], radius, NLIST, keys=keys[:n]))
            emit({"data": what, "about": about, "radius": radius, "n": n, "range_search_exact_ms": ms, "last_range_exact": last,
                  "results_per_query": round(float(lims[n]) / n, 1), "baseline_range_search_identity_keys_ms": base,
                  "speedup": round(base / ms, 2)})
    h.close()


if __name__ == "__main__":
    if "--step" in args:
        step(args[args.index("--step") + 1])
        sys.exit(0)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(f"# exact_range_timing: nb {NB}, nlist {NLIST}, medians of {REPS} synchronising calls, ONE run on one MI355X\n")
    env = dict(os.environ, AUNCEL_AMD_EXACT_TIMING="1")
    for what in ("sift", "deep"):
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", what, "--nb", str(NB), "--out", OUT]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        # the stages' own times (HIP events) of the last range_search_exact call at every point (one slice: n <= 8192): the last
        # line behind a point's mark -- the baseline's calls print nothing
        point, stages = None, {}
        for l in p.stderr.splitlines():
            if l.startswith("[point]"):
                point = l
            elif l.startswith("[range exact]") and point:
                stages[point] = l
        with open(OUT, "a") as f:
            for k, l in stages.items():
                f.write(f"# {k[8:]}: {l}\n")
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit(f"step {what} ended with status {p.returncode}: nothing further is started")
