"""Time of the exact search under an id selector: 1M x 128 SIFT-like bytes and 1M x 96 DEEP-like floats (inner
product, option exact_float = 1) of auncel_amd/synth.py, IVF1024, batches of 100 / 1000 / 5000 queries at k = 10 and 100, under
selectors that keep 1 %, 10 %, 50 % and 100 % of the entries (ID_MOD 100 / 10 / 2 / 1).  At each point the median of 10
synchronising calls of (a) search_exact_selected, with last_exact, last_exact_detail and the seed nprobe the rule gives; (b)
search_preassigned_selected with identity keys -- the only way before the call existed; (c) search_exact on subset(the same
selector).  Making the selector and cutting the subset are timed on their own, once per kept fraction (medians of 5).  A data set is
a child process of its own under its own time limit; the first that fails ends the run.  One JSON line per point, appended to
profiles/exact_selected_timing.txt.
usage: python3 scripts/exact_selected_timing.py [--nb N] [--out FILE]"""
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
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "exact_selected_timing.txt")
NLIST, REPS, SEED = 1024, 10, 16
POINTS = [(n, k) for n in (100, 1000, 5000) for k in (10, 100)]
MODS = [100, 10, 2, 1]  # id % m == 0: one in m is kept


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def median_ms(f, reps=REPS):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def step(what):
    import numpy as np
    from auncel_amd import capi, synth
    if what == "bytes":
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
    h.search_exact(xq[:100], 10)  # (every derived copy of the lists is made before anything is timed)
    for m in MODS:
        made = []

        def make():
            made.append(h.selector(capi.SUBSET_ID_MOD, m, 0))

        create_ms = median_ms(make, 5)
        for s in made[1:]:
            s.close()
        s = made[0]
        kept = s.info()[1]
        cut = []
        subset_ms = median_ms(lambda: cut.append(h.subset(capi.SUBSET_ID_MOD, m, 0)), 5)
        for x in cut[1:]:
            x.close()
        sub = cut[0]
        emit({"what": "creation", "data": what, "kept_fraction": 1.0 / m, "kept": kept, "selector_create_ms": create_ms, "subset_ms": subset_ms,
              "seed_nprobe_under_the_selector": -(-SEED * NB // kept)})
        for n, k in POINTS:
            row = {"data": what, "kept_fraction": 1.0 / m, "n": n, "k": k}
            h.search_exact_selected(s, xq[:n], k)
            row["search_exact_selected_ms"] = median_ms(lambda: h.search_exact_selected(s, xq[:n], k))
            row["last_exact"], row["last_exact_detail"] = h.last_exact(), h.last_exact_detail()
            h.search_preassigned_selected(s, xq[:n], k, keys[:n])
            row["search_preassigned_selected_ms"] = median_ms(lambda: h.search_preassigned_selected(s, xq[:n], k, keys[:n]))
            sub.search_exact(xq[:n], k)
            row["subset_search_exact_ms"] = median_ms(lambda: sub.search_exact(xq[:n], k))
            row["subset_last_exact"] = sub.last_exact()
            emit(row)
        sub.close()
        s.close()
    h.close()


if __name__ == "__main__":
    if "--step" in args:
        step(args[args.index("--step") + 1])
        sys.exit(0)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(f"# exact_selected_timing: nb {NB}, nlist {NLIST}, exact_seed_nprobe {SEED}, medians of {REPS} synchronising calls, ONE run on one MI355X\n")
    for what in ("bytes", "float"):
        cmd = ["timeout", "-k", "10", "280", sys.executable, os.path.abspath(__file__), "--step", what, "--nb", str(NB), "--out", OUT]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit(f"step {what} ended with status {p.returncode}: nothing further is started")
