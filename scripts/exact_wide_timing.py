"""Time of the exact search over float lists BEYOND 128 DIMENSIONS: auncel_amd/synth.py's GIST-like data, nb x 960
(1M by default), IVF1024, under the inner product and under L2; batches of 100 / 1000 / 5000 queries at k = 10 and 100.  At each point
the median of 10 synchronising calls of (a) search_exact with the workgroup-tiled fp16 list pass (options exact_float = 1 and
exact_wide = 1), with last_exact, last_exact_detail and the pass's and the selection's own time (AUNCEL_AMD_EXACT_TIMING); (b) the same
build with exact_wide = 0: the general way; (c) with --baseline-lib FILE: search_exact of that library -- the commit before the pass,
built from a checkout of it -- on the same data, which (b) must agree with (the same code path).  Beside the pass's time its
roofline: the fp16 copy streamed once per tile of 128 queries, and n x ntotal x d x 2 FLOP.  Every step is a child process of its own
under its own time limit; the first step that fails ends the run.  One JSON line per point, appended to profiles/exact_wide_timing.txt.
usage: python3 scripts/exact_wide_timing.py [--nb N] [--out FILE] [--baseline-lib FILE] [--limit SECONDS]"""
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
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "exact_wide_timing.txt")
BASELINE = args[args.index("--baseline-lib") + 1] if "--baseline-lib" in args else None
LIMIT = args[args.index("--limit") + 1] if "--limit" in args else "300"
NLIST, D, REPS = 1024, 960, 10
POINTS = [(n, k) for n in (100, 1000, 5000) for k in (10, 100)]
HBM_BYTES_PER_S, FP16_FLOP_PER_S = 8.0e12, 2.5e15  # MI355X: peak HBM3E bandwidth, dense fp16 matrix rate


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


def step(what, metric_name):
    from auncel_amd import capi, synth
    xb, xq = synth.gist_like(NB, 5000, d=D)[:2]
    metric = capi.METRIC_IP if metric_name == "ip" else capi.METRIC_L2
    cen = synth.sample_centroids(xb, NLIST)
    h = capi.Handle(D, NLIST, metric, 0)
    h.set_centroids(cen)
    h.add(xb)
    h.set_option("exact_float", 1)
    if what != "baseline":  # (the library of the commit before does not know the key)
        h.set_option("exact_wide", 1 if what == "pass" else 0)
    pieces = (D + 15) // 16  # filter_steps16 beyond 128 dimensions (even: 60): KiB per 32-vector block of the fp16 copy
    pieces += pieces & 1
    for n, k in POINTS:
        h.search_exact(xq[:n], k)
        row = {"what": {"pass": "search_exact, wide fp16 pass", "off": "search_exact, exact_wide = 0 (general way)",
                        "baseline": "search_exact of the baseline library"}[what], "metric": metric_name, "n": n, "k": k,
               "ms": median_ms(lambda: h.search_exact(xq[:n], k)), "last_exact": h.last_exact(), "last_exact_detail": h.last_exact_detail()}
        if what == "pass":
            tiles = (n + 127) // 128
            row["roofline_ms"] = {"bytes": round(tiles * (NB / 32) * pieces * 1024 / HBM_BYTES_PER_S * 1e3, 4),
                                  "flop": round(n * NB * D * 2 / FP16_FLOP_PER_S * 1e3, 4)}
        emit(row)
    h.close()


if __name__ == "__main__":
    if "--step" in args:
        i = args.index("--step")
        step(args[i + 1], args[i + 2])
        sys.exit(0)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(f"# exact_wide_timing: GIST-like floats, nb {NB}, nlist {NLIST}, d {D}, medians of {REPS} synchronising calls, ONE run on one MI355X\n")
    for metric_name in ("ip", "l2"):
        for what in ("pass", "off") + (("baseline",) if BASELINE else ()):
            env = dict(os.environ, AUNCEL_AMD_EXACT_TIMING="1")
            if what == "baseline":
                env["AUNCEL_AMD_LIB"] = os.path.abspath(BASELINE)
            cmd = ["timeout", "-k", "10", LIMIT, sys.executable, os.path.abspath(__file__), "--step", what, metric_name, "--nb", str(NB), "--out", OUT]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            stages = [l for l in p.stderr.splitlines() if l.startswith("[exact]")]
            last = {l.split(":")[0]: l for l in stages}  # the stages' own times of the last call at every point (HIP events)
            with open(OUT, "a") as f:
                for l in last.values():
                    f.write(f"# {metric_name} {what} " + l + "\n")
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-3000:])
                sys.exit(f"step {what} {metric_name} ended with status {p.returncode}: nothing further is started")
