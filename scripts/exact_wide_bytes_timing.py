"""Time of the exact search over BYTE-CODED lists beyond 128 dimensions: byte-valued rows 0 .. 132 around byte
centroids, nb x 960 (200 000 by default), IVF1024, under the inner product and under L2; batches of 100 / 1000 / 5000 queries at
k = 10 and 100.  At each point the median of 10 synchronising calls of (a) search_exact with the workgroup-tiled byte list pass
(option exact_wide_bytes = 1), with last_exact, last_exact_detail and the pass's and the selection's own time
(AUNCEL_AMD_EXACT_TIMING); (b) the same build with exact_wide_bytes = 0: the general way; (c) with --baseline-lib FILE: search_exact
of that library -- the commit before the pass, built from a checkout of it -- on the same data, which (b) must agree with (the same
code path: how far the two differ is the run's noise).  Beside the pass's time its roofline: the byte fragments streamed once per
tile of 128 queries at 8 TB/s, and 2 n ntotal d int8 operations at the dense int8 matrix rate (twice the fp16 one).  Every step is a
child process of its own under its own time limit; the first step that fails ends the run.  One JSON line per point, appended to
profiles/exact_wide_bytes_timing.txt.
usage: python3 scripts/exact_wide_bytes_timing.py [--nb N] [--out FILE] [--baseline-lib FILE] [--limit SECONDS]"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = sys.argv[1:]
NB = int(args[args.index("--nb") + 1]) if "--nb" in args else 200_000
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "exact_wide_bytes_timing.txt")
BASELINE = args[args.index("--baseline-lib") + 1] if "--baseline-lib" in args else None
LIMIT = args[args.index("--limit") + 1] if "--limit" in args else "300"
NLIST, D, REPS, TOP = 1024, 960, 10, 132  # (960 x 132^2 <= 2^24: the byte rule holds)
POINTS = [(n, k) for n in (100, 1000, 5000) for k in (10, 100)]
HBM_BYTES_PER_S, INT8_OP_PER_S = 8.0e12, 5.0e15  # MI355X: peak HBM3E bandwidth, dense int8 matrix rate


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


def data():
    rs = np.random.RandomState(960)
    cen = rs.randint(0, TOP + 1, size=(NLIST, D))
    assign = rs.randint(0, NLIST, size=NB)
    xb = np.clip(cen[assign] + rs.randint(-16, 17, size=(NB, D)), 0, TOP).astype(np.float32)
    xq = np.clip(cen[rs.randint(0, NLIST, size=5000)] + rs.randint(-16, 17, size=(5000, D)), 0, TOP).astype(np.float32)
    return cen.astype(np.float32), assign, xb, xq


def step(what, metric_name):
    from auncel_amd import capi
    cen, assign, xb, xq = data()
    metric = capi.METRIC_IP if metric_name == "ip" else capi.METRIC_L2
    h = capi.Handle(D, NLIST, metric, 0)
    h.set_centroids(cen)
    h.set_lists_from_assign(xb, assign)
    if what != "baseline":  # (the library of the commit before does not know the key)
        h.set_option("exact_wide_bytes", 1 if what == "pass" else 0)
    pieces = (D + 31) // 32  # mfma_ksteps: KiB per 32-vector block of the byte fragments
    for n, k in POINTS:
        h.search_exact(xq[:n], k)
        row = {"what": {"pass": "search_exact, wide byte pass", "off": "search_exact, exact_wide_bytes = 0 (general way)",
                        "baseline": "search_exact of the baseline library"}[what], "metric": metric_name, "n": n, "k": k,
               "ms": median_ms(lambda: h.search_exact(xq[:n], k)), "last_exact": h.last_exact(), "last_exact_detail": h.last_exact_detail()}
        if what == "pass":
            tiles = (n + 127) // 128
            row["roofline_ms"] = {"bytes": round(tiles * (NB / 32) * pieces * 1024 / HBM_BYTES_PER_S * 1e3, 4),
                                  "int8": round(n * NB * D * 2 / INT8_OP_PER_S * 1e3, 4)}
        emit(row)
    assert h.scan_arith() == 2, "the byte codes are not in use"
    h.close()


if __name__ == "__main__":
    if "--step" in args:
        i = args.index("--step")
        step(args[i + 1], args[i + 2])
        sys.exit(0)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(f"# exact_wide_bytes_timing: bytes 0 .. {TOP}, nb {NB}, nlist {NLIST}, d {D}, medians of {REPS} synchronising calls, ONE run on one MI355X\n")
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
