"""Time of a search from and into device memory against the same search from host memory: the benchmark's index
shape -- SIFT-like bytes (auncel_amd/synth.py), 10M x 128, IVF4096 -- at n = 1 and n = 5000 queries, k = 10, nprobe = 32.  At each
point the median of REPS synchronising calls, alternating the three forms in one process: (a) search_dev on a GPU tensor, results
into GPU tensors, (b) search from pageable host memory, (c) search from page-locked host memory into page-locked results.  Beside
them set_queries_dev alone -- the ingest launches, the 12-byte read-back and its synchronisation -- with the bytes the ingest moves
(n * d * 4 read, n * dpad * 4 written) over that time as a share of the HBM peak (8 TB/s): a call time, so a lower bound of the
kernel's own rate.  One JSON line per point, appended to profiles/device_io_timing.txt.  A run without a GPU fails.
usage: python3 scripts/device_io_timing.py [--nb N] [--nlist N] [--out FILE]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = sys.argv[1:]
NB = int(args[args.index("--nb") + 1]) if "--nb" in args else 10_000_000
NLIST = int(args[args.index("--nlist") + 1]) if "--nlist" in args else 4096
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "device_io_timing.txt")
D, K, NPROBE, REPS, WARM = 128, 10, 32, 30, 5
HBM_PEAK = 8.0e12  # bytes / s


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def main():
    import numpy as np
    import torch
    from auncel_amd import capi, synth
    if not torch.cuda.is_available():
        sys.exit("device_io_timing: no GPU")
    xb, xq = synth.sift_like(NB, 5000, d=D)
    cen = synth.sample_centroids(xb, NLIST)
    h = capi.Handle(D, NLIST, capi.METRIC_L2, 0)
    h.set_centroids(cen)
    h.add(xb)
    with open(OUT, "a") as f:
        f.write(f"# device_io_timing: nb {NB}, nlist {NLIST}, d {D}, k {K}, nprobe {NPROBE}; medians of {REPS} synchronising calls after "
                f"{WARM} warm-up calls, the forms alternating; ONE run on one MI355X\n")
    for n in (1, 5000):
        x_host = np.ascontiguousarray(xq[:n])
        x_pin = torch.from_numpy(x_host.copy()).pin_memory()
        D_pin, I_pin = torch.empty((n, K), dtype=torch.float32).pin_memory(), torch.empty((n, K), dtype=torch.int64).pin_memory()
        x_dev = x_pin.cuda()
        out = (torch.empty((n, K), dtype=torch.float32, device="cuda"), torch.empty((n, K), dtype=torch.int64, device="cuda"))
        L = capi.lib()
        import ctypes as C

        def pinned():
            capi._chk(L.amd_ivf_search(h._h, C.c_size_t(n), C.c_void_p(x_pin.data_ptr()), C.c_size_t(K), C.c_size_t(NPROBE), 0,
                                       C.c_void_p(D_pin.data_ptr()), C.c_void_p(I_pin.data_ptr())))

        forms = {"search_dev": lambda: h.search_dev(x_dev, K, NPROBE, out=out), "search, pageable": lambda: h.search(x_host, K, NPROBE),
                 "search, page-locked": pinned, "set_queries_dev alone": lambda: h.set_queries_dev(x_dev)}
        ts = {name: [] for name in forms}
        for rep in range(WARM + REPS):
            for name, f in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()  # (every form returns after the engine's stream has finished)
                if rep >= WARM:
                    ts[name].append((time.perf_counter() - t0) * 1e3)
        # the three forms computed the same thing
        want = h.search(x_host, K, NPROBE)
        got = h.search_dev(x_dev, K, NPROBE, out=out)
        assert np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
        assert h.last_dev_io()[:2] == [0, 0]
        row = {"n": n, "k": K, "nprobe": NPROBE}
        for name, v in ts.items():
            row[name + " ms"] = round(statistics.median(v), 4)
            row[name + " min ms"] = round(min(v), 4)
        moved = n * D * 4 + n * ((D + 3) // 4 * 4) * 4
        row["ingest bytes"] = moved
        row["ingest call: share of HBM peak"] = round(moved / (row["set_queries_dev alone ms"] * 1e-3) / HBM_PEAK, 6)
        emit(row)
    h.close()


if __name__ == "__main__":
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    main()
