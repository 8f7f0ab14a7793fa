"""Child process of test_gpu_device_io_paths.py: runs the calls of an input .npz twice each through auncel_amd.capi on one GPU -- the
host-pointer form, then the `_dev` form on the same handle with the same options -- and writes what both returned into OUTDIR/out.npz.
No pytest and no oracle here: the parent only compares files.  The planner's knobs (AUNCEL_AMD_DIST_BUDGET_MB,
AUNCEL_AMD_SEG_CAP_PAIRS) and the exact call's candidate slots (AUNCEL_AMD_EXACT_CAP) are read once per process by the engine, which
is why these calls run in a process of their own: the parent sets them in this one's environment.

    python device_io_paths_child.py INPUT.npz OUTDIR

INPUT.npz: "manifest" (JSON: indexes = [name, d, nlist, metric], calls = [name, index, op, xq, k, ...]) and the arrays it names
("<index>/cen", "/xb", "/assign").  op "search" / "preassigned" / "resident" (nprobe, options = {key: value}) and "exact".
out.npz: per call "<call>/<side>_<field>" for side in host, dev: D, I, state (scan_arith, last_exact x 4, last_exact_detail x 4,
stats x 4, last_tie_fixed, planning passes), and "<call>/dev_io".  At the first exception the script writes the finished calls and
OUTDIR/error.txt (the traceback) and exits with status 1."""
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def state(h):
    st = h.stats()
    return np.array([h.scan_arith(), *h.last_exact(), *h.last_exact_detail(), st["nq"], st["nlist"], st["ndis"], st["nheap_updates"],
                     h.last_tie_fixed(), int(h.last_timing()["rounds"])], dtype=np.int64)


def run_call(torch, h, inp, call, done):
    xq = inp[call["xq"]]
    n, k, op = len(xq), call["k"], call["op"]
    x = torch.from_numpy(xq.copy()).cuda()
    for key, value in call.get("options", {}).items():
        h.set_option(key, value)
    keys = h.coarse(xq, call["nprobe"])[1] if op == "preassigned" else None
    for side in ("host", "dev"):
        h.stats(reset=True)
        if op == "search":
            D, I = h.search(xq, k, call["nprobe"]) if side == "host" else h.search_dev(x, k, call["nprobe"])
        elif op == "preassigned":
            D, I = h.search_preassigned(xq, k, keys) if side == "host" else h.search_preassigned_dev(x, k, torch.from_numpy(keys).cuda())
        elif op == "resident":
            if side == "host":
                h.set_queries(xq)
                D, I = h.search_resident(0, n, k, call["nprobe"])
            else:
                h.set_queries(xq[:1] * 0.5)  # (what the host call left resident must not be what the device call searches)
                h.set_queries_dev(x)
                D, I = h.search_resident_dev(0, n, k, call["nprobe"])
        elif op == "exact":
            D, I = h.search_exact(xq, k) if side == "host" else h.search_exact_dev(x, k)
        else:
            raise ValueError("unknown op " + op)
        p = call["name"] + "/" + side
        done[p + "_state"] = state(h)
        done[p + "_D"] = D if side == "host" else D.cpu().numpy()
        done[p + "_I"] = I if side == "host" else I.cpu().numpy()
    done[call["name"] + "/dev_io"] = np.array(h.last_dev_io(), dtype=np.int64)
    for key in call.get("options", {}):
        h.set_option(key, None)


def main(argv):
    inp_path, outdir = argv[1], argv[2]
    os.makedirs(outdir, exist_ok=True)
    inp = np.load(inp_path)
    manifest = json.loads(str(inp["manifest"]))
    import torch

    from auncel_amd import capi
    capi.lib()
    handles, done, rc = {}, {}, 0
    try:
        for spec in manifest["indexes"]:
            h = capi.Handle(spec["d"], spec["nlist"], spec["metric"], 0)
            h.set_centroids(inp[spec["name"] + "/cen"])
            h.set_lists_from_assign(inp[spec["name"] + "/xb"], inp[spec["name"] + "/assign"])
            handles[spec["name"]] = h
        for call in manifest["calls"]:
            run_call(torch, handles[call["index"]], inp, call, done)
    except BaseException:
        with open(os.path.join(outdir, "error.txt"), "w") as f:
            f.write(traceback.format_exc())
        traceback.print_exc()
        rc = 1
    np.savez(os.path.join(outdir, "out.npz"), **done)
    print(f"{len(manifest['calls'])} calls, exit {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv))
