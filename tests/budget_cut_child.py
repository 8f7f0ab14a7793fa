"""Child process of test_gpu_budget_cut.py: runs the calls of an input .npz through auncel_amd.capi on one GPU and writes what
they returned, one .npz per group of calls, into an output directory.  No pytest and no oracle here: the parent process holds the
expected values and only compares files.  The planner's knobs (AUNCEL_AMD_DIST_BUDGET_MB, AUNCEL_AMD_SEG_CAP_PAIRS) are read once
per process by the engine, which is why the calls run in a process of their own: the parent sets them in this one's environment.

    python budget_cut_child.py INPUT.npz OUTDIR

INPUT.npz: "manifest" (JSON: indexes, groups of calls) and the arrays the manifest names.  OUTDIR/<group>.npz: per call
"<call>/<field>" arrays and "<call>/rounds" (last_timing()["rounds"]: planning passes of the call).  At the first exception the
script writes the group's finished calls and OUTDIR/error.txt (the traceback) and exits with status 1."""
import json
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# per-call environment of the engine options that are read per call (Options::get in ivf_engine.hip)
PER_CALL_ENV = ("AUNCEL_AMD_FIXED_ROUNDS", "AUNCEL_AMD_SELECT")


def make_index(capi, inp, spec):
    name = spec["name"]
    h = capi.Handle(spec["d"], spec["nlist"], spec["metric"], 0)
    h.set_centroids(inp[name + "/cen"])
    h.set_lists_from_assign(inp[name + "/xb"], inp[name + "/assign"])
    if spec.get("ntraces"):
        traces = [(inp[f"{name}/tr{i}_x"], inp[f"{name}/tr{i}_y"], inp[f"{name}/tr{i}_s"]) for i in range(spec["ntraces"])]
        h.set_interdis(None)
        h.set_tuner(spec["K"], traces, capi.arcos_table())
    return h


def run_call(capi, inp, h, call):
    """one engine call -> {field: array}"""
    op = call["op"]
    xq = inp[call["xq"]]
    keys = inp[call["keys"]] if "keys" in call else None
    out = {}
    h.stats(reset=True)
    if op == "pre":
        out["D"], out["I"] = h.search_preassigned(xq, call["k"], keys, store_pairs=call["store_pairs"], max_codes=call["max_codes"])
    elif op == "range":
        out["lims"], out["lab"], out["dis"] = h.range_search(xq, call["radius"], call["nprobe"], keys=keys)
    elif op == "range_sel":
        with h.selector(capi.SUBSET_ID_MOD, 3, 0) as s:
            out["lims"], out["lab"], out["dis"] = h.range_search_selected(s, xq, call["radius"], call["nprobe"], keys=keys)
    elif op == "selected":
        with h.selector(capi.SUBSET_ID_MOD, 3, 0) as s:
            out["D"], out["I"] = h.search_selected(s, xq, call["k"], call["nprobe"])
    elif op == "timed":
        n = xq.shape[0]
        h.set_queries(xq)
        out["D"], out["I"], used = h.search_timed(0, n, call["k"], call["nprobe"], np.full(n, 1e9, np.float32))
        out["used"] = used.astype(np.int64)
    elif op == "adaptive":
        n = xq.shape[0]
        h.set_queries(xq)
        my_np = np.zeros(n, dtype=np.uint64)
        t_rec = np.zeros(n, dtype=np.float32)
        out["D"], out["I"] = h.search_adaptive(0, n, call["query_topk"], call["multipler"], call["std_m"], inp[call["req"]], my_np, t_rec,
                                               gt_D=inp[call["gt"]], profile=call["profile"])
        out["my_nprobe"] = my_np.astype(np.int64)
        out["t_recalls"] = t_rec
    elif op == "train":
        n, K, ntr = xq.shape[0], call["K"], call["ntraces"]
        h.set_queries(xq)
        raw = [np.full((n * (K // 4), 2), -1, dtype=np.float32) for _ in range(ntr)]
        out["D"], out["I"] = h.train_samples(0, n, K, inp[call["gt"]], n, raw)
        for i, r in enumerate(raw):
            out[f"raw{i}"] = r
    else:
        raise ValueError("unknown op " + op)
    st = h.stats()
    out["stats"] = np.array([st["nlist"], st["ndis"], st["nheap_updates"]], dtype=np.int64)
    out["rounds"] = np.array(h.last_timing()["rounds"], dtype=np.float64)
    return out


def main(argv):
    inp_path, outdir = argv[1], argv[2]
    os.makedirs(outdir, exist_ok=True)
    inp = np.load(inp_path)
    manifest = json.loads(str(inp["manifest"]))
    from auncel_amd import capi
    capi.lib()
    specs = {s["name"]: s for s in manifest["indexes"]}
    handles = {}
    for group in manifest["groups"]:
        done = {}
        t0 = time.time()
        try:
            for call in group["calls"]:
                if call["index"] not in handles:
                    handles[call["index"]] = make_index(capi, inp, specs[call["index"]])
                for key in PER_CALL_ENV:
                    os.environ.pop(key, None)
                os.environ.update(call.get("env", {}))
                for field, value in run_call(capi, inp, handles[call["index"]], call).items():
                    done[call["name"] + "/" + field] = value
        except BaseException:
            with open(os.path.join(outdir, "error.txt"), "w") as f:
                f.write(f"group {group['name']}\n" + traceback.format_exc())
            np.savez(os.path.join(outdir, group["name"] + ".partial.npz"), **done)
            traceback.print_exc()
            return 1
        done["seconds"] = np.array(time.time() - t0)
        np.savez(os.path.join(outdir, group["name"] + ".npz"), **done)
        print(f"{group['name']}: {len(group['calls'])} calls, {time.time() - t0:.2f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
