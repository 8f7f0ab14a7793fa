"""Child process of test_gpu_exact_range.py: builds the indexes of an input .npz through auncel_amd.capi on one GPU, runs
range_search_exact over the query sets it names and writes (lims, labels, distances, last_range_exact) of every call into an output
.npz.  No pytest and no oracle here: the parent holds the expected values and only compares.  AUNCEL_AMD_EXACT_CAP is read once per
process by the engine, which is why these calls run in a process of their own: the parent sets it in this one's environment.

    python exact_range_child.py INPUT.npz OUTPUT.npz

INPUT.npz: "manifest" (JSON list of calls: name, metric, cen, xb, assign, xq, radius) and the arrays it names."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv):
    inp = np.load(argv[1])
    from auncel_amd import capi
    capi.lib()
    out = {}
    for call in json.loads(str(inp["manifest"])):
        cen = inp[call["cen"]]
        h = capi.Handle(cen.shape[1], cen.shape[0], call["metric"], 0)
        h.set_centroids(cen)
        h.set_lists_from_assign(inp[call["xb"]], inp[call["assign"]])
        lims, labels, dist = h.range_search_exact(inp[call["xq"]], call["radius"])
        name = call["name"]
        out[name + "/lims"], out[name + "/labels"], out[name + "/dist"] = lims, labels, dist
        out[name + "/last"] = np.array(h.last_range_exact(), dtype=np.int64)
        h.close()
    np.savez(argv[2], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
