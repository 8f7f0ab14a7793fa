"""Child process of test_gpu_exact_selected.py: builds the indexes of an input .npz through auncel_amd.capi on one GPU, makes the
selector every call names, runs search_exact_selected over the call's queries and writes (D, I, last_exact, last_exact_detail) into an
output .npz.  No pytest and no oracle here: the parent holds the expected values and only compares.  AUNCEL_AMD_EXACT_CAP is read once
per process by the engine, which is why these calls run in a process of their own: the parent sets it (or AUNCEL_AMD_EXACT_SEED) in
this one's environment.  (tests/exact_child.py issues the unfiltered call only.)

    python exact_selected_child.py INPUT.npz OUTPUT.npz

INPUT.npz: "manifest" (JSON list of calls: name, metric, cen, xb, assign, xq, k, kind, a1, a2, sel -- sel the name of an array or
null) and the arrays it names."""
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
        with h.selector(call["kind"], call["a1"], call["a2"], inp[call["sel"]] if call["sel"] else None) as s:
            D, I = h.search_exact_selected(s, inp[call["xq"]], call["k"])
            out[call["name"] + "/D"], out[call["name"] + "/I"] = D, I
            out[call["name"] + "/last"] = np.array(h.last_exact(), dtype=np.int64)
            out[call["name"] + "/detail"] = np.array(h.last_exact_detail(), dtype=np.int64)
        h.close()
    np.savez(argv[2], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
