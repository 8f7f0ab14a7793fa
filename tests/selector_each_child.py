"""Child process of test_gpu_selector_each.py's deferred-queries test: one mixed call under a selector per query, in a process of its
own because the planner's knobs (AUNCEL_AMD_DIST_BUDGET_MB, AUNCEL_AMD_SEG_CAP_PAIRS) are read once per process; the parent sets them
in this one's environment.  No oracle here: the parent holds the expected values and compares.

    python selector_each_child.py CASE OUT.npz SELECTOR [SELECTOR ...]

The case and the selectors are the parent's own recipes (test_gpu_update.make_case, test_gpu_subset.selector); sel_of is the parent's
seeded draw, read from sel_of.npy beside OUT.npz.  OUT.npz: per entry point D and I, the planning passes
of the call (last_timing()["rounds"]) and its statistics."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv):
    name, out, sel_names = argv[1], argv[2], argv[3:]
    from auncel_amd import capi
    capi.lib()
    from test_gpu_subset import selector
    from test_gpu_update import K, NPROBE, Model, handle, make_case
    metric, cen, assign, xb, xq = make_case(name)
    sel_of = np.load(os.path.join(os.path.dirname(out), "sel_of.npy"))
    model = Model(cen.shape[0], cen.shape[1], xb, assign)
    h = handle(capi, metric, cen, xb, assign, 1)
    sels = [h.selector(*selector(capi, s, model)[0]) for s in sel_names]
    done = {}
    for byte in (1, 0):
        h.set_byte_codes(byte)
        h.stats(reset=True)
        D, I = h.search_selected_each(sels, sel_of, xq, K, NPROBE)
        st = h.stats()
        done[f"b{byte}/D"], done[f"b{byte}/I"] = D, I
        done[f"b{byte}/rounds"] = np.array(h.last_timing()["rounds"], dtype=np.float64)
        done[f"b{byte}/stats"] = np.array([st["nq"], st["nlist"], st["ndis"], st["nheap_updates"]], dtype=np.int64)
    for s in sels:
        s.close()
    h.close()
    np.savez(out, **done)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
