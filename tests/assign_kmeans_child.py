"""Child process of test_gpu_assign.py: capi.kmeans over the rows of INPUT.npy (k = 40, 2 iterations, L2), centroids and the
assignment counters into OUTPUT.npz.  The handle amd_ivf_kmeans makes is its own, so option "assign_fused" reaches it only through
AUNCEL_AMD_ASSIGN_FUSED, which the parent sets (or not) in this process's environment.

    python assign_kmeans_child.py INPUT.npy OUTPUT.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

if __name__ == "__main__":
    from auncel_amd import capi
    cen, obj = capi.kmeans(capi.METRIC_L2, np.load(sys.argv[1]), 40, niter=2)
    np.savez(sys.argv[2], cen=cen, obj=obj, last=np.array(capi.kmeans_last_assign(), dtype=np.int64))
