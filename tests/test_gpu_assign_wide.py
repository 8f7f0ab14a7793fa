"""amd_ivf_assign / amd_ivf_assign_dev beyond 128 dimensions under option "assign_wide" = 1 (assign_rows16_kernel + assign_wide_kernel,
DESIGN.md 18.1) against the CPU oracle's knn(x, cen, 1): the same centroid, the same distance bit for bit.  d at the piece and stage
edges of a stage of 6 pieces (130: 9 pieces padded to 10 and d % 4 != 0; 132; 176: 11 to 12; 192: two full stages; 516; 960: ten
full stages; 1024: 64 pieces), nlist below, at and above the four waves' blocks (1, 31, 32, 33, 129: a second tile with one live
wave, 257, 5000), n at the edges of a workgroup's 128 rows.  The data and its precondition are test_gpu_assign.py's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_assign import ASSIGN_CAND, CHILD, IP, L2, bits, capi, crowd, gaussian  # noqa: F401 (capi: the fixture)

pytestmark = pytest.mark.gpu

# (nlist, n, d, metric)
SHAPES = [(1, 1, 1024, L2), (129, 1, 130, IP), (31, 127, 130, L2), (32, 128, 132, IP), (33, 129, 132, L2), (31, 128, 176, IP),
          (33, 127, 192, L2), (129, 129, 516, IP), (257, 300, 960, L2), (257, 257, 960, IP), (33, 300, 1024, L2), (5000, 300, 1024, IP)]
SOME = [(33, 300, 132, L2), (257, 300, 960, IP)]


def check(capi, oracle, metric, x, cen, dev=None):
    """assign (or assign_dev of the tensor `dev`) with assign_wide = 1 == the oracle; -> last_assign"""
    h = capi.Handle(cen.shape[1], cen.shape[0], metric, 0)
    h.set_centroids(cen)
    h.set_option("assign_wide", 1)
    eD, eI = oracle.knn(metric, x, cen, 1)
    a, dis = h.assign(x) if dev is None else (t.cpu().numpy() for t in h.assign_dev(dev))
    last = tuple(h.last_assign())
    h.close()
    assert np.array_equal(a, eI[:, 0]), np.nonzero(a != eI[:, 0])[0][:10]
    assert np.array_equal(bits(dis), bits(eD[:, 0])), np.nonzero(bits(dis) != bits(eD[:, 0]))[0][:10]
    return last


@pytest.mark.parametrize("nlist,n,d,metric", SHAPES)
def test_gaussian_rows_are_decided_by_the_wide_pass(capi, oracle, nlist, n, d, metric):
    x, cen = gaussian(nlist, n, d, 7)
    assert crowd(metric, x, cen) <= ASSIGN_CAND // 2  # (a condition of the test: another seed, never another cap)
    last = check(capi, oracle, metric, x, cen)
    assert last[:3] == (n, n, 0) and last[3] >= n, last


@pytest.mark.parametrize("nlist,n,d,metric", SOME)
def test_duplicated_centroids_tie_and_the_lowest_number_wins(capi, oracle, nlist, n, d, metric):
    rng = np.random.default_rng(11)
    x = rng.integers(-8, 9, (n, d)).astype(np.float32)
    cen = rng.integers(-8, 9, (nlist, d)).astype(np.float32)
    cen[(nlist + 1) // 2:] = cen[:nlist // 2]  # every centroid of the first half has a copy in the second
    assert (oracle.knn(metric, x, cen, 1)[1][:, 0] < (nlist + 1) // 2).all()
    last = check(capi, oracle, metric, x, cen)
    assert last[0] == n and last[1] + last[2] == n, last


@pytest.mark.parametrize("nlist,n,d,metric", SOME)
def test_poisoned_rows_are_flagged_one_by_one(capi, oracle, nlist, n, d, metric):
    x, cen = gaussian(nlist, n, d, 7)
    assert crowd(metric, x, cen) <= ASSIGN_CAND // 2
    rows = [0, 31, 32, 127, 128, n - 1]  # the first and the last row of a block and of a workgroup's 128
    for i, r in enumerate(rows):
        x[r, (5 * i) % d] = (np.nan, np.inf, 1e30)[i % 3]
    assert check(capi, oracle, metric, x, cen)[:3] == (n, n - len(rows), len(rows))


@pytest.mark.parametrize("nlist,n,d,metric", [(33, 129, 130, L2), (257, 300, 516, IP)])
def test_fp16_rows_at_an_odd_stride_from_device_memory(capi, oracle, nlist, n, d, metric):
    import torch
    x, cen = gaussian(nlist, n, d, 17)
    wide = torch.zeros((n, d + 3), dtype=torch.float16, device="cuda:0")
    wide[:, :d] = torch.from_numpy(x).to("cuda:0")
    x16 = wide[:, :d]
    assert x16.stride(0) % 2 == 1
    xf = x16.float().cpu().numpy()
    assert crowd(metric, xf, cen) <= ASSIGN_CAND // 2
    assert check(capi, oracle, metric, xf, cen, dev=x16)[:3] == (n, n, 0)


@pytest.mark.parametrize("metric", [L2, IP])
def test_beyond_1024_dimensions_the_general_path_serves_the_call(capi, oracle, metric):
    x, cen = gaussian(33, 129, 1028, 19)
    assert check(capi, oracle, metric, x, cen) == (129, 0, 129, 0)


@pytest.mark.parametrize("caller", ["add", "build_dev"])
def test_the_options_leave_the_callers_layout_alone(capi, caller):
    import torch
    x, cen = gaussian(257, 3000, 132, 23)
    digests = []
    for on in (0, 1):
        h = capi.Handle(132, 257, L2, 0)
        h.set_centroids(cen)
        h.set_option("assign_fused", on)
        h.set_option("assign_wide", on)
        if caller == "add":
            h.add(x)
            h.search(x[:8], 4, 4)  # (the lists reach the device)
            digests.append(h.layout_digest())
        else:
            b = h.build_dev(torch.from_numpy(x).to("cuda:0"))
            digests.append(b.layout_digest())
            b.close()
        last = h.last_assign()
        assert last[0] == 3000 and (last[1] > 0) == bool(on), last
        h.close()
    assert digests[0] == digests[1]


def test_kmeans_under_the_environment_variables(tmp_path):
    """2 iterations, k = 40, n = 2000, d = 132: AUNCEL_AMD_ASSIGN_FUSED and AUNCEL_AMD_ASSIGN_WIDE unset against 1, a child process each"""
    np.save(str(tmp_path / "x.npy"), gaussian(1, 2000, 132, 29)[0])
    names, out = ("AUNCEL_AMD_ASSIGN_FUSED", "AUNCEL_AMD_ASSIGN_WIDE"), []
    for on in (False, True):
        env = {k: v for k, v in os.environ.items() if k not in names}
        env.update({k: "1" for k in names if on})
        f = str(tmp_path / f"out{int(on)}.npz")
        p = subprocess.run([sys.executable, CHILD, str(tmp_path / "x.npy"), f], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        out.append(np.load(f))
    assert out[0]["last"][1] == 0 and out[1]["last"][1] > 0 and out[1]["last"][0] == 4000, (out[0]["last"], out[1]["last"])
    assert np.array_equal(bits(out[0]["cen"]), bits(out[1]["cen"])) and np.array_equal(bits(out[0]["obj"]), bits(out[1]["obj"]))
