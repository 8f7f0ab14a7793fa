"""amd_ivf_assign / amd_ivf_assign_dev (the fused matrix-core nearest-centroid pass, ivf_assign.hip) against the CPU oracle's
knn(x, cen, 1): the same centroid, the same distance bit for bit, and amd_ivf_coarse(nprobe 1, mode 0) on the same handle agreeing.
Shapes at the edges of the 32-centroid block (nlist 31 / 32 / 33), of a wave's and a workgroup's rows (n 127 / 128 / 129, 257, 300),
with a padded tail (d = 30) and beyond the pick path's 4096 centroids; option "assign_fused" 0 against 1 in its three callers."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP = 1, 0
ASSIGN_CAND = 8
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assign_kmeans_child.py")
# (nlist, n, d, metric): every value of each axis at least once, the block-edge values of nlist and n crossed
EDGES = [(nl, n, d, m) for (nl, d, m) in ((31, 30, L2), (32, 96, IP), (33, 128, L2)) for n in (127, 128, 129)]
SHAPES = EDGES + [(1, 1, 8, L2), (33, 127, 8, IP), (257, 300, 96, L2), (257, 257, 30, IP), (5000, 300, 128, L2), (5000, 129, 96, IP)]
SOME = [(33, 129, 128, L2), (32, 128, 96, IP), (257, 300, 30, L2), (5000, 300, 128, IP)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def gaussian(nlist, n, d, seed):
    """Gaussian centroids, and rows scattered around centroids drawn at random (half the centroids' spread)"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((nlist, d)).astype(np.float32)
    return cen[rng.integers(0, nlist, n)] + np.float32(0.5) * rng.standard_normal((n, d)).astype(np.float32), cen


def crowd(metric, x, cen):
    """the most centroids any (finite) row has within 4 eps of its minimum, in float64: eps = C16 (|x|^2 + max |c|^2) under L2,
    C16 |x| max |c| under the inner product, C16 = (2 d + 32) 2^-24 + 2^-10 + 2^-12 -- the pass keeps those within 2.125 eps"""
    X, Y = x[np.isfinite(x).all(axis=1) & (np.abs(x).max(axis=1) < 1e6)].astype(np.float64), cen.astype(np.float64)
    c16 = (2 * x.shape[1] + 32) * 2.0 ** -24 + 2.0 ** -10 + 2.0 ** -12
    xn, cn = (X * X).sum(1), (Y * Y).sum(1)
    v = xn[:, None] + cn[None, :] - 2 * X @ Y.T if metric == L2 else -(X @ Y.T)
    eps = c16 * (xn + cn.max()) if metric == L2 else c16 * np.sqrt(xn * cn.max())
    return int((v <= v.min(axis=1, keepdims=True) + 4 * eps[:, None]).sum(axis=1).max())


def check(capi, oracle, metric, x, cen, dev=None):
    """assign (or assign_dev of the tensor `dev`) == the oracle == coarse(nprobe 1) on one handle; -> last_assign of the assignment"""
    h = capi.Handle(cen.shape[1], cen.shape[0], metric, 0)
    h.set_centroids(cen)
    eD, eI = oracle.knn(metric, x, cen, 1)
    if dev is None:
        a, dis = h.assign(x)
    else:
        a, dis = (t.cpu().numpy() for t in h.assign_dev(dev))
    last = h.last_assign()
    assert np.array_equal(a, eI[:, 0]), np.nonzero(a != eI[:, 0])[0][:10]
    assert np.array_equal(bits(dis), bits(eD[:, 0])), np.nonzero(bits(dis) != bits(eD[:, 0]))[0][:10]
    cD, cI = h.coarse(x, 1)
    assert np.array_equal(cI, eI) and np.array_equal(bits(cD), bits(eD))
    h.close()
    assert last[0] == len(x) and last[1] + last[2] == len(x), last
    return last


@pytest.mark.parametrize("nlist,n,d,metric", SHAPES)
def test_gaussian_rows_are_decided_by_the_fused_pass(capi, oracle, nlist, n, d, metric):
    x, cen = gaussian(nlist, n, d, 7)
    assert crowd(metric, x, cen) <= ASSIGN_CAND // 2  # (a condition of the test: another seed or scale, never another cap)
    last = check(capi, oracle, metric, x, cen)
    assert last[1] == n and last[2] == 0 and last[3] >= n, last


@pytest.mark.parametrize("nlist,n,d,metric", SOME)
def test_duplicated_centroids_tie_and_the_lowest_number_wins(capi, oracle, nlist, n, d, metric):
    rng = np.random.default_rng(11)
    x = rng.integers(-8, 9, (n, d)).astype(np.float32)
    cen = rng.integers(-8, 9, (nlist, d)).astype(np.float32)
    cen[(nlist + 1) // 2:] = cen[:nlist // 2]  # every centroid of the first half has a copy in the second
    eI = oracle.knn(metric, x, cen, 1)[1][:, 0]
    assert (eI < (nlist + 1) // 2).all()
    check(capi, oracle, metric, x, cen)


@pytest.mark.parametrize("nlist,n,d,metric", SOME)
def test_pairs_one_ulp_apart_are_both_rescored(capi, oracle, nlist, n, d, metric):
    x, cen = gaussian(nlist, n, d, 13)
    cen[1::2] = cen[0:2 * (nlist // 2):2]
    j = np.arange(nlist // 2) % d
    cen[1::2, :][np.arange(nlist // 2), j] = np.nextafter(cen[1::2, :][np.arange(nlist // 2), j], np.float32(np.inf))
    assert crowd(metric, x, cen) <= ASSIGN_CAND
    last = check(capi, oracle, metric, x, cen)
    assert last[2] == 0 and last[3] >= 2 * n, last


@pytest.mark.parametrize("nlist,n,d,metric", SOME)
def test_poisoned_rows_are_flagged_one_by_one(capi, oracle, nlist, n, d, metric):
    x, cen = gaussian(nlist, n, d, 7)
    assert crowd(metric, x, cen) <= ASSIGN_CAND // 2
    rows = [0, 31, 32, 63, 64, n - 1]  # the first and the last row of a block
    for i, r in enumerate(rows):
        x[r, (5 * i) % d] = (np.nan, np.inf, 1e30)[i % 3]
    last = check(capi, oracle, metric, x, cen)
    assert last[2] == len(rows) and last[1] == n - len(rows), last


@pytest.mark.parametrize("nlist,n,d,metric", [(33, 129, 30, L2), (257, 300, 96, IP)])
def test_fp16_rows_at_an_odd_stride_from_device_memory(capi, oracle, nlist, n, d, metric):
    import torch
    x, cen = gaussian(nlist, n, d, 17)
    wide = torch.zeros((n, d + 3), dtype=torch.float16, device="cuda:0")
    wide[:, :d] = torch.from_numpy(x).to("cuda:0")
    x16 = wide[:, :d]
    assert x16.stride(0) % 2 == 1
    xf = x16.float().cpu().numpy()
    assert crowd(metric, xf, cen) <= ASSIGN_CAND // 2
    last = check(capi, oracle, metric, xf, cen, dev=x16)
    assert last[1] == n, last


@pytest.mark.parametrize("metric", [L2, IP])
def test_beyond_128_dimensions_the_general_path_serves_the_call(capi, oracle, metric):
    x, cen = gaussian(33, 129, 132, 19)
    assert check(capi, oracle, metric, x, cen) == (129, 0, 129, 0)


@pytest.mark.parametrize("caller", ["add", "build_dev"])
def test_option_assign_fused_leaves_the_callers_layout_alone(capi, caller):
    import torch
    x, cen = gaussian(257, 3000, 96, 23)
    digests = []
    for fused in (0, 1):
        h = capi.Handle(96, 257, L2, 0)
        h.set_centroids(cen)
        h.set_option("assign_fused", fused)
        if caller == "add":
            h.add(x)
            h.search(x[:8], 4, 4)  # (the lists reach the device)
            digests.append(h.layout_digest())
        else:
            b = h.build_dev(torch.from_numpy(x).to("cuda:0"))
            digests.append(b.layout_digest())
            b.close()
        last = h.last_assign()
        assert last[0] == 3000 and (last[1] > 0) == bool(fused), last
        h.close()
    assert digests[0] == digests[1]


def test_kmeans_under_the_environment_variable(tmp_path):
    """2 iterations, k = 40, n = 2000: AUNCEL_AMD_ASSIGN_FUSED unset against 1, a child process each"""
    np.save(str(tmp_path / "x.npy"), gaussian(1, 2000, 64, 29)[0])
    out = []
    for fused in (None, "1"):
        env = {k: v for k, v in os.environ.items() if k != "AUNCEL_AMD_ASSIGN_FUSED"}
        if fused:
            env["AUNCEL_AMD_ASSIGN_FUSED"] = fused
        f = str(tmp_path / f"out{fused}.npz")
        p = subprocess.run([sys.executable, CHILD, str(tmp_path / "x.npy"), f], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        out.append(np.load(f))
    assert out[0]["last"][1] == 0 and out[1]["last"][1] > 0 and out[1]["last"][0] == 4000, (out[0]["last"], out[1]["last"])
    assert np.array_equal(bits(out[0]["cen"]), bits(out[1]["cen"])) and np.array_equal(bits(out[0]["obj"]), bits(out[1]["obj"]))
