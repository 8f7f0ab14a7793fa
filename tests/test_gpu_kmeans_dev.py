"""amd_ivf_kmeans_dev against the oracle's restatement of Clustering::train (gemm=False): the same centroid bits and the same
objective bits in every iteration, at the smallest shapes at which the device-side loop (ivf_kmeans_dev.hip) can go wrong -- the
update kernel's column slabs and staged runs, the counting sort's tiles, void clusters, sub-sampling, post-processing, fp16 and
strided input, the finite check.  Most of the time goes to the oracle, on the CPU."""
import os

import numpy as np
import pytest

ORACLE_THREADS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "8") or 8)))
IP, L2 = 0, 1

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_both(capi, oracle, x, k, *, metric=L2, niter=3, seed=1234, max_pts=256, spherical=False, int_centroids=False, t=None):
    """capi.kmeans_dev on the GPU tensor t (default: x uploaded as it is) and oracle.kmeans on x, the same values as fp32 on the
    host.  Where the training set has exactly k points both give the first k rows of x and no objective."""
    import torch
    if t is None:
        t = torch.from_numpy(x).cuda()
    cen, obj = capi.kmeans_dev(metric, t, k, niter, seed, max_pts, spherical, int_centroids)
    ocen, oobj = oracle.kmeans(metric, x, k, niter, seed, max_pts, spherical, int_centroids, gemm=False, nthreads=ORACLE_THREADS)
    assert cen.device == t.device and cen.dtype == torch.float32
    bad_obj = np.nonzero(bits(obj) != bits(oobj))[0]
    assert bad_obj.size == 0, f"objective differs from iteration {bad_obj[0]}: {obj[bad_obj[0]]!r} vs {oobj[bad_obj[0]]!r}"
    bad_rows = np.nonzero((bits(cen.cpu().numpy()) != bits(ocen)).any(axis=1))[0]
    assert bad_rows.size == 0, f"{bad_rows.size} centroid rows differ, first {bad_rows[:8].tolist()}"
    return cen


# the update kernel's one, two and four columns a lane, its slab edges, rows at stride dpad, the wide assignment beyond 128
@pytest.mark.parametrize("d,metric", [(1, L2), (3, IP), (63, L2), (64, IP), (65, L2), (132, IP), (260, L2)])
def test_dimensions(capi, oracle, d, metric):
    from auncel_amd import synth
    x, _ = synth.gauss_like(5000, 1, d=d, nblobs=150, sigma=0.6, seed=100 + d)
    run_both(capi, oracle, x, 100, metric=metric)


# the counting sort's 1024-row tiles; with 7 clusters some runs are longer than one staged piece of idx (512) and than the unroll
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_sort_tile_edges(capi, oracle, n):
    from auncel_amd import synth
    x, _ = synth.gauss_like(n, 1, d=8, nblobs=5, sigma=0.8, seed=200 + n)
    run_both(capi, oracle, x, 7, max_pts=1024)


@pytest.mark.parametrize("n,k", [(3000, 1), (3000, 1000)], ids=["one_run_of_all", "runs_of_0_to_3"])
def test_run_lengths(capi, oracle, n, k):
    from auncel_amd import synth
    x, _ = synth.gauss_like(n, 1, d=20, nblobs=40, sigma=0.5, seed=300 + k)
    run_both(capi, oracle, x, k, max_pts=4096)


# fewer distinct points than clusters: many splits an iteration (the two data sets of test_gpu_kmeans.py)
@pytest.mark.parametrize("kind", ["int", "float"])
def test_void_clusters(capi, oracle, kind):
    rs = np.random.RandomState(800 if kind == "int" else 510)
    base = rs.randint(0, 40, size=(300, 16)).astype(np.float32) if kind == "int" else rs.standard_normal((300, 24)).astype(np.float32)
    x = base[rs.randint(0, 300, size=20000)]
    run_both(capi, oracle, x, 512, niter=6)


@pytest.mark.parametrize("n,max_pts,niter", [(1600, 20, 4), (1601, 20, 4), (5000, 1, 4), (80, 256, 4), (3000, 256, 0), (3000, 256, 1)],
                         ids=["n_eq_k_max_pts", "one_more_subsampled", "nx_eq_k", "n_eq_k", "niter0", "niter1"])
def test_subsampling_and_iteration_edges(capi, oracle, n, max_pts, niter):
    from auncel_amd import synth
    x, _ = synth.gauss_like(n, 1, d=24, nblobs=60, sigma=0.5, seed=600 + n)
    run_both(capi, oracle, x, 80, niter=niter, max_pts=max_pts)


@pytest.mark.parametrize("d", [16, 96])
def test_spherical_ip(capi, oracle, d):
    from auncel_amd import synth
    x, _ = synth.deep_like(4000, 1, d=d, nblobs=128, sigma=0.4, seed=800 + d)
    run_both(capi, oracle, x, 64, metric=IP, spherical=True, niter=4)


def test_int_centroids_on_bytes(capi, oracle):
    """from the second iteration on both operands of the assignment are integers in range: the fused arithmetic may be chosen"""
    x = np.random.RandomState(901).randint(0, 256, size=(6000, 64)).astype(np.float32)
    run_both(capi, oracle, x, 64, int_centroids=True, niter=4)


@pytest.mark.parametrize("form", ["fp16_odd_stride", "fp32_ldx_gt_d"])
def test_input_forms(capi, oracle, form):
    import torch
    from auncel_amd import synth
    x, _ = synth.gauss_like(3000, 1, d=24, nblobs=60, sigma=0.5, seed=950)
    if form == "fp16_odd_stride":
        wide = torch.full((3000, 27), 7.0, dtype=torch.float16, device="cuda")
        wide[:, :24] = torch.from_numpy(x).cuda().half()
        x = wide[:, :24].float().cpu().numpy()  # (the values the call reads, widened)
    else:
        wide = torch.full((3000, 32), 7.0, dtype=torch.float32, device="cuda")
        wide[:, :24] = torch.from_numpy(x).cuda()
    t = wide[:, :24]
    assert t.stride(0) == wide.shape[1]
    run_both(capi, oracle, x, 40, max_pts=50, t=t)


def test_non_finite_beyond_the_sample(capi, oracle):
    """the sample has 4 rows, so at least one of five rows is outside it: each of them refuses the call, which works again after"""
    from auncel_amd import synth
    x, _ = synth.gauss_like(2000, 1, d=12, nblobs=10, sigma=0.5, seed=960)
    for row, bad in zip((100, 500, 900, 1300, 1999), (np.nan, np.inf, -np.inf, np.nan, np.inf)):
        y = x.copy()
        y[row, row % 12] = bad
        with pytest.raises(capi.EngineError, match="input contains NaN's or Inf's") as e:
            run_both(capi, oracle, y, 2, max_pts=2)
        assert e.value.code == -2
    run_both(capi, oracle, x, 2, max_pts=2)


def test_against_the_host_call(capi, oracle):
    import torch
    from auncel_amd import synth
    x, _ = synth.gauss_like(6000, 1, d=40, nblobs=90, sigma=0.5, seed=970)
    cen, obj = capi.kmeans(L2, x, 50, 4, 1234, 100)
    dcen, dobj = capi.kmeans_dev(L2, torch.from_numpy(x).cuda(), 50, 4, 1234, 100)
    assert np.array_equal(bits(dcen.cpu().numpy()), bits(cen)) and np.array_equal(bits(dobj), bits(obj))
