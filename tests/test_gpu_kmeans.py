"""amd_ivf_kmeans against the oracle's restatement of Clustering::train at the shapes that real indexes are trained at.

With coarse_mode 0 the engine promises the exact SSE-order assignment arithmetic (include/auncel_amd.h), and the oracle
with gemm=False assigns through that same arithmetic, so the centroids and every iteration's objective must be the same
bits at any size -- whichever device path the assignment takes (coarse_pick's approximate ranking with exact recompute, or
the exact kernel), however many clusters run empty, whatever the sub-sampling.  The oracle itself is pinned to the
compiled reference by tests/test_oracle_golden.py::test_kmeans.  The cases are named for the path they reach; most of the
time goes to the oracle, on the CPU."""
import os
import re

import numpy as np
import pytest

from util import load_case

# AUNCEL_TEST_SEED_OFFSET=<n>: the random sweep's 40 shapes drawn from other seeds (one-off fuzzing after kernel changes)
SEED_OFFSET = int(os.environ.get("AUNCEL_TEST_SEED_OFFSET", "0"))
# the oracle's CPU threads: what the job may use (OMP_NUM_THREADS), at most 16
ORACLE_THREADS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "8") or 8)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP, L2 = 0, 1  # the reference's MetricType values, as capi.METRIC_IP / capi.METRIC_L2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    assert (capi.METRIC_IP, capi.METRIC_L2) == (IP, L2)
    return capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- which assignment path a k-means iteration takes (coarse_dev in ivf_engine.hip, nprobe = 1, coarse_mode 0, prefix 0)
DIST_BUDGET_FLOATS = 768 << 20  # amd_ivf::dist_budget_floats


def assignment_path(nx, k):
    """coarse_dev's condition restated: coarse_pick (fp16 approximate ranking, candidates recomputed exactly, rows with
    equal distances flagged and redone exactly) when n >= 256, nprobe <= 128, nlist <= 4096, nlist >= 4 * nprobe + 64 and
    n * nlist within the distance budget; the exact per-pair kernel otherwise"""
    nprobe = 1
    if nx >= 256 and nprobe <= 128 and k <= 4096 and k >= 4 * nprobe + 64 and nx * k <= DIST_BUDGET_FLOATS:
        return "coarse_pick"
    return "exact"


def test_assignment_path_restatement_matches_the_engine():
    """the restatement above is the engine's condition (if this fails, update assignment_path and the cases' intents)"""
    src = open(os.path.join(ROOT, "auncel_amd", "csrc", "ivf_engine.hip")).read()
    assert "size_t dist_budget_floats = (size_t)768 << 20;" in src
    cond = re.sub(r"\s+", " ", src[src.index("if (!gemm && !h->in_coarse_pick"):src.index("size_t t = h->timer.begin(CAT_COARSE, s);")])
    for part in ("n >= 256", "nprobe <= 128", "nlist <= 4096", "nlist >= 4 * nprobe + 64", "prefix == 0",
                 "n * nlist <= h->dist_budget_floats"):
        assert part in cond, part


def training_size(n, k, max_pts):
    return k * max_pts if n > k * max_pts else n


# ---- the comparison
def run_both(capi, oracle, x, k, *, metric=L2, niter=4, seed=1234, max_pts=256, spherical=False, int_centroids=False, what=""):
    """capi.kmeans (coarse_mode 0) and oracle.kmeans (gemm=False) on the same input: the same centroid bits, the same
    objective bits in every iteration.  Returns the centroids."""
    n, d = x.shape
    nx = training_size(n, k, max_pts)
    shape = (f"{what}: n={n} nx={nx} d={d} k={k} metric={metric} niter={niter} seed={seed} max_pts={max_pts} "
             f"spherical={spherical} int_centroids={int_centroids} path={assignment_path(nx, k)}")
    cen, obj = capi.kmeans(metric, x, k, niter, seed, max_pts, spherical, int_centroids, coarse_mode=0, device=0)
    ocen, oobj = oracle.kmeans(metric, x, k, niter, seed, max_pts, spherical, int_centroids, gemm=False, nthreads=ORACLE_THREADS)
    if nx == k:
        # the reference's corner case: the centroids are the first k rows of x_in (not of the sample), no objective
        assert np.array_equal(bits(cen), bits(x[:k])), shape
        assert np.array_equal(bits(ocen), bits(x[:k])), shape
        assert not obj.any() and not oobj.any(), shape
        return cen
    bad_obj = np.nonzero(bits(obj) != bits(oobj))[0]
    assert bad_obj.size == 0, f"{shape}: objective differs from iteration {bad_obj[0]}: {obj[bad_obj[0]]!r} vs {oobj[bad_obj[0]]!r}"
    bad_rows = np.nonzero((bits(cen) != bits(ocen)).any(axis=1))[0]
    assert bad_rows.size == 0, f"{shape}: {bad_rows.size} centroid rows differ, first {bad_rows[:8].tolist()}"
    return cen


# ---- dimensions: kmeans_sums_kernel's blockIdx.y > 0, d not dividing 64, rows at stride dpad
@pytest.mark.parametrize("d,metric", [(1, L2), (3, L2), (4, IP), (17, L2), (63, L2), (64, IP), (65, L2), (100, L2), (128, IP),
                                      (129, L2), (960, L2)])
def test_dimensions(capi, oracle, d, metric):
    from auncel_amd import synth
    # generic float data: sums are rounded, so only the ascending point order gives the oracle's bits
    x, _ = synth.gauss_like(5000, 1, d=d, nblobs=150, sigma=0.6, seed=100 + d)
    assert assignment_path(5000, 100) == "coarse_pick"
    run_both(capi, oracle, x, 100, metric=metric, niter=5, what=f"dimensions d={d}")


# ---- k across the coarse_pick bounds (68 = 4 * nprobe + 64, 4096) and the radix sort's bit boundaries (2^m, 2^m + 1)
K_CASES = [
    (1, "exact"),           # one cluster: every point the same key, a 1-bit sort
    (2, "exact"),
    (67, "exact"),          # one below coarse_pick's lower bound
    (68, "coarse_pick"),    # its lower bound
    (255, "coarse_pick"),
    (256, "coarse_pick"),   # 8 sort bits
    (257, "coarse_pick"),   # 9 sort bits
    (1024, "coarse_pick"),
    (4096, "coarse_pick"),  # nlist <= 4096: the upper bound
    (4097, "exact"),        # one above it, 13 sort bits
]


@pytest.mark.parametrize("k,path", K_CASES, ids=[f"k{k}_{p}" for k, p in K_CASES])
def test_k_boundaries(capi, oracle, k, path):
    from auncel_amd import synth
    n = max(2000, 16 * k)
    assert assignment_path(n, k) == path
    x, _ = synth.gauss_like(n, 1, d=32, nblobs=max(8, k // 2), sigma=0.5, seed=200 + k)
    run_both(capi, oracle, x, k, niter=3 if k < 1024 else 2, what=f"k={k}")


# ---- the distance budget: n * k just within and just beyond 768 Mi floats, on the same data
@pytest.mark.parametrize("n,path", [(DIST_BUDGET_FLOATS // 4096, "coarse_pick"), (DIST_BUDGET_FLOATS // 4096 + 1, "exact")],
                         ids=["at_budget_coarse_pick", "past_budget_exact"])
def test_distance_budget(capi, oracle, n, path):
    from auncel_amd import synth
    assert assignment_path(n, 4096) == path
    x, _ = synth.gauss_like(DIST_BUDGET_FLOATS // 4096 + 1, 1, d=32, nblobs=3000, sigma=0.5, seed=300)
    run_both(capi, oracle, x[:n], 4096, niter=2, max_pts=1024, what="budget")


# ---- bench.py's training shape: sift-like, k = 4096, 256 points per centroid sub-sampled out of more than a million
def test_bench_shape(capi, oracle):
    from auncel_amd import synth
    x, _ = synth.sift_like(1_200_000, 1, d=128, nblobs=20000, sigma=18.0, seed=400)
    assert training_size(len(x), 4096, 256) == 1 << 20 and assignment_path(1 << 20, 4096) == "exact"  # beyond the budget
    run_both(capi, oracle, x, 4096, niter=1, what="bench shape")


def test_bench_shape_subsampled_below_budget(capi, oracle):
    from auncel_amd import synth
    x, _ = synth.sift_like(300_000, 1, d=128, nblobs=20000, sigma=18.0, seed=401)
    assert training_size(len(x), 4096, 32) == 131072 and assignment_path(131072, 4096) == "coarse_pick"
    run_both(capi, oracle, x, 4096, niter=2, max_pts=32, what="bench shape, 32 per centroid")


# ---- void clusters at scale: fewer distinct points than clusters, seeds that repeat, many splits per iteration
@pytest.mark.parametrize("distinct", [300, 530])
def test_void_clusters(capi, oracle, distinct):
    rs = np.random.RandomState(500 + distinct)
    base = rs.randint(0, 40, size=(distinct, 16)).astype(np.float32)
    x = base[rs.randint(0, distinct, size=20000)]
    assert assignment_path(20000, 512) == "coarse_pick"
    run_both(capi, oracle, x, 512, niter=6, what=f"{distinct} distinct points")


def test_void_clusters_float(capi, oracle):
    # the same with float values: split centroids are 2^-10 apart relatively, their sums rounded
    rs = np.random.RandomState(510)
    base = rs.standard_normal((300, 24)).astype(np.float32)
    x = base[rs.randint(0, 300, size=20000)]
    run_both(capi, oracle, x, 512, niter=6, what="300 distinct float points")


# ---- sub-sampling edges and iteration counts
@pytest.mark.parametrize("n,max_pts,what", [(1600, 20, "n = k * max_pts, no sub-sampling"),
                                            (1601, 20, "n = k * max_pts + 1, sub-sampled"),
                                            (5000, 1, "max_pts = 1: nx == k, first k rows of x_in"),
                                            (80, 256, "n == k")])
def test_subsampling_edges(capi, oracle, n, max_pts, what):
    from auncel_amd import synth
    x, _ = synth.gauss_like(n, 1, d=24, nblobs=60, sigma=0.5, seed=600 + n)
    run_both(capi, oracle, x, 80, niter=4, max_pts=max_pts, what=what)


@pytest.mark.parametrize("niter", [0, 1, 25])
def test_iteration_count(capi, oracle, niter):
    from auncel_amd import synth
    x, _ = synth.gauss_like(3000, 1, d=24, nblobs=50, sigma=0.5, seed=700)
    cen = run_both(capi, oracle, x, 40, niter=niter, what=f"niter={niter}")
    if niter == 0:  # the seeds: rows rand_perm(nx, seed + 1) picks (and nothing else ran)
        assert len(np.unique(bits(cen), axis=0)) == 40 and all((x == c).all(axis=1).any() for c in cen)


# ---- post-processing: spherical (IP) and int_centroids
@pytest.mark.parametrize("d", [16, 96, 128])
@pytest.mark.parametrize("k", [64, 1000])
def test_spherical_ip(capi, oracle, d, k):
    from auncel_amd import synth
    x, _ = synth.deep_like(max(4000, 20 * k), 1, d=d, nblobs=2 * k, sigma=0.4, seed=800 + d + k)
    run_both(capi, oracle, x, k, metric=IP, spherical=True, niter=4, what="spherical")


@pytest.mark.parametrize("kind", ["sift", "bytes"])
def test_int_centroids(capi, oracle, kind):
    """rounded centroids on integer points: from the second iteration on the assignment's operands are integers in range,
    and the engine may take its fused arithmetic (centroid_range.fusable_with) -- still the reference's bits"""
    from auncel_amd import synth
    if kind == "sift":
        x, _ = synth.sift_like(30000, 1, d=128, nblobs=400, sigma=18.0, seed=900)
    else:
        x = np.random.RandomState(901).randint(0, 256, size=(20000, 64)).astype(np.float32)
    run_both(capi, oracle, x, 256, int_centroids=True, niter=5, what=f"int_centroids {kind}")


# ---- random sweep
SWEEP_COST = 4e9  # n * k * d * niter: a few tenths of a second of the oracle per case


def make_sweep_case(seed):
    rs = np.random.RandomState(5000 + SEED_OFFSET + seed)
    d = int(rs.choice([1, 2, 5, 8, 16, 31, 32, 48, 64, 65, 96, 128, 200]))
    k = int(rs.choice([1, 3, 16, 50, 67, 68, 100, 127, 128, 129, 300, 512, 1000, 1500]))
    metric = int(rs.choice([L2, IP]))
    spherical = bool(metric == IP and rs.rand() < 0.6)
    int_centroids = bool(rs.rand() < 0.25)
    kind = str(rs.choice(["float", "bytes", "smallint", "dups"]))
    max_pts = int(rs.choice([1, 2, 5, 39, 256]))
    niter = int(rs.randint(0, 7))
    n = int(rs.choice([k, k + 1, 3 * k, 10 * k, 40 * k, 100 * k, 256 * k + 7]))
    n = max(k, min(n, int(SWEEP_COST / max(1, k * d * max(niter, 1)))), 1)
    if kind == "float":
        x = rs.standard_normal((n, d)).astype(np.float32)
    elif kind == "bytes":
        x = rs.randint(0, 256, size=(n, d)).astype(np.float32)
    elif kind == "smallint":
        x = rs.randint(-20, 21, size=(n, d)).astype(np.float32)
    else:
        base = rs.randint(0, 5, size=(max(2, n // 20), d)).astype(np.float32)
        x = base[rs.randint(0, len(base), size=n)]
    return dict(x=x, k=k, metric=metric, niter=niter, seed=int(rs.randint(0, 1 << 30)), max_pts=max_pts, spherical=spherical,
                int_centroids=int_centroids, kind=kind)


@pytest.mark.parametrize("seed", range(40))
def test_random_sweep(capi, oracle, seed):
    c = make_sweep_case(seed)
    run_both(capi, oracle, c["x"], c["k"], metric=c["metric"], niter=c["niter"], seed=c["seed"], max_pts=c["max_pts"],
             spherical=c["spherical"], int_centroids=c["int_centroids"], what=f"sweep {seed} ({c['kind']})")


# ---- coarse_mode -1: the reference's own switch takes its exact path below 20 points, so the goldens hold bit for bit
@pytest.mark.parametrize("name", ["kmeans_toy", "kmeans_void", "kmeans_toy_ip"])
def test_reference_switch_on_the_goldens(capi, name):
    case, gold = load_case(name)
    assert case["x"].shape[0] < 20 and case["d"] % 4 == 0
    cen, obj = capi.kmeans(case["metric"], case["x"], case["k"], case["niter"], case["seed"], case["max_points_per_centroid"],
                           bool(case["spherical"]), coarse_mode=-1, device=0)
    assert np.array_equal(bits(cen), bits(gold["centroids"]))
    assert np.array_equal(bits(obj), bits(gold["obj"]))


# ---- coarse_mode 1: the matrix cores' |x|^2 + |y|^2 - 2xy, first objective only
def gamma(m):
    u = 2.0 ** -24
    return m * u / (1 - m * u)


@pytest.mark.parametrize("metric", [L2, IP])
def test_matrix_core_objective(capi, oracle, metric):
    """The seeds are the same bits on both sides, so obj[0] = fp32 sum over points of each point's best distance to the
    seeds differs only by how those distances are rounded.  Bound (standard forward error analysis, u = 2^-24,
    gamma(m) = m u / (1 - m u)), for a point x and a centroid c of dimension d:
      L2, exact SSE order: fl(sum_j fl(fl(x_j - c_j)^2)) is within gamma(d + 2) |x - c|^2 <= gamma(d + 2) (|x| + |c|)^2 of
          |x - c|^2;  matrix cores: |x|^2, |c|^2 and x.c each within gamma(d) of |x|^2, |c|^2, |x||c|, then two more
          roundings, so within gamma(d + 2) (|x| + |c|)^2.  The two differ by at most 2 gamma(d + 2) (|x| + |c|)^2.
      IP: both are dot products of length d in some order, each within gamma(d) |x||c|: differ by 2 gamma(d) |x||c|.
    The best of the k distances moves by at most the largest per-centroid difference (a clamp of a negative L2 value to 0
    only moves it closer), so per point e_i = that bound with |c| the largest seed norm.  The objective is a running fp32
    sum over nx points in the same order on both sides: each sum is within gamma(nx - 1) sum |m_i| of the exact one, so
      |obj_gemm - obj_exact| <= sum_i e_i + gamma(nx - 1) (2 sum_i |m_i| + sum_i e_i),
    with sum |m_i| bounded by the exact objective's magnitude (plus its own rounding).  Later iterations start from
    different centroids and are not compared."""
    from auncel_amd import synth
    if metric == L2:
        x, _ = synth.gauss_like(20000, 1, d=64, nblobs=300, sigma=0.5, seed=1000)
    else:
        x, _ = synth.deep_like(20000, 1, d=96, nblobs=300, sigma=0.4, seed=1001)
    n, d = x.shape
    k = 256
    _, obj = capi.kmeans(metric, x, k, 2, 1234, 256, False, False, coarse_mode=1, device=0)
    _, oobj = oracle.kmeans(metric, x, k, 1, 1234, 256, False, False, gemm=False, nthreads=ORACLE_THREADS)
    xn = np.linalg.norm(x.astype(np.float64), axis=1)
    cmax = xn.max()  # the seeds are rows of x
    if metric == L2:
        e = 2 * gamma(d + 2) * (xn + cmax) ** 2
    else:
        e = 2 * gamma(d) * xn * cmax
    # sum |m_i|: for L2 the objective itself (all terms >= 0); for IP |m_i| <= |x_i| cmax
    mags = abs(float(oobj[0])) * (1 + gamma(n)) if metric == L2 else float((xn * cmax).sum())
    bound = e.sum() + gamma(n - 1) * (2 * mags + e.sum())
    diff = abs(float(obj[0]) - float(oobj[0]))
    assert diff <= bound, f"metric={metric}: |{obj[0]!r} - {oobj[0]!r}| = {diff} > {bound} (relative {bound / abs(float(oobj[0]))})"
