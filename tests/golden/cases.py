"""Input definitions of the golden cases.  Inputs are regenerated from seeds
(auncel_amd.synth); the expected outputs in tests/golden/<case>.npz were produced by the
compiled reference through oracle/_ref/ref_harness (see make_golden.py)."""
import numpy as np

from auncel_amd import synth

METRIC_IP, METRIC_L2 = 0, 1  # reference MetricType values (Auncel/Index.h:49-52)


def _radius(xb, xq, metric, frac=0.01):
    """a range-search radius that keeps about `frac` of the (query, vector) pairs: fp32 value taken from a sample"""
    a, b = xq[:16].astype(np.float64), xb[:4000].astype(np.float64)
    if metric == METRIC_L2:
        dd = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T
        return np.array([np.quantile(dd, frac)], dtype=np.float32)
    return np.array([np.quantile(a @ b.T, 1.0 - frac)], dtype=np.float32)


def _fixed(xb, xq, nlist, nprobe, ks, metric=METRIC_L2, nshard=0, max_codes=0, cseed=99, dedup=0):
    cen = synth.sample_centroids(xb, nlist, seed=cseed)
    return dict(kind="fixed", d=xb.shape[1], nlist=nlist, nprobe=nprobe, metric=metric,
                centroids=cen, xb=xb, xq=xq, ks=np.array(ks, dtype=np.int64), nshard=nshard,
                max_codes=max_codes, radius=_radius(xb, xq, metric), dedup=dedup)


def fixed_sift_l2():
    xb, xq = synth.sift_like(20000, 64, d=128, nblobs=40, sigma=30.0, seed=11)
    return _fixed(xb, xq, 32, 4, [10, 1, 100], nshard=3, max_codes=900)


def fixed_gauss_l2_d96():
    xb, xq = synth.gauss_like(20000, 64, d=96, nblobs=200, sigma=0.6, seed=12)
    return _fixed(xb, xq, 256, 16, [10, 100], nshard=2)


def fixed_deep_ip_d96():
    xb, xq = synth.deep_like(20000, 64, d=96, nblobs=100, sigma=0.5, seed=13)
    return _fixed(xb, xq, 64, 8, [100, 10], metric=METRIC_IP, nshard=2)


def fixed_gist_l2_d960():
    xb, xq = synth.gist_like(4000, 32, d=960, nblobs=20, sigma=0.06, seed=14)
    return _fixed(xb, xq, 32, 8, [10])


def fixed_odd_d30():
    # d % 4 != 0: masked tail in fvec_L2sqr (utils_simd.cpp:405-411); integer data keeps the
    # BLAS coarse path exact
    xb, xq = synth.sift_like(6000, 40, d=30, nblobs=30, sigma=25.0, seed=15)
    return _fixed(xb, xq, 16, 5, [10])


def fixed_ragged():
    # more lists than most vectors can fill, k larger than the candidate count, nprobe > nlist
    # (coarse keys padded with -1: Heap.h:317-320)
    xb, xq = synth.sift_like(300, 40, d=16, nblobs=5, sigma=20.0, seed=16)
    return _fixed(xb, xq, 8, 12, [100, 10], nshard=2)


def fixed_dups():
    # heavy exact ties: few distinct values per dimension and duplicated rows
    rs = np.random.RandomState(17)
    base = rs.randint(0, 4, size=(500, 16)).astype(np.float32)
    xb = base[rs.randint(0, 500, size=8000)]
    xq = base[rs.randint(0, 500, size=48)] + (rs.randint(0, 2, size=(48, 16))).astype(np.float32)
    return _fixed(xb, xq, 16, 6, [10, 100], nshard=2, dedup=1)


def _auncel(xb, xq, ts, ses, runs, metric=METRIC_L2, nlist=1024, K=100, niter=10):
    return dict(kind="auncel", d=xb.shape[1], nlist=nlist, metric=metric, max_topk=K,
                train_num=ts, test_num=ses, xb=xb, xq=xq, kmeans_niter=niter,
                topks=np.array([r[0] for r in runs], dtype=np.int64),
                require_acc=np.array([r[1] for r in runs], dtype=np.float32),
                multipler=np.array([r[2] for r in runs], dtype=np.float32),
                std_m=np.array([r[3] for r in runs], dtype=np.float32))


def auncel_sift_d32():
    xb, xq = synth.sift_like(100000, 400, d=32, nblobs=300, sigma=40.0, seed=21)
    return _auncel(xb, xq, 200, 200, [(10, 0.9, 2.0, 1.0), (100, 0.95, 1.5, 2.0), (50, 0.99, 1.0, 0.5)])


def auncel_gauss_d64():
    xb, xq = synth.gauss_like(120000, 300, d=64, nblobs=400, sigma=0.8, seed=22)
    return _auncel(xb, xq, 200, 100, [(10, 0.9, 1.7, 1.0), (100, 0.9, 1.2, 3.0)])


def auncel_deep_ip_d64():
    # inner-product metric through IVF_pro: acos of the similarities, fvec_inter_vecs_IP centroid table.  max_topk stays
    # below the list sizes: a heap that still holds -FLT_MAX after the first probe makes the reference throw
    # ("arcos's domain definition is [-1, 1]", IndexIVF.cpp:562-564)
    xb, xq = synth.deep_like(100000, 300, d=64, nblobs=300, sigma=0.5, seed=23)
    return _auncel(xb, xq, 200, 100, [(10, 0.9, 1.5, 1.0), (20, 0.9, 1.2, 2.0)], metric=METRIC_IP, K=20)


def auncel_sift_nl4096():
    # BASELINE config 2's shape: nlist = 4096 changes max_num (532), the trace count (10), the coarse prefix ranking and the
    # round planner's scale.  make_golden.py trims what would not fit the repository (trim_big below).
    xb, xq = synth.sift_like(400000, 400, d=32, nblobs=1200, sigma=45.0, seed=24)
    c = _auncel(xb, xq, 200, 200, [(10, 0.95, 1.0, 0.5), (10, 0.9, 1.2, 1.0)], nlist=4096, niter=8)
    c["big"] = 1
    return c


BIG_KEEP_COLS = 704  # coarse ranking columns kept for big cases: the probe loop ends by floor(nlist / 8 * multipler) <= 614


def trim_big(out, case):
    """golden tensors of a `big` case that are O(nlist^2) or O(nq * nlist): replaced by digests / the part the tests read"""
    import hashlib
    ts = case["train_num"]
    t = out.pop("interdis_cem")
    out["interdis_cem_sha"] = np.array(hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest())
    out["interdis_cem_sample"] = t[::4099].copy()
    for k in ("coarse_dis_sse", "coarse_keys_sse"):
        out[k + "_test"] = out.pop(k)[ts:, :BIG_KEEP_COLS].copy()
    for k in ("coarse_dis_blas_train", "coarse_keys_blas_train", "train_D", "train_I", "cenTocen"):
        out.pop(k, None)
    for k in [k for k in out if k.startswith("raw_trace") or k.endswith("_batched")]:
        out.pop(k)
    return out


def _kmeans(x, k, niter, metric=METRIC_L2, spherical=0, max_pts=256, seed=1234):
    return dict(kind="kmeans", d=x.shape[1], k=k, niter=niter, metric=metric, spherical=spherical,
                max_points_per_centroid=max_pts, seed=seed, x=x)


def kmeans_toy():
    # fewer than 20 points: the reference assigns through its exact (non-BLAS) path, so every bit is pinned
    xb, _ = synth.gauss_like(19, 1, d=8, nblobs=4, sigma=0.5, seed=41)
    return _kmeans(xb, 4, 6)


def kmeans_void():
    # duplicates: clusters run empty and are split off bigger ones (km_update_centroids, utils.cpp:1126-1159)
    rs = np.random.RandomState(42)
    base = rs.randint(0, 6, size=(3, 8)).astype(np.float32)
    x = base[rs.randint(0, 3, size=18)]
    return _kmeans(x, 6, 5)


def kmeans_toy_ip():
    xb, _ = synth.deep_like(18, 1, d=16, nblobs=3, sigma=0.5, seed=43)
    return _kmeans(xb, 3, 5, metric=METRIC_IP, spherical=1)


def kmeans_sub_int():
    # sub-sampling (n > k * max_points_per_centroid) and the BLAS assignment path: integer data, objective pinned loosely
    xb, _ = synth.sift_like(4000, 1, d=16, nblobs=24, sigma=20.0, seed=44)
    return _kmeans(xb, 24, 8, max_pts=100)


def kmeans_sub_int_d100():
    # d = 100 (two blocks of 64 dimensions, not a multiple of 64), k = 300 past coarse_pick's lower bound, sub-sampled;
    # integer data with more tight blobs than clusters: the reference's BLAS assignment picks the exact kernel's centroids
    # in every iteration (with fewer blobs than clusters, split blobs make near-ties on which the two disagree)
    xb, _ = synth.sift_like(20000, 1, d=100, nblobs=600, sigma=4.0, seed=45)
    return _kmeans(xb, 300, 6, max_pts=40)


def kmeans_ip_spherical_d96():
    # IP + spherical at d = 96, sub-sampled, more blobs than clusters (the BLAS and exact rankings agree on the best centroid)
    xb, _ = synth.deep_like(6000, 1, d=96, nblobs=200, sigma=0.1, seed=46)
    return _kmeans(xb, 100, 5, metric=METRIC_IP, spherical=1, max_pts=50)


def io_ragged():
    c = fixed_ragged()
    c["kind"] = "io"
    return c


def io_sift():
    xb, xq = synth.sift_like(3000, 4, d=32, nblobs=10, sigma=30.0, seed=31)
    c = _fixed(xb, xq, 16, 4, [10])
    c["kind"] = "io"
    return c


def _worlds():
    import os
    import sys
    tests = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import extreme_range_cases
    return extreme_range_cases


def _extreme(metric, cen, xb, xq, radius):
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return dict(kind="fixed", d=24, nlist=4, nprobe=4, metric=metric, centroids=f(cen), xb=f(xb), xq=f(xq), ks=np.array([10, 1], dtype=np.int64),
                nshard=0, max_codes=0, radius=np.array([radius], dtype=np.float32), dedup=0)


def extreme_l2_d24():
    # the ends of the fp32 range under L2 (tests/extreme_range_cases.py at d = 24): norms that overflow, a NaN / +inf / -inf element,
    # all-zero and non-finite queries, subnormal distances (a reference build that flushed them would return zeros).  19 rows: the
    # reference assigns fewer than 20 through its exact path.  The radius is a subnormal.
    X = _worlds()
    big, sub, odd = X.world("l2_norm_overflow", 24), X.world("subnormal", 24), X.world("nonfinite_l2", 24)
    kinds = {k: r for r, k in sorted(odd["planted"].items(), reverse=True)}
    rows = np.nonzero(big["assign"] < 3)[0][:9]
    xb = np.concatenate([big["xb"][rows], odd["xb"][[kinds["nan"], kinds["+inf"], kinds["-inf"], kinds["overflow"]]],
                         sub["xb"][np.nonzero(sub["assign"] == 0)[0][:6]]])
    cen = np.concatenate([big["cen"][:3], sub["cen"][:1]])
    xq = np.concatenate([big["xb"][rows[:2]] * np.float32(1.0001), big["xq"][:1], odd["xq"][[X.Q_NAN, X.Q_INF, X.Q_ZERO]], sub["xq"][:1], sub["xq"][20:21]])
    return _extreme(METRIC_L2, cen, xb, xq, 2.0 ** -127)


def extreme_ip_d24():
    # ... under the inner product: products whose single-chain sum overflows while the reference's four chains stay finite, rows whose
    # product is +inf (admitted as the best) and -inf (never), NaN / +-inf elements
    X = _worlds()
    big, odd = X.world("ip_norm_overflow", 24), X.world("nonfinite_ip", 24)
    kinds = {k: r for r, k in sorted(odd["planted"].items(), reverse=True)}
    pl = {k: r for r, k in sorted(big["planted"].items(), reverse=True)}
    rows = np.nonzero(big["assign"] < 2)[0][:10]
    xb = np.concatenate([big["xb"][rows], big["xb"][[pl["+inf"], pl["-inf"]]], odd["xb"][[kinds["nan"], kinds["+inf"], kinds["-inf"], kinds["overflow"]]],
                         odd["xb"][np.nonzero(odd["assign"] == 0)[0][1:4]]])
    cen = np.concatenate([big["cen"][:2], odd["cen"][:2]])
    own = np.nonzero((big["xq"][:, 0] > 0) & (big["xq"][:, 1] > 0))[0][:4]  # (queries of groups 0 and 1: all coordinates but the last two positive)
    xq = np.concatenate([big["xq"][own], odd["xq"][[X.Q_NAN, X.Q_INF, X.Q_ZERO]], odd["xq"][:1]])
    return _extreme(METRIC_IP, cen, xb, xq, 0.0)


CASES = {f.__name__: f for f in [extreme_l2_d24, extreme_ip_d24, io_ragged, io_sift, fixed_sift_l2, fixed_gauss_l2_d96, fixed_deep_ip_d96, fixed_gist_l2_d960,
                                  fixed_odd_d30, fixed_ragged, fixed_dups, auncel_sift_d32, auncel_gauss_d64, auncel_deep_ip_d64, auncel_sift_nl4096, kmeans_toy, kmeans_void, kmeans_toy_ip, kmeans_sub_int,
                                  kmeans_sub_int_d100, kmeans_ip_spherical_d96]}


def input_sha(case):
    arrs = [case[k] for k in ("xb", "xq", "x") if k in case]
    if "centroids" in case:
        arrs.append(case["centroids"])
    return synth.sha(*arrs)
