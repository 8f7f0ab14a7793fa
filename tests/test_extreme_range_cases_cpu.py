"""The premise of tests/test_gpu_extreme_range.py, without a GPU: the worlds of tests/extreme_range_cases.py are what they claim to
be, checked against the pinned oracle alone.  These are conditions on the inputs (a world that missed one would be drawn from another
seed), not measurements of the engine.

  * worlds with finite neighbours (l2_norm_overflow, ip_norm_overflow, subnormal, integers_2p62): for at least half of the queries at
    least 3 of the true top 10 over the 8 probed lists lie in lists ranked second or later -- a threshold round that drops
    candidates changes the result;
  * l2_norm_overflow / integers_2p62: |x|^2 and |y|^2 are +inf in fp32, every query's 10th distance is finite;
  * ip_norm_overflow: |x| |y| overflows for the pairs of one group while the reference's value is finite; the planted +inf rows are
    admitted as the best, the -inf rows never;
  * subnormal: at least a third of all top-10 distances are nonzero subnormals at every d, zeros occur, and beyond 24 dimensions
    values at and above 2^-126 occur as well;
  * nonfinite_*: a planted row is in an expected result only under the inner product, with the value +inf (or against the all-zero
    query, where an overflowing row's product is 0); no expected distance is a NaN or, under L2, an infinity; every clean query's
    result is full;
  * the keep-test model (extreme_range_cases.keep_model: the filter's two tests as they stood before non-finite operands were
    kept), run at each query's threshold after the dense first round, drops a true neighbour in at least 16 of the 64 queries of
    l2_norm_overflow, ip_norm_overflow and integers_2p62 -- after one dense probe (the filter off in that round) and after two (what
    the engine's rule gives these shapes): the GPU test can fail, and the keep rule as it stood loses neighbours on these cases.
    Observed (queries, entries) after one / two dense probes:
        l2_norm_overflow  d 24  (64, 375) / (62, 197)   d 128  (64, 290) / (60, 157)   d 200  (63, 242) / (56, 129)
        ip_norm_overflow  d 24  (61, 191) / (29, 51)    d 128  (64, 171) / (23, 30)    d 200  (61, 169) / (21, 31)
        integers_2p62     d 24  (64, 407) / (61, 219)   d 128  (62, 270) / (58, 137)   d 200  (64, 237) / (54, 114)
    Under L2 every candidate is lost (xn = yn = +inf: the right side is +inf, the left -inf or NaN); under the inner product every
    row of the query's own group (the chain is at -inf after d / 2 steps).
No query and no row is excluded anywhere: the GPU test compares every row of every call."""
import numpy as np
import pytest

import extreme_range_cases as X

CASES = [(name, d) for name in X.WORLDS for d in X.DS]


@pytest.fixture(autouse=True)
def quiet(oracle):
    with np.errstate(all="ignore"):
        yield


@pytest.mark.parametrize("name,d", CASES)
def test_shapes(name, d):
    w = X.world(name, d)
    assert w["cen"].shape == (16, d) and w["xq"].shape == (64, d) and w["xb"].shape == (X.NB, d) and 2900 <= X.NB <= 3100
    assert np.bincount(w["assign"], minlength=16).min() > 65
    assert all(a.dtype == np.float32 for a in (w["cen"], w["xq"], w["xb"]))


@pytest.mark.parametrize("name,d", [(n, d) for n in X.SPREAD_WORLDS for d in X.DS])
def test_neighbours_lie_in_several_probed_lists(name, d):
    assert (X.spread(name, d) >= 3).sum() >= X.NQ // 2


@pytest.mark.parametrize("name", ["l2_norm_overflow", "integers_2p62"])
@pytest.mark.parametrize("d", X.DS)
def test_l2_norms_overflow_and_neighbours_are_finite(name, d):
    w = X.world(name, d)
    assert np.isposinf(X.norms(X.L2, w["xq"])).all() and np.isposinf(X.norms(X.L2, w["xb"])).all()
    assert d * 2.0 ** 124 > X.FMAX
    D, I, _ = X.expected(name, d)
    assert (I >= 0).all() and np.isfinite(D).all()
    # between the pairs of groups the reference's distance is +inf: never admitted, though probed where fewer than 8 lists are near
    far = X.expected_exact(name, d)[0]
    assert np.isfinite(far).all()
    from oracle import pyoracle
    cd, _ = pyoracle.knn(X.L2, w["xq"][:4], w["cen"], 16)
    assert np.isfinite(cd[:, :8]).all() and (cd[:, 8:] == X.FMAX).all()  # (the heap's initial value: an infinity never enters)
    # every value is an integer that no int holds
    for a in (w["xb"], w["xq"], w["cen"]):
        assert (a == np.trunc(a)).all() and (np.abs(a) > 2.0 ** 61).all()


@pytest.mark.parametrize("d", X.DS)
def test_ip_products_overflow_where_the_reference_is_finite(d):
    w = X.world("ip_norm_overflow", d)
    D, I, _ = X.expected("ip_norm_overflow", d)
    assert (I >= 0).all() and not np.isnan(D).any() and not np.isneginf(D).any()
    plus = {r for r, kind in w["planted"].items() if kind == "+inf"}
    minus = {r for r, kind in w["planted"].items() if kind == "-inf"}
    assert not np.isin(I, list(minus)).any()
    assert np.isin(I, list(plus)).any() and np.isposinf(D[np.isin(I, list(plus))]).all()
    assert (np.isfinite(D[:, X.K - 1])).sum() >= 60
    # a query and the finite entries of its result: |x| |y| is beyond FLT_MAX, and the filter's chain is at -inf or NaN
    xn, yn = X.norms(X.IP, w["xq"]).astype(np.float64), X.norms(X.IP, w["xb"]).astype(np.float64)
    chain = X.chain_product(w["xq"], w["xb"])
    fin = np.isfinite(D)
    q = np.nonzero(fin)[0]
    assert (xn[q] * yn[I[fin]] > X.FMAX).mean() > 0.9
    assert (~np.isfinite(chain[q, I[fin]])).mean() > 0.9


@pytest.mark.parametrize("d", X.DS)
def test_subnormal_distances(d):
    D, I, _ = X.expected("subnormal", d)
    assert (I >= 0).all()
    sub = (D != 0) & (D < X.TINY)
    assert sub.mean() >= 1 / 3 and (D == 0).sum() >= 8
    if d > 24:
        assert (D >= X.TINY).mean() > 0.2 and D.max() < 4 * X.TINY
    w = X.world("subnormal", d)
    n = w["xb"].astype(np.float64) * 2.0 ** 76
    assert (n == np.rint(n)).all() and np.abs(n).max() <= 1024


@pytest.mark.parametrize("name", ["nonfinite_l2", "nonfinite_ip"])
@pytest.mark.parametrize("d", X.DS)
def test_nonfinite_rows_and_queries(name, d):
    w = X.world(name, d)
    # six planted rows in every list, at the block and mask-word edges, every kind at every position somewhere
    seen = set()
    for l in range(X.NLIST):
        rows = np.nonzero(w["assign"] == l)[0]
        for j, pos in enumerate(X.POSITIONS):
            kind = w["planted"][int(rows[pos])]
            seen.add((kind, pos))
            row = w["xb"][rows[pos]]
            assert {"nan": np.isnan(row).sum() == 1, "+inf": np.isposinf(row).sum() == 1, "-inf": np.isneginf(row).sum() == 1,
                    "overflow": np.isfinite(row).all() and np.abs(row).max() > 2e38}[kind]
    assert len(seen) == 24 and len(w["planted"]) == 6 * X.NLIST
    assert np.isfinite(np.delete(w["xb"], sorted(w["planted"]), axis=0)).all()
    assert np.isnan(w["xq"][X.Q_NAN]).sum() == 1 and np.isposinf(w["xq"][X.Q_INF]).sum() == 1 and not w["xq"][X.Q_ZERO].any()
    assert np.isfinite(w["xq"][w["clean"]]).all() and len(w["clean"]) == 61
    D, I, _ = X.expected(name, d)
    hit = np.isin(I, sorted(w["planted"]))
    assert not np.isnan(D).any() and not np.isneginf(D).any()
    if w["metric"] == X.L2:
        assert not hit.any() and np.isfinite(D).all()
    else:
        zero_q = np.zeros(D.shape, bool)
        zero_q[X.Q_ZERO] = True
        assert (np.isposinf(D[hit]) | zero_q[hit]).all()
        assert hit[w["clean"]].any() and not np.isposinf(D[w["clean"]][~hit[w["clean"]]]).any()
        assert (np.isposinf(D[w["clean"]]).sum(axis=1) < X.K).all()  # (finite neighbours are left in every clean result)
    assert (I[w["clean"]] >= 0).all()
    cD, cI, _ = X.expected(name, d, queries="clean")
    assert np.array_equal(cI, I[w["clean"]]) and np.array_equal(X.bits(cD), X.bits(D[w["clean"]]))


@pytest.mark.parametrize("name", ["l2_norm_overflow", "ip_norm_overflow", "integers_2p62"])
@pytest.mark.parametrize("d", X.DS)
def test_the_keep_rule_as_it_stood_loses_neighbours(name, d, capsys):
    one, two = X.lost_by_model(name, d, 1), X.lost_by_model(name, d, 2)
    with capsys.disabled():
        print(f"\n    {name:18s} d {d:<4d} lost (queries, entries) after one dense probe {one}, after two {two}")
    assert one[0] >= 16 and two[0] >= 16


@pytest.mark.parametrize("name,d", CASES)
def test_exact_radius_separates_the_fifth_from_the_sixth(name, d):
    w = X.world(name, d)
    r = X.exact_radius(name, d)
    D = X.expected_exact(name, d)[0][w["clean"]]
    inside = ((D < r) if w["metric"] == X.L2 else (D > r)) & np.isfinite(D)
    # (the inner product over every list of the planted rows: ten or more +inf lead every result, the finite ones lie behind them)
    assert np.isfinite(r) and ((inside.sum(axis=1) == 5).any() or name == "nonfinite_ip")
