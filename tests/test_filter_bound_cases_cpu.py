"""What the GPU tests of the list-side error bound (test_gpu_filter_bound.py) require of their data, asserted from the numpy model
alone (filter_bound_cases.py): with the kernels' own constant no true neighbour is dropped and the candidates stay far below the
exact pass's slots; with the fp32 form's constant behind the same keep rule at least half of the queries lose a neighbour at the tight
seed (and leave the pass), at least an eighth get a wrong result at the mid seed, and at least an eighth certainly lose one in the
filter's later rounds.  The floors are conditions on the data, not tolerances: a case that misses one gets another assignment or
depth (filter_bound_cases.py says which were tried), never a lower floor.  The seed's ranking is the model's and, once more, the
reference's own (the oracle, on the CPU)."""
import numpy as np
import pytest

import coarse_pick_cases as cp
import filter_bound_cases as fb

HALF, EIGHTH = fb.N // 2, fb.N // 8


def constants(d):
    return cp.half_constant(d, False), cp.fp32_constant(d)


def check_scales(c):
    """every operand has a usable scale and none is held exactly: the 2^-10 term is in force"""
    for m in (c.xq, c.xb):
        assert cp.half_scale(m) == 2.0 ** 14 and not cp.held_exactly(m)


def check_exact(c, deep, mid, rank=None):
    C, F = constants(c.d)
    for s in (deep, mid):
        r = fb.report(c, s, C, rank)
        print("real constant", s, r)
        assert r["lost"] == 0 and r["most"] <= fb.CAP // 4
    deep_r, mid_r = fb.report(c, deep, F, rank), fb.report(c, mid, F, rank)
    print("fp32 constant", deep, deep_r, mid, mid_r)
    assert deep_r["lost"] >= HALF
    assert mid_r["wrong"] >= EIGHTH


@pytest.mark.parametrize("metric,d,W,mid,seed", fb.EXACT_CASES)
def test_exact_cases_sit_at_the_edge_of_the_bound(oracle, metric, d, W, mid, seed):
    c = fb.case(metric, d, W, seed=seed)
    check_scales(c)
    assert np.bincount(c.assign, minlength=fb.NLIST).min() > 0
    check_exact(c, fb.TIGHT, mid)
    check_exact(c, fb.TIGHT, mid, rank=oracle.knn(metric, c.xq, c.cen, fb.NLIST)[1])
    assert 0.5 < fb.err_over_bound(c) < 0.8  # (random data: a few per cent)


@pytest.mark.parametrize("metric,d,W,seed", fb.SELECTED_CASES)
def test_selected_cases_sit_at_the_edge_of_the_bound(oracle, metric, d, W, seed):
    c = fb.every_second(fb.case(metric, d, W, seed=seed))
    assert len(c.xb) == fb.NB // 2
    check_scales(c)
    deep, mid = (fb.selected_depth(o) for o in fb.SELECTED_OPTION)
    assert mid < deep < fb.NLIST  # (a seed of every list is the whole search: the call would go the general way)
    check_exact(c, deep, mid)
    check_exact(c, deep, mid, rank=oracle.knn(metric, c.xq, c.cen, fb.NLIST)[1])


@pytest.mark.parametrize("metric", [fb.L2, fb.IP])
@pytest.mark.parametrize("d", fb.FILTER_D)
def test_dense_first_cases_lose_neighbours_in_later_rounds(metric, d):
    assert set(fb.NARROW_D) <= set(fb.FILTER_D)
    c = fb.case(metric, d, fb.spread(metric), "dense")
    check_scales(c)
    sizes = np.bincount(c.assign, minlength=fb.NLIST)
    assert abs(sizes[0] - fb.DENSE * fb.NB) < 0.02 * fb.NB and sizes[1:].min() > 0
    C, F = constants(d)
    real, fp32 = fb.dense_first_report(c, C), fb.dense_first_report(c, F)
    print(real, fp32)
    assert real["lost"] == 0
    assert fp32["lost"] >= EIGHTH


def test_the_selected_dense_first_case():
    metric, d = fb.FILTER_SELECTED
    c = fb.every_second(fb.case(metric, d, fb.spread(metric), "dense"))
    check_scales(c)
    C, F = constants(d)
    assert fb.dense_first_report(c, C)["lost"] == 0
    assert fb.dense_first_report(c, F)["lost"] >= EIGHTH


def test_the_data_cannot_see_the_smallest_term():
    """said in filter_bound_cases.py: without the 2^-12 term nothing is lost; with half the constant 41 .. 256 queries are"""
    for metric, d, W, mid, seed in fb.EXACT_CASES:
        c = fb.case(metric, d, W, seed=seed)
        C = cp.half_constant(d, False)
        assert fb.report(c, fb.TIGHT, C - 2.0 ** -12)["lost"] == 0
        assert fb.report(c, fb.TIGHT, C / 2)["lost"] >= 32


def test_model_keep_rule():
    """the two sides of the rule on numbers worked by hand: L2 2 p - (1 - C) yn >= (1 - C) xn - tau, IP p + C xn yn >= tau"""
    one = np.ones(1, np.float32)
    p = np.array([[1.0]], np.float32)
    # L2, C = 0: |x|^2 = |y|^2 = 2, x.y = 1 -> distance 2: kept at tau = 2 (non-strict), dropped just below
    assert fb.keep(fb.L2, 0.0, p, 2 * one, 2 * one, 2 * one).all()
    assert not fb.keep(fb.L2, 0.0, p, 2 * one, 2 * one, np.nextafter(2 * one, one)).any()
    # ... C = 2^-10 widens it by C (xn + yn) = 2^-8
    assert fb.keep(fb.L2, 2.0 ** -10, p, 2 * one, 2 * one, (2 - 2.0 ** -8) * one).all()
    assert not fb.keep(fb.L2, 2.0 ** -10, p, 2 * one, 2 * one, (2 - 2.0 ** -7) * one).any()
    # IP: p = 1, |x| = |y| = 2
    assert fb.keep(fb.IP, 0.0, p, 2 * one, 2 * one, one).all()
    assert not fb.keep(fb.IP, 0.0, p, 2 * one, 2 * one, np.nextafter(one, 2 * one)).any()
    assert fb.keep(fb.IP, 2.0 ** -10, p, 2 * one, 2 * one, (1 + 2.0 ** -8) * one).all()
    assert not fb.keep(fb.IP, 2.0 ** -10, p, 2 * one, 2 * one, (1 + 2.0 ** -7) * one).any()
    assert fb.within(fb.L2, np.array([[1.0, 2.0, 3.0]]), np.array([2.0])).tolist() == [[True, True, False]]
    assert fb.within(fb.IP, np.array([[1.0, 2.0, 3.0]]), np.array([2.0])).tolist() == [[False, True, True]]
