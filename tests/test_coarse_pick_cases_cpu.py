"""What the GPU tests of the matrix-core coarse ranking (test_gpu_coarse_pick_edges.py) require of their data, asserted from the numpy
model alone (coarse_pick_cases.py): the data of the bound cases sits where a too-small error constant loses true neighbours and the
kernel's own does not, and the data of the cap cases fills the candidate buffer as far as each case says.  The share of rankings the
picked path must answer is the reference's (the oracle, on the CPU)."""
import numpy as np
import pytest

import coarse_pick_cases as cp


@pytest.mark.parametrize("metric,d,nlist,nprobe,W", cp.BOUND_CASES)
def test_bound_cases_sit_at_the_edge_of_the_bound(oracle, metric, d, nlist, nprobe, W):
    cen, xq, _ = cp.coherent(d, nlist, cp.BOUND_N, W)
    assert cp.half_scale(xq) == cp.half_scale(cen) == 2.0 ** 14
    r = cp.bound_report(metric, xq, cen, nprobe)
    print(r)
    n = r["n"]
    # a true top-nprobe member outside the threshold widened with the fp32 form's constant, and outside the unwidened one: 10 % at least
    assert r["lost_fp32"] >= 0.1 * n and r["lost_unwidened"] >= 0.1 * n
    assert r["lost"] == 0       # none with exact_float_constant(d, false)
    assert r["most"] <= cp.PICK_CAP
    assert 0.45 < r["err_over_eps"] < 0.55  # the rounding is coherent: half of eps (random data: a few per cent of it)
    a, _ = cp.distinct_counts(oracle.knn(metric, xq, cen, nprobe + 1)[0])
    assert a >= n // 2          # the kernel, not the fallback, answers


def test_bound_cases_survive_the_other_end_of_the_scale_range():
    """the same data with the centroids multiplied by 2^-20 and the queries by 2^18: both scales are usable, at the far ends of what
    half_scale_of accepts, and the rounding pattern is the same (powers of two)"""
    cen, xq, _ = cp.coherent(64, 1024, cp.BOUND_N, 128)
    c2, x2 = cen * np.float32(2.0 ** -20), xq * np.float32(2.0 ** 18)
    assert cp.half_scale(c2) == 2.0 ** 34 and cp.half_scale(x2) == 2.0 ** -4
    assert np.array_equal(cp.approx_distances(0, x2, c2), cp.approx_distances(0, xq, cen) * 0.25)


def test_cap_cases_fill_the_candidate_buffer():
    nlist, nprobe, n = cp.CAP_OVER
    cen, xq, _ = cp.coherent(cp.CAP_D, nlist, n, cp.CAP_W)
    r = cp.bound_report(1, xq, cen, nprobe)
    print(r)
    assert n % 8 != 0 and r["fewest_at_first_stop"] >= 2 * cp.PICK_CAP  # (counted at the tightest threshold the kernel may stop at)
    assert cp.fewest_candidates_fp32_form(1, xq, cen, nprobe) >= 2 * cp.PICK_CAP  # (the fp32 form's smaller eps overflows it too)
    nlist, nprobe, n = cp.CAP_AT
    cen, xq, _ = cp.coherent(cp.CAP_D, nlist, n, cp.CAP_W)
    r = cp.bound_report(1, xq, cen, nprobe)
    print(r)
    assert nlist == cp.PICK_CAP and r["fewest_at_first_stop"] == r["most"] == cp.PICK_CAP and r["lost"] == 0


def test_model_constants():
    assert cp.fp32_constant(30) == cp.fp32_constant(32) == 96 * 2.0 ** -24
    assert cp.half_constant(64, True) == 160 * 2.0 ** -24
    assert cp.half_constant(64, False) == 160 * 2.0 ** -24 + 2.0 ** -10 + 2.0 ** -12
    byte_rows = np.arange(512, dtype=np.float32).reshape(8, 64) % 256
    assert cp.half_scale(byte_rows) == 1.0 and cp.half_scale(byte_rows + 0.5) == 2.0 ** 7
    assert cp.half_scale(byte_rows * np.float32(2.0 ** 40)) == 0.0
    tiny_row = byte_rows + 0.5
    tiny_row[3] *= 2.0 ** -14
    assert cp.half_scale(tiny_row) == 0.0
