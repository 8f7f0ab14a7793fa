"""What test_gpu_adaptive_selected.py requires of its data (adaptive_selected_cases.py), asserted from the oracle over the filtered lists
alone.  These are conditions on the data: a world that misses one gets another seed."""
import numpy as np
import pytest

import adaptive_selected_cases as ac


@pytest.fixture(scope="module")
def arcos(oracle):
    return oracle.arcos_table()


def test_shapes_and_selectors():
    for name, metric in ac.WORLDS:
        w = ac.world(name, metric)
        assert (w.nlist, w.d, w.K, w.qk) == ((32, 16, 20, 10) if name == "A" else (256, 32, 20, 10))
        assert w.nlist > w.nlist // 8 + 20  # (the tuner's own condition)
        if name == "A":
            assert w.nb == 3000 and w.nq == 48 and set(np.unique(w.req)) <= {np.float32(0.8), np.float32(0.9), np.float32(0.95)}
            if metric == ac.L2:
                assert (w.sizes == 0).any() and w.sizes.max() > 2 * np.median(w.sizes)  # ragged
        else:
            assert 11000 <= w.nb <= 13000 and w.nq >= 20  # (20 queries and more: the call is one pass under the default tie regime)
            # rows stored twice under different ids
            _, inv, cnt = np.unique(w.xb, axis=0, return_inverse=True, return_counts=True)
            assert (cnt[inv] > 1).sum() >= w.nb // 2
        if metric == ac.L2:
            assert np.array_equal(w.xb, np.round(w.xb)) and w.xb.min() >= 0 and w.xb.max() <= 255  # byte codes apply
        masks = {s: ac.selector(name, metric, s)[1] for s in ac.SELECTORS}
        assert 0.08 * w.nb <= masks["range_10pct"].sum() <= 0.12 * w.nb
        assert masks["everything"].all()
        assert masks["few"].sum() < w.K
        kept_lists = np.bincount(w.assign[masks["sparse"]], minlength=w.nlist)
        assert (kept_lists == 0).sum() * 3 >= w.nlist and masks["sparse"].sum() > 10 * w.K
        # the selectors split the copies of duplicated rows
        if name == "B":
            m = masks["range_10pct"]
            _, inv = np.unique(w.xb, axis=0, return_inverse=True)
            both = np.intersect1d(inv[m], inv[~m])
            assert len(both) >= 100


def test_world_b_premises_under_the_ten_percent_selector(oracle, arcos):
    w = ac.world("B", ac.L2)
    r = ac.reference(oracle, arcos, "B", ac.L2, "range_10pct")
    p = r.my_nprobe
    print(np.bincount(p).tolist())
    assert (p > ac.ROUND0).sum() * 4 >= w.nq and (p == 1).any()
    fb = w.xb[ac.selector("B", ac.L2, "range_10pct")[1]]
    gd, _ = oracle.knn(ac.L2, w.xq, fb, w.K + 1, nthreads=8)
    assert ((gd[:, 1:] == gd[:, :-1]).any(axis=1)).sum() >= 5  # equal distances among the best Kmax + 1 members
    assert sum(ac.first_run(r.cd[q]) < p[q] for q in range(w.nq)) >= 5  # a run of equal coarse distances inside the probes read


def test_world_b_inner_product_premises(oracle, arcos):
    """the inner-product world meets them under the selector that keeps everything (under the selective ones the reference throws)"""
    w = ac.world("B", ac.IP)
    r = ac.reference(oracle, arcos, "B", ac.IP, "everything")
    p = r.my_nprobe
    assert (p > ac.ROUND0).sum() * 4 >= w.nq and (p == 1).any()
    gd, _ = oracle.knn(ac.IP, w.xq, w.xb, w.K + 1, nthreads=8)
    assert ((gd[:, 1:] == gd[:, :-1]).any(axis=1)).sum() >= 5
    assert sum(ac.first_run(r.cd[q]) < p[q] for q in range(w.nq)) >= 5
    for sel in ("range_10pct", "sparse", "few"):
        with pytest.raises(RuntimeError, match="arcos"):
            ac.reference(oracle, arcos, "B", ac.IP, sel)


@pytest.mark.parametrize("name", ["A", "B"])
def test_sparse_selector_meets_lists_that_keep_nothing(oracle, arcos, name):
    w = ac.world(name, ac.L2)
    r = ac.reference(oracle, arcos, name, ac.L2, "sparse")
    hit = [q for q in range(w.nq) if (r.kept_sizes[r.ck[q, :r.my_nprobe[q]]] == 0).any()]
    # ... of lists that hold rows: what the planner's skip saves is their scan
    full = [q for q in hit if ((r.kept_sizes[r.ck[q, :r.my_nprobe[q]]] == 0) & (w.sizes[r.ck[q, :r.my_nprobe[q]]] > 0)).any()]
    assert len(hit) >= 1 and len(full) >= 1


def test_every_l2_reference_exists_and_the_few_selector_pads(oracle, arcos):
    for name in ("A", "B"):
        for sel in ac.SELECTORS:
            r = ac.reference(oracle, arcos, name, ac.L2, sel)
            assert (r.my_nprobe >= 1).all()
        r = ac.reference(oracle, arcos, name, ac.L2, "few")
        assert (r.I[:, len(r.kept):] == -1).all() and (r.I[:, 0] >= 0).any()
