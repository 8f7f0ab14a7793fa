"""IndexIVFFlat::search_selected of the host-side mirror (auncel_amd/csrc/host), run by tests/cpp/selector_driver.cpp: the plain search
under an IDSelectorRange and an IDSelectorBatch returns the (D, I) bits of the CPU oracle over the lists with the non-members removed;
the selector's bits are kept while the lists and the selector's parameters repeat, and made again after an add."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "selector_driver.cpp")
K, NPROBE = 10, 6


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from auncel_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("drv") / "selector_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", DRIVER_SRC, "-o", exe, "-L" + build.LIBDIR, "-lfaiss_amd", "-launcel_amd",
                    "-Wl,-rpath," + build.LIBDIR, "-pthread"], check=True)
    return exe


def test_selector_driver_builds_and_links(driver):
    """CPU-side: the mirror overload compiles and links"""
    assert os.path.exists(driver)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [1, 0])
def test_search_selected_equals_the_oracle_over_the_filtered_lists(driver, oracle, tmp_path, metric):
    from oracle import tbundle
    rs = np.random.RandomState(6)
    nlist, d, nb, nb2, nq = 16, 40, 2500, 60, 64
    cen = rs.randn(nlist, d).astype(np.float32)
    xb = (cen[rs.randint(0, nlist, size=nb)] + 0.3 * rs.randn(nb, d)).astype(np.float32)
    xq = (cen[rs.randint(0, nlist, size=nq)] + 0.3 * rs.randn(nq, d)).astype(np.float32)
    xb2 = (xq[:nb2] + 0.01 * rs.randn(nb2, d)).astype(np.float32)  # (rows the queries find)
    batch = np.concatenate([rs.choice(nb, 300, replace=False), [nb + 9, nb + 10]]).astype(np.int64)
    lo, hi = nb // 3, nb + nb2
    t = {"d": d, "nlist": nlist, "nprobe": NPROBE, "k": K, "metric": metric, "centroids": cen, "xb": xb, "xb2": xb2, "xq": xq,
         "range_lo": np.int64(lo), "range_hi": np.int64(hi), "batch": batch}
    fin, fout = str(tmp_path / "in.tb"), str(tmp_path / "out.tb")
    tbundle.save(fin, t)
    r = subprocess.run([driver, fin, fout], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    out = tbundle.load(fout)
    cd, ck = oracle.knn(metric, xq, cen, NPROBE)

    def want(x, assign, keep):
        ids = np.nonzero(keep)[0].astype(np.int64)
        eD, eI, _ = oracle.search_preassigned(oracle.Lists(metric, cen, x[ids], assign[ids], ids), xq, K, ck, cd)
        return eD, eI

    assign = out["assign"].astype(np.int64)
    ids = np.arange(nb)
    eD, eI = want(xb, assign, (ids >= lo) & (ids < hi))
    for p in ("range_", "range2_", "range3_", "range4_"):
        assert np.array_equal(out[p + "I"], eI) and np.array_equal(bits(out[p + "D"]), bits(eD)), p
        assert [int(v) for v in out[p + "info"][:2]] == [nb, nb - lo], p
    bD, bI = want(xb, assign, np.isin(ids, batch))
    for p in ("batch_", "batch2_"):
        assert np.array_equal(out[p + "I"], bI) and np.array_equal(bits(out[p + "D"]), bits(bD)), p
        assert [int(v) for v in out[p + "info"][:2]] == [nb, 300], p
    assert (eI >= 0).any() and (bI >= 0).any()
    # a pass for new parameters or new lists, none for a repeat
    assert [int(v) for v in out["passes"]] == [1, 1, 2, 2, 3, 3, 4]
    assign2 = out["assign_added"].astype(np.int64)
    ids2 = np.arange(nb + nb2)
    aD, aI = want(np.vstack([xb, xb2]), assign2, (ids2 >= lo) & (ids2 < hi))
    assert np.array_equal(out["added_I"], aI) and np.array_equal(bits(out["added_D"]), bits(aD))
    assert (aI >= nb).any(), "no added row among the results"
    assert [int(v) for v in out["added_info"][:2]] == [nb + nb2, nb + nb2 - lo]
    assert int(out["throws_selector"][0]) == 1
