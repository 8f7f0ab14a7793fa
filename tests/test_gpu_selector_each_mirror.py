"""The vector form of IndexIVFFlat::search_selected of the host-side mirror (auncel_amd/csrc/host), run by
tests/cpp/selector_each_driver.cpp: one batch under a selector per query, IDSelectorRange and IDSelectorBatch mixed in one table,
returns row by row the (D, I) bits of the CPU oracle over the lists with that query's non-members removed -- which is what the call
that takes the selector alone returns -- and every device selector is made once, whether a table or a single-selector call asked first."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "selector_each_driver.cpp")
K, NPROBE = 10, 6


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from auncel_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("drv") / "selector_each_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", DRIVER_SRC, "-o", exe, "-L" + build.LIBDIR, "-lfaiss_amd", "-launcel_amd",
                    "-Wl,-rpath," + build.LIBDIR, "-pthread"], check=True)
    return exe


def test_selector_each_driver_builds_and_links(driver):
    """CPU-side: the vector overload compiles and links"""
    assert os.path.exists(driver)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [1, 0])
def test_vector_form_equals_the_oracle_and_the_single_selector_calls(driver, oracle, tmp_path, metric):
    from oracle import tbundle
    rs = np.random.RandomState(16)
    nlist, d, nb, nq = 16, 40, 2500, 64
    cen = rs.randn(nlist, d).astype(np.float32)
    xb = (cen[rs.randint(0, nlist, size=nb)] + 0.3 * rs.randn(nb, d)).astype(np.float32)
    xq = (cen[rs.randint(0, nlist, size=nq)] + 0.3 * rs.randn(nq, d)).astype(np.float32)
    batch = np.concatenate([rs.choice(nb, 300, replace=False), [nb + 9, nb + 10]]).astype(np.int64)
    lo, hi, lo2, hi2 = nb // 3, nb, 100, nb // 2
    sel_of = rs.randint(0, 4, size=nq).astype(np.int64)  # table: range, batch, range2, range again
    assert len(set(sel_of.tolist())) == 4
    t = {"d": d, "nlist": nlist, "nprobe": NPROBE, "k": K, "metric": metric, "centroids": cen, "xb": xb, "xq": xq, "range_lo": np.int64(lo),
         "range_hi": np.int64(hi), "range2_lo": np.int64(lo2), "range2_hi": np.int64(hi2), "batch": batch, "sel_of": sel_of}
    fin, fout = str(tmp_path / "in.tb"), str(tmp_path / "out.tb")
    tbundle.save(fin, t)
    r = subprocess.run([driver, fin, fout], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    out = tbundle.load(fout)
    cd, ck = oracle.knn(metric, xq, cen, NPROBE)
    assign = out["assign"].astype(np.int64)
    ids = np.arange(nb)

    def want(keep):
        m = np.nonzero(keep)[0].astype(np.int64)
        eD, eI, _ = oracle.search_preassigned(oracle.Lists(metric, cen, xb[m], assign[m], m), xq, K, ck, cd)
        return eD, eI

    per = [want((ids >= lo) & (ids < hi)), want(np.isin(ids, batch)), want((ids >= lo2) & (ids < hi2))]
    per.append(per[0])
    eD = np.stack([per[j][0][i] for i, j in enumerate(sel_of)])
    eI = np.stack([per[j][1][i] for i, j in enumerate(sel_of)])
    assert any(not np.array_equal(per[0][1][i], per[1][1][i]) for i in range(nq)) and (eI >= 0).any()
    for p in ("each_", "each2_", "each3_"):
        assert np.array_equal(out[p + "I"], eI) and np.array_equal(bits(out[p + "D"]), bits(eD)), p
    for p, j in (("range_", 0), ("batch_", 1), ("range2_", 2)):
        assert np.array_equal(out[p + "I"], per[j][1]) and np.array_equal(bits(out[p + "D"]), bits(per[j][0])), p
    # range alone: a pass; the table: the batch and the second range (the first range is kept, its twin shares it); then none
    assert [int(v) for v in out["passes"]] == [1, 3, 3, 3, 3, 3]
    assert int(out["throws_sel_of"][0]) == 1
