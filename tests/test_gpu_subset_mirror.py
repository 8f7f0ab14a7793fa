"""IndexIVFFlatSubset of the host-side mirror (auncel_amd/csrc/host), run by tests/cpp/subset_driver.cpp: an index cut on the device by
an IDSelectorRange, by an IDSelectorBatch and by copy_subset_to's type 1 returns the same (D, I) bits as an IndexIVFFlat that the
driver fills on the host with the members of every list in list order; it is read-only, and other selectors are "not implemented"."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "subset_driver.cpp")
K, NPROBE = 10, 6


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from auncel_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("drv") / "subset_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", DRIVER_SRC, "-o", exe, "-L" + build.LIBDIR, "-lfaiss_amd", "-launcel_amd",
                    "-Wl,-rpath," + build.LIBDIR, "-pthread"], check=True)
    return exe


def test_subset_driver_builds_and_links(driver):
    """CPU-side: the new mirror class compiles and links"""
    assert os.path.exists(driver)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [1, 0])
def test_subset_index_equals_the_host_subset(driver, tmp_path, metric):
    from oracle import tbundle
    rs = np.random.RandomState(6)
    nlist, d, nb, nq = 16, 40, 2500, 64
    cen = rs.randn(nlist, d).astype(np.float32)
    xb = (cen[rs.randint(0, nlist, size=nb)] + 0.3 * rs.randn(nb, d)).astype(np.float32)
    xq = (cen[rs.randint(0, nlist, size=nq)] + 0.3 * rs.randn(nq, d)).astype(np.float32)
    batch = np.concatenate([rs.choice(nb, 300, replace=False), [nb + 9, nb + 10]]).astype(np.int64)
    t = {"d": d, "nlist": nlist, "nprobe": NPROBE, "k": K, "metric": metric, "centroids": cen, "xb": xb, "xq": xq,
         "range_lo": np.int64(nb // 3), "range_hi": np.int64(2 * nb // 3), "batch": batch}
    fin, fout = str(tmp_path / "in.tb"), str(tmp_path / "out.tb")
    tbundle.save(fin, t)
    r = subprocess.run([driver, fin, fout], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    out = tbundle.load(fout)
    want_n = {"range": 2 * nb // 3 - nb // 3, "batch": 300, "mod": len(range(2, nb, 4))}
    for p in ("range", "batch", "mod"):
        assert int(out[p + "_dev_ntotal"][0]) == int(out[p + "_host_ntotal"][0]) == want_n[p], p
        assert np.array_equal(out[p + "_dev_I"], out[p + "_host_I"]), p
        assert np.array_equal(bits(out[p + "_dev_D"]), bits(out[p + "_host_D"])), p
        assert (out[p + "_dev_I"] >= 0).any()
    assert np.array_equal(out["range_after_I"], out["range_host_I"]) and np.array_equal(bits(out["range_after_D"]), bits(out["range_host_D"]))
    looked, kept, h2d, d2h = (int(v) for v in out["range_last_subset"])
    assert looked == nb and kept == want_n["range"]
    assert h2d <= 16 * (nlist + 1) + 65536 and d2h <= 16 * (nlist + 1) + 65536
    for w in ("add", "train", "reset", "selector", "type", "dedup"):
        assert int(out["throws_" + w][0]) == 1, w
