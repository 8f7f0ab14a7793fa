"""The joins of the host-side mirror (auncel_amd/csrc/host), run by tests/cpp/concat_driver.cpp: IndexIVFFlatSubset's constructor
from parts and ivflib::SlidingIndexWindowDevice.  After every one of five window steps -- the three branches of the reference's
SlidingIndexWindow::step -- the device window and an index joined from the window's slices return the (D, I) bits of an IndexIVFFlat
that the driver fills on the host with the same lists; the exceptions and the compatibility refusal are the reference's."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "concat_driver.cpp")
K, NPROBE, NSLICE = 10, 6, 4
HELD = [[0], [0, 1], [1, 2], [2], [3]]  # the slices in the window after every step of the driver's script


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from auncel_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("drv") / "concat_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", DRIVER_SRC, "-o", exe, "-L" + build.LIBDIR, "-lfaiss_amd", "-launcel_amd",
                    "-Wl,-rpath," + build.LIBDIR, "-pthread"], check=True)
    return exe


def test_concat_driver_builds_and_links(driver):
    """CPU-side: the parts constructor and IVFlib.h compile and link"""
    assert os.path.exists(driver)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [1, 0])
def test_window_and_parts_equal_the_host_lists(driver, tmp_path, metric):
    from oracle import tbundle
    rs = np.random.RandomState(6)
    nlist, d, nb, nq = 16, 40, 2500, 64
    cen = rs.randn(nlist, d).astype(np.float32)
    xb = (cen[rs.randint(0, nlist, size=nb)] + 0.3 * rs.randn(nb, d)).astype(np.float32)
    xq = (cen[rs.randint(0, nlist, size=nq)] + 0.3 * rs.randn(nq, d)).astype(np.float32)
    slice_of = rs.randint(0, NSLICE, size=nb).astype(np.int64)
    t = {"d": d, "nlist": nlist, "nprobe": NPROBE, "k": K, "metric": metric, "centroids": cen, "xb": xb, "xq": xq,
         "slice_of": slice_of, "nslice": NSLICE}
    fin, fout = str(tmp_path / "in.tb"), str(tmp_path / "out.tb")
    tbundle.save(fin, t)
    r = subprocess.run([driver, fin, fout], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    out = tbundle.load(fout)
    for w in ("none", "nothing", "nlist", "d", "type", "add"):
        assert int(out["throws_" + w][0]) == 1, w
    assert int(out["refused_ntotal"][0]) == 0 and int(out["refused_n_slice"][0]) == 0
    count = np.bincount(slice_of, minlength=NSLICE)
    for step, held in enumerate(HELD):
        p = "step%d_" % step
        want = int(count[held].sum())
        assert int(out[p + "n_slice"][0]) == len(held), step
        assert int(out[p + "sizes_ok"][0]) == 1, step
        for who in ("win_", "parts_"):
            assert int(out[p + who + "ntotal"][0]) == int(out[p + "host_ntotal"][0]) == want, (step, who)
            assert np.array_equal(out[p + who + "I"], out[p + "host_I"]), (step, who)
            assert np.array_equal(bits(out[p + who + "D"]), bits(out[p + "host_D"])), (step, who)
        assert (out[p + "host_I"] >= 0).any()
    for p in ("shift_", "runs_"):
        assert int(out[p + "dev_ntotal"][0]) == int(out[p + "host_ntotal"][0]) > 0, p
        assert np.array_equal(out[p + "dev_I"], out[p + "host_I"]), p
        assert np.array_equal(bits(out[p + "dev_D"]), bits(out[p + "host_D"])), p
    assert (out["shift_host_I"] >= 100000).any() and int(out["shift_host_ntotal"][0]) == int(count[[0, 1]].sum())
    taken, nparts, h2d, d2h = (int(v) for v in out["runs_last_concat"])
    assert taken == int(out["runs_host_ntotal"][0]) and nparts == 2
    assert h2d <= (2 * nparts + 2) * 8 * (nlist + 1) + 65536 and d2h <= 65536
    # the slices were destroyed before this search: the window borrows nothing
    assert np.array_equal(out["after_win_I"], out["step4_host_I"]) and np.array_equal(bits(out["after_win_D"]), bits(out["step4_host_D"]))
