"""Stored vectors back through the host-side mirror (auncel_amd/csrc/host), run by tests/cpp/reconstruct_driver.cpp: an
IndexIVFFlatSubset -- cut on the device, no host rows -- answers make_direct_map + reconstruct, reconstruct_n and
search_and_reconstruct with the bits of a host IndexIVFFlat that copy_subset_to fills and whose calls walk the host invlists as the
reference's do; a subset whose ids are not 0 .. ntotal - 1 is refused a direct map with the reference's message, and reconstruct_n
outside [0, ntotal] throws as the reference's does."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "reconstruct_driver.cpp")
K, NPROBE = 10, 6


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from auncel_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("drv") / "reconstruct_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", DRIVER_SRC, "-o", exe, "-L" + build.LIBDIR, "-lfaiss_amd", "-launcel_amd",
                    "-Wl,-rpath," + build.LIBDIR, "-pthread"], check=True)
    return exe


def test_reconstruct_driver_builds_and_links(driver):
    """CPU-side: the new mirror methods compile and link"""
    assert os.path.exists(driver)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("metric,d", [(1, 40), (0, 30)])
def test_subset_reconstructs_as_the_host_index(driver, tmp_path, metric, d):
    from oracle import tbundle
    rs = np.random.RandomState(6)
    nlist, nb, nq = 16, 2500, 64
    m = nb  # the slice [0, ntotal) of copy_subset_to's type 2: every entry, so the ids are 0 .. m - 1 whatever list they fell into
    cen = rs.randn(nlist, d).astype(np.float32)
    xb = (cen[rs.randint(0, nlist, size=nb)] + 0.3 * rs.randn(nb, d)).astype(np.float32)
    xq = (cen[rs.randint(0, nlist, size=nq)] + 0.3 * rs.randn(nq, d)).astype(np.float32)
    keys = np.concatenate([rs.permutation(m)[:100], [0, m - 1, 5, 5]]).astype(np.int64)
    i0, ni = 10, 300
    t = {"d": d, "nlist": nlist, "nprobe": NPROBE, "k": K, "metric": metric, "centroids": cen, "xb": xb, "xq": xq, "keys": keys,
         "slice": np.int64(m), "i0": np.int64(i0), "ni": np.int64(ni)}
    fin, fout = str(tmp_path / "in.tb"), str(tmp_path / "out.tb")
    tbundle.save(fin, t)
    r = subprocess.run([driver, fin, fout], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    out = tbundle.load(fout)
    assert int(out["dev_ntotal"][0]) == int(out["host_ntotal"][0]) == m
    assert [int(v) for v in out["dev_info"]] == [1, m, 0, 1]
    # the rows are the database rows themselves, and the host index's
    assert np.array_equal(bits(out["dev_rec"]), bits(xb[keys])) and np.array_equal(bits(out["host_rec"]), bits(xb[keys]))
    assert np.array_equal(bits(out["dev_recn"]), bits(xb[i0:i0 + ni])) and np.array_equal(bits(out["host_recn"]), bits(xb[i0:i0 + ni]))
    assert np.array_equal(out["dev_I"], out["host_I"]) and np.array_equal(bits(out["dev_D"]), bits(out["host_D"]))
    assert np.array_equal(bits(out["dev_R"]), bits(out["host_R"]))
    I, R = out["dev_I"], out["dev_R"]
    assert (I >= 0).any() and np.array_equal(bits(R[I >= 0]), bits(xb[I[I >= 0]])) and np.all(bits(R[I < 0]) == 0xffffffff)
    for w in ("throws_nomap", "throws_rn_past", "throws_rn_negative", "throws_rn_host_past", "ok_rn_empty", "ok_rn_whole", "throws_key",
              "throws_nonsequential", "throws_nonsequential_reconstruct"):
        assert int(out[w][0]) == 1, w
