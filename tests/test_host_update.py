"""In-place changes through the host-side mirror (auncel_amd/csrc/host): IndexIVFFlat::update_vectors and IndexIVF::merge_from, run
by tests/cpp/update_driver.cpp, against Python restatements of the reference (IndexIVFFlat.cpp:190-224, InvertedLists.cpp:77-97)
and the CPU oracle; the engine takes the changed lists through the journal (amd_ivf_update_lists) rather than whole."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "update_driver.cpp")
K, NPROBE = 10, 6


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from auncel_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("drv") / "update_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", DRIVER_SRC, "-o", exe, "-L" + build.LIBDIR, "-lfaiss_amd", "-launcel_amd",
                    "-Wl,-rpath," + build.LIBDIR, "-pthread"], check=True)
    return exe


def test_update_driver_builds_and_links(driver):
    """CPU-side: the new mirror methods compile and link"""
    assert os.path.exists(driver)


def _run(driver, kind, tensors, tmp_path):
    from oracle import tbundle
    fin, fout = str(tmp_path / "in.tb"), str(tmp_path / "out.tb")
    tbundle.save(fin, tensors)
    r = subprocess.run([driver, kind, fin, fout], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    return tbundle.load(fout)


def _case(metric, seed=4, nlist=16, d=40, nb=2500, nq=64):
    rs = np.random.RandomState(seed)
    cen = rs.randn(nlist, d).astype(np.float32)
    xb = (cen[rs.randint(0, nlist, size=nb)] + 0.3 * rs.randn(nb, d)).astype(np.float32)
    xq = (cen[rs.randint(0, nlist, size=nq)] + 0.3 * rs.randn(nq, d)).astype(np.float32)
    return rs, {"d": d, "nlist": nlist, "nprobe": NPROBE, "k": K, "metric": metric, "centroids": cen, "xb": xb, "xq": xq}


def _lists(out, p, nlist):
    off = out[p + "off"]
    return ([out[p + "codes"][off[l]:off[l + 1]] for l in range(nlist)], [out[p + "ids"][off[l]:off[l + 1]] for l in range(nlist)])


def _oracle_search(oracle, t, codes, ids):
    nlist = t["nlist"]
    xb = np.vstack(codes).astype(np.float32)
    assign = np.concatenate([np.full(len(ids[l]), l, np.int64) for l in range(nlist)])
    lists = oracle.Lists(t["metric"], t["centroids"], xb, assign, np.concatenate(ids))
    cd, ck = oracle.knn(t["metric"], t["xq"], t["centroids"], NPROBE)
    D, I, _ = oracle.search_preassigned(lists, t["xq"], K, ck, cd)
    return D, I


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [1, 0])
def test_update_vectors(driver, oracle, tmp_path, metric):
    rs, t = _case(metric)
    nb, nlist = len(t["xb"]), t["nlist"]
    upd = rs.choice(nb, 150, replace=False).astype(np.int64)
    upd[:3] = [upd[3], upd[3], upd[4]]  # (an id updated twice in one call)
    t["upd_ids"] = upd
    t["upd_x"] = (t["centroids"][rs.randint(0, nlist, size=len(upd))] + 0.3 * rs.randn(len(upd), t["d"])).astype(np.float32)
    out = _run(driver, "update", t, tmp_path)
    # restatement of IndexIVFFlat::update_vectors (IndexIVFFlat.cpp:190-224) on the lists before
    codes, ids = _lists(out, "before_", nlist)
    codes, ids = [c.copy() for c in codes], [list(i) for i in ids]
    codes = [list(c) for c in codes]
    dm = out["before_direct_map"].copy()
    for i, idv in enumerate(upd):
        il, ofs = int(dm[idv]) >> 32, int(dm[idv]) & 0xffffffff
        n = len(ids[il])
        if ofs != n - 1:
            id2 = ids[il][n - 1]
            dm[id2] = (il << 32) | ofs
            ids[il][ofs], codes[il][ofs] = id2, codes[il][n - 1]
        ids[il].pop()
        codes[il].pop()
        nl = int(out["upd_assign"][i])
        dm[idv] = (nl << 32) | len(ids[nl])
        ids[nl].append(idv)
        codes[nl].append(t["upd_x"][i])
    got_c, got_i = _lists(out, "after_", nlist)
    for l in range(nlist):
        assert np.array_equal(got_i[l], np.array(ids[l], np.int64)), l
        assert np.array_equal(bits(got_c[l]), bits(np.array(codes[l], np.float32).reshape(-1, t["d"]))), l
    assert np.array_equal(out["after_direct_map"], dm)
    # the new vectors' lists are the oracle's nearest centroids
    _, a = oracle.knn(metric, t["upd_x"], t["centroids"], 1)
    assert np.array_equal(out["upd_assign"], a[:, 0])
    D, I = _oracle_search(oracle, t, got_c, got_i)
    assert np.array_equal(out["after_I"], I) and np.array_equal(bits(out["after_D"]), bits(D))
    assert out["before_last_update"][0] == 2 and out["after_last_update"][0] == 1, (out["before_last_update"], out["after_last_update"])
    assert int(out["throws_no_direct_map"][0]) == 1
    assert int(out["throws_out_of_range"][0]) == 1
    assert int(out["throws_dedup"][0]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("add_id", [0, 100000])
def test_merge_from(driver, oracle, tmp_path, add_id):
    rs, t = _case(1, seed=9)
    nlist = t["nlist"]
    t["add_id"] = add_id
    out = _run(driver, "merge", t, tmp_path)
    ac, ai = _lists(out, "a_", nlist)
    bc, bi = _lists(out, "b_", nlist)
    mc, mi = _lists(out, "merged_", nlist)
    for l in range(nlist):
        assert np.array_equal(mi[l], np.concatenate([ai[l], bi[l] + add_id])), l
        assert np.array_equal(bits(mc[l]), bits(np.vstack([ac[l], bc[l]]))), l
    assert int(out["merged_ntotal"][0]) == len(t["xb"]) and int(out["other_ntotal"][0]) == 0
    assert len(out["other_ids"]) == 0
    D, I = _oracle_search(oracle, t, mc, mi)
    assert np.array_equal(out["merged_I"], I) and np.array_equal(bits(out["merged_D"]), bits(D))
    assert out["merged_last_update"][0] in (1, 2)  # (half the entries are new: more than a quarter, the full path)
    assert int(out["throws_nlist"][0]) == 1 and int(out["throws_type"][0]) == 1
