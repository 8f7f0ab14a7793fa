"""An index built on the device from device-resident rows (amd_ivf_build_dev, ivf_build.hip).  The placement is compared with a stable
grouping in numpy, the whole index with an owner that took the same rows through amd_ivf_add (all eight digest words after the same
warm-up, searches against the pinned CPU oracle).  Every comparison is of bits or of integers."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_concat import capi, model_of  # noqa: F401 (capi: the module's fixture)
from test_gpu_subset import check_searches
from test_gpu_update import bits, make_case, warm

pytestmark = pytest.mark.gpu
T, NLIST = 1024, 40  # (the tile of the second sweep; a list count that is no multiple of 64)


def fresh(capi, cen, metric=1):
    h = capi.Handle(cen.shape[1], cen.shape[0], metric, 0)
    h.set_centroids(cen)
    return h


def quantizer(capi, d):
    return fresh(capi, np.random.RandomState(1).randn(NLIST, d).astype(np.float32))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def keys_of(pattern, n):
    rs = np.random.RandomState(n + 11)
    k = {"one_list": np.full(n, 17), "round_robin": np.arange(n) % NLIST, "empty_lists": rs.choice([0, 3, 4, 5, 21, 38, 39], size=n),
         "tenth_skipped": rs.randint(0, NLIST, size=n)}[pattern].astype(np.int64)
    if pattern == "tenth_skipped":
        k[rs.rand(n) < 0.1] = -rs.randint(1, 1 << 40)
    return k


def check_lists(b, x, ids, keys):
    """get_list of every list against the stable grouping of (x, ids) by keys; the transfer report"""
    order = np.argsort(keys, kind="stable")
    order = order[keys[order] >= 0]
    assert b.ntotal == len(order)
    for l in range(NLIST):
        rows = order[keys[order] == l]
        c, i = b.get_list(l)
        assert np.array_equal(i, ids[rows]) and np.array_equal(bits(c), bits(x[rows])), l
    offered, stored, h2d, d2h = b.last_build()
    assert (offered, stored) == (len(keys), len(order)) and h2d <= 8 * (NLIST + 1) + 16 and d2h <= 16 * (NLIST + 1) + 20, b.last_build()


# n around one tile, three tiles in one chunk, three chunks of a tile, chunks of two tiles with one row above the last edge
@pytest.mark.parametrize("n,chunk", [(0, 0), (1, 0), (T - 1, 0), (T, 0), (T + 1, 0), (2 * T + 1, 0), (2 * T + 1, T), (4 * T + 1, 2 * T)])
@pytest.mark.parametrize("pattern", ["one_list", "round_robin", "empty_lists", "tenth_skipped"])
def test_placement_is_the_stable_grouping(capi, monkeypatch, pattern, n, chunk):
    if chunk:
        monkeypatch.setenv("AUNCEL_AMD_BUILD_CHUNK", str(chunk))
    d, q = 32, quantizer(capi, 32)
    x, keys = np.random.RandomState(n).randn(n, d).astype(np.float32), keys_of(pattern, n)
    b = q.build_dev(dev(x), id_base=-5, assign=dev(keys))
    check_lists(b, x, np.arange(n, dtype=np.int64) - 5, keys)
    b.close(), q.close()


@pytest.mark.parametrize("form,ldx", [("d30_gap_of_nan", 36), ("fp16", 36), ("fp16_odd_stride", 33), ("ids_given", 30)])
def test_strides_types_and_ids(capi, monkeypatch, form, ldx):
    monkeypatch.setenv("AUNCEL_AMD_BUILD_CHUNK", str(T))
    n, d, rs = 2 * T + 1, 30, np.random.RandomState(4)
    wide = np.full((n, ldx), np.nan, np.float16 if form.startswith("fp16") else np.float32)
    wide[:, :d] = rs.randn(n, d)
    keys = keys_of("tenth_skipped", n)
    ids = rs.randint(-(1 << 62), 1 << 62, size=n).astype(np.int64) if form == "ids_given" else np.arange(n, dtype=np.int64)
    q = quantizer(capi, d)
    b = q.build_dev(dev(wide)[:, :d], ids=dev(ids) if form == "ids_given" else None, assign=dev(keys))
    check_lists(b, wide[:, :d].astype(np.float32), ids, keys)
    b.close(), q.close()


def same_as_owner(oracle, metric, cen, xq, built, owner, words=8):
    """the digest words after the same warm-up (all eight); the searches of `built` against the oracle over the owner's lists"""
    warm(built, xq), warm(owner, xq)
    db, do = built.layout_digest(), owner.layout_digest()
    assert db[:words] == do[:words], [i for i in range(8) if db[i] != do[i]]
    lists = [owner.get_list(l) for l in range(owner.nlist)]
    check_searches(oracle, built, metric, cen, model_of(owner.d, [c for c, _ in lists], [i for _, i in lists]), xq)


@pytest.mark.parametrize("name", ["sift_l2", "l2_96", "ip_96", "odd_30", "bytes_200"])
def test_same_index_as_add_with_its_own_assignment(capi, oracle, name):
    metric, cen, _, xb, xq = make_case(name)
    q, owner = fresh(capi, cen, metric), fresh(capi, cen, metric)
    owner.add(xb)
    built = q.build_dev(dev(xb))
    q.close()
    same_as_owner(oracle, metric, cen, xq, built, owner)
    built.close(), owner.close()


@pytest.mark.parametrize("skipped", [True, False])
def test_byte_eligibility_is_taken_over_the_rows_stored(capi, oracle, skipped):
    """ntotal of a built index counts the rows stored; amd_ivf_add's counts a skipped row too (ntotal += n, as the reference), and
    ntotal is part of digest word 7.  So with a row skipped, the owner that was given the skip is equal in words 0..6, and the owner
    that was given the stored rows alone, under their ids, in all eight."""
    metric, cen, assign, xb, xq = make_case("sift_l2")
    xb[1500] += 0.5  # the only row that is not of integers
    assign = assign.astype(np.int64)
    if skipped:
        assign[1500] = -1
    q, owner = fresh(capi, cen, metric), fresh(capi, cen, metric)
    owner.add(xb, None, assign)
    built = q.build_dev(dev(xb), assign=dev(assign))
    same_as_owner(oracle, metric, cen, xq, built, owner, 7 if skipped else 8)
    assert (built.scan_arith() == 2) == skipped and (built.layout_digest()[3] != 0) == skipped
    if skipped:
        stored, keep = fresh(capi, cen, metric), assign >= 0
        stored.add(xb[keep], np.nonzero(keep)[0], assign[keep])
        same_as_owner(oracle, metric, cen, xq, built, stored)
        assert built.ntotal == len(xb) - 1 == stored.ntotal == owner.ntotal - 1
        stored.close()
    built.close(), owner.close(), q.close()


def test_concat_with_a_built_part_is_an_add_from_device_memory(capi, oracle):
    metric, cen, _, xb, xq = make_case("l2_96")
    owner, ref = fresh(capi, cen, metric), fresh(capi, cen, metric)
    owner.add(xb[:2000])
    part = owner.build_dev(dev(xb[2000:]), id_base=2000)
    joined = capi.Handle.concat([owner, part])
    owner.add(xb[2000:])
    same_as_owner(oracle, metric, cen, xq, joined, owner)
    ref.add(xb[2000:], np.arange(2000, len(xb)))
    owner.close()  # the built part borrows nothing from the handle that gave it its quantizer
    same_as_owner(oracle, metric, cen, xq, part, ref)
    part.close(), joined.close(), ref.close()


def test_refusals(capi):
    q, L = quantizer(capi, 32), capi.lib()
    x = np.zeros((8, 32), np.float32)
    with pytest.raises(capi.EngineError, match="-2: Invalid list number in add"):
        q.build_dev(dev(x), assign=dev(np.array([0, 1, 2, NLIST, 3, -1, 0, 0], np.int64)))
    host, out = dev(x).cpu().pin_memory(), C.c_void_p(7)
    rc = L.amd_ivf_build_dev(q._h, C.c_size_t(8), C.c_void_p(host.data_ptr()), 0, C.c_size_t(32), None, C.c_int64(0), None, 0, None, C.byref(out))
    assert rc == -2 and out.value is None and b"d_x: not a device pointer" in L.amd_ivf_last_error()
    b = q.build_dev(dev(x))
    with pytest.raises(capi.EngineError, match="-2: .*read-only"):
        b.add(x)
    b.close(), q.close()
