"""Stored vectors back from a device-resident index (include/auncel_amd.h: amd_ivf_make_direct_map, amd_ivf_reconstruct,
_reconstruct_n, _reconstruct_from_offsets, amd_ivf_search_and_reconstruct; ivf_reconstruct.hip).  Every comparison is
of bits: a reconstructed row is the stored row, -0.0, subnormals and NaN payloads included; where an id is stored more than once the
row is the one at the largest position; search_and_reconstruct returns search()'s (D, I) and the row of the entry that was admitted,
which is looked up in a Python model of the lists at the positions a store_pairs search returns."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_exact import byte_case, make_handle, ragged_assign
from test_gpu_update import Model, make_case

pytestmark = pytest.mark.gpu

L2, IP = 1, 0
NLIST, NB = 16, 3000
DIMS = [1, 3, 30, 128, 130, 960]  # the scalar tail alone, dpad != d, the 16-byte path, both, and a wide row


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(u32(a), u32(b))


def refused(capi, f, word, code=-2):
    with pytest.raises(capi.EngineError) as e:
        f()
    assert e.value.code == code and word in str(e.value), str(e.value)


def odd_floats(rs, n, d):
    """rows of every kind of bits a copy must not touch: -0.0, subnormals, infinities, quiet and signalling NaN payloads"""
    x = rs.randn(n, d).astype(np.float32)
    b = x.view(np.uint32)
    flat = b.reshape(-1)
    special = np.array([0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc12345, 0x7f800001, 0xffffffff, 0],
                       np.uint32)
    pos = rs.choice(flat.size, size=min(flat.size, max(10, flat.size // 7)), replace=False)
    flat[pos] = special[np.arange(len(pos)) % len(special)]
    return x


def ragged_world(capi, d, metric=L2, seed=11, nb=NB, values="odd"):
    """lists of 0, 1, 31, 32, 33, 63, 64, 65 and 70 entries among longer ones; ids 0 .. nb - 1 in database order"""
    rs = np.random.RandomState(seed + d)
    assign = ragged_assign(NLIST, nb)
    xb = odd_floats(rs, nb, d) if values == "odd" else rs.randn(nb, d).astype(np.float32)
    cen = rs.randn(NLIST, d).astype(np.float32)
    return make_handle(capi, metric, cen, xb, assign), Model(NLIST, d, xb, assign), xb, cen


def set_model(h, model):
    h.set_lists([len(i) for i in model.ids], model.codes, model.ids)


def last_rows(model):
    """id -> (row, position) of its LAST entry in list-by-list, offset-by-offset order: what the reference's loops leave"""
    out = {}
    for l in range(len(model.ids)):
        for o, i in enumerate(model.ids[l]):
            out[int(i)] = (model.codes[l][o], (l << 32) | o)
    return out


def rows_of_labels(model, labels, d):
    labels = np.asarray(labels).reshape(-1)
    rows = np.empty((len(labels), d), np.float32)
    ids = np.empty(len(labels), np.int64)
    for i, lab in enumerate(labels):
        if lab < 0:
            rows[i].view(np.uint32)[:] = 0xffffffff
            ids[i] = -1
        else:
            l, o = int(lab) >> 32, int(lab) & 0xffffffff
            rows[i], ids[i] = model.codes[l][o], model.ids[l][o]
    return rows, ids


# ------------------------------------------------------------------------------------------------ by id
@pytest.mark.parametrize("d", DIMS)
def test_reconstruct_by_id_returns_the_stored_bits(capi, d):
    nb = 1500 if d == 960 else NB
    h, model, xb, _ = ragged_world(capi, d, nb=nb)
    refused(capi, lambda: h.reconstruct([0]), "direct map is not initialized")
    h.make_direct_map()
    assert h.direct_map_info() == [1, nb, 0, 1]
    rs = np.random.RandomState(d)
    for ids in (np.arange(nb), rs.permutation(nb), rs.randint(0, nb, size=777), np.array([nb - 1]), np.array([], np.int64)):
        assert same_bits(h.reconstruct(ids), xb[ids]), (d, len(ids))
    h.make_direct_map()  # (nothing to do: no second pass)
    assert h.direct_map_info()[3] == 1
    # an id outside [0, ntotal): refused on the host, naming its position, recons untouched
    sent = np.full((3, d), 7.25, np.float32)
    for bad in (nb, -1, 2 ** 40):
        refused(capi, lambda: h.reconstruct([5, bad, 6], out=sent), "invalid key %d at position 1" % bad)
    assert np.all(sent == 7.25)
    # reconstruct_n: the whole range, found everywhere, with and without the found array
    rec, found = h.reconstruct_n(0, nb)
    assert same_bits(rec, xb) and found.all()
    rec, found = h.reconstruct_n(0, nb, want_found=False)
    assert same_bits(rec, xb) and found is None
    h.make_direct_map(False)
    assert h.direct_map_info()[:3] == [0, 0, 0]
    refused(capi, lambda: h.reconstruct([0]), "direct map is not initialized")


def duplicate_world(capi):
    """one id stored in list 2 and twice in list 5, with three different rows; the two ids it replaced in list 5 are then absent"""
    metric, cen, assign, xb, _ = make_case("odd_30")
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(NLIST, xb.shape[1], xb, assign)
    dup = int(model.ids[2][4])
    at = [(5, 3), (5, len(model.ids[5]) - 1)]
    gone = sorted(int(model.ids[l][o]) for l, o in at)
    for l, o in at:
        model.ids[l][o] = dup
    set_model(h, model)
    return h, model, dup, gone


def test_duplicate_ids_resolve_to_the_largest_position(capi):
    d = 30
    h, model, dup, gone = duplicate_world(capi)
    nb = h.ntotal
    want = last_rows(model)
    where77 = [(l, o) for l in range(NLIST) for o, i in enumerate(model.ids[l]) if i == dup]
    assert len(where77) == 3 and [l for l, _ in where77] == [2, 5, 5]
    rows77 = [model.codes[l][o] for l, o in where77]
    assert not same_bits(rows77[0], rows77[2]) and not same_bits(rows77[1], rows77[2])
    h.make_direct_map()
    info = h.direct_map_info()
    assert info[0] == 1 and info[1] == nb - len(gone) and info[2] == len(gone) == 2
    assert same_bits(h.reconstruct([dup])[0], rows77[2]) and want[dup][1] == (5 << 32) | where77[2][1]
    present = np.array(sorted(want), np.int64)
    assert same_bits(h.reconstruct(present), np.stack([want[int(i)][0] for i in present]))
    rec, found = h.reconstruct_n(0, nb, out=np.full((nb, d), -3.5, np.float32))
    for i in range(nb):
        if i in want:
            assert found[i] == 1 and same_bits(rec[i], want[i][0]), i
        else:
            assert found[i] == 0 and np.all(rec[i] == -3.5), i
    assert sorted(np.nonzero(found == 0)[0].tolist()) == gone
    # an id of [0, ntotal) without an entry: refused, naming the position, recons untouched
    sent = np.full((4, d), 9.5, np.float32)
    refused(capi, lambda: h.reconstruct([1, 2, gone[0], gone[1]], out=sent), "invalid key %d at position 2" % gone[0])
    assert np.all(sent == 9.5)
    # the labels say which entry: each of the three rows of the repeated id by its own position
    rec, ids = h.reconstruct_from_offsets([(l << 32) | o for l, o in where77])
    assert ids.tolist() == [dup] * 3 and same_bits(rec, np.stack(rows77))


@pytest.mark.parametrize("which", ["huge", "negative"])
def test_ids_outside_the_direct_maps_range(capi, which):
    d = 3
    h, model, xb, _ = ragged_world(capi, d, seed=5)
    base = 10 ** 12 if which == "huge" else -5000
    for l in range(NLIST):
        model.ids[l] = model.ids[l] + base
    set_model(h, model)
    refused(capi, h.make_direct_map, "direct map supported only for")
    assert h.direct_map_info()[0] == 0
    refused(capi, lambda: h.reconstruct([0]), "direct map is not initialized")
    rec, found = h.reconstruct_n(base, NB)
    assert same_bits(rec, xb) and found.all()
    # a window that straddles stored and unstored ids on either side; unstored slots keep their sentinel
    rec, found = h.reconstruct_n(base - 40, 100, out=np.full((100, d), 2.5, np.float32))
    assert not found[:40].any() and found[40:].all() and np.all(rec[:40] == 2.5) and same_bits(rec[40:], xb[:60])
    rec, found = h.reconstruct_n(base + NB - 10, 64, out=np.full((64, d), 2.5, np.float32))
    assert found[:10].all() and not found[10:].any() and same_bits(rec[:10], xb[-10:]) and np.all(rec[10:] == 2.5)
    rec, found = h.reconstruct_n(base + NB + 5, 33, out=np.full((33, d), 2.5, np.float32), want_found=False)
    assert np.all(rec == 2.5)
    rec, found = h.reconstruct_n(base, 0)
    assert rec.shape == (0, d) and found.shape == (0,)


def test_the_map_follows_the_lists(capi):
    metric, cen, assign, xb, xq = make_case("odd_30")
    d = xb.shape[1]
    h = make_handle(capi, metric, cen, xb, assign)
    model = Model(cen.shape[0], d, xb, assign)
    nb = len(xb)
    h.make_direct_map()
    assert h.direct_map_info() == [1, nb, 0, 1]
    h.search(xq[:5], 3, 4)  # (the lists are in use)
    # add: new rows with the next ids
    rs = np.random.RandomState(4)
    xa = odd_floats(rs, 50, d)
    la = rs.randint(0, cen.shape[0], size=50)
    h.add(xa, precomputed_idx=la)
    model.add(xa, np.arange(nb, nb + 50), la)
    assert same_bits(h.reconstruct(np.arange(nb - 5, nb + 50)), np.vstack([xb[-5:], xa]))
    assert h.direct_map_info() == [1, nb + 50, 0, 2]
    # update_lists: a row overwritten in place
    l = 3
    o = int(np.nonzero(model.ids[l] > 100)[0][0])  # (not one of the ids looked at below)
    new = odd_floats(rs, 1, d)
    the_id = int(model.ids[l][o])
    sizes = [len(i) for i in model.ids]
    h.update_lists(sizes, [(l << 32) | o], [the_id], new)
    model.update(sizes, [(l << 32) | o], [the_id], new)
    assert same_bits(h.reconstruct([the_id]), new)
    assert h.direct_map_info()[3] == 3
    rec, found = h.reconstruct_n(the_id, 1)
    assert same_bits(rec, new) and found.all()
    # remove_ids leaves a hole: ntotal shrinks below the largest id, the next call that needs the map says so and the map is off
    assert h.remove_ids([10]) == 1
    refused(capi, lambda: h.reconstruct([0]), "direct map supported only for")
    assert h.direct_map_info()[0] == 0
    refused(capi, lambda: h.reconstruct([0]), "direct map is not initialized")
    rec, found = h.reconstruct_n(9, 3, out=np.full((3, d), 1.5, np.float32))
    assert found.tolist() == [1, 0, 1] and np.all(rec[1] == 1.5) and same_bits(rec[[0, 2]], xb[[9, 11]])


# ------------------------------------------------------------------------------------------------ by label
@pytest.mark.parametrize("d", DIMS)
def test_reconstruct_from_offsets_over_every_entry(capi, d):
    nb = 1500 if d == 960 else NB
    h, model, xb, _ = ragged_world(capi, d, nb=nb, seed=31)
    labels = np.array([(l << 32) | o for l in range(NLIST) for o in range(len(model.ids[l]))] + [-1, -1], np.int64)
    labels = labels[np.random.RandomState(d).permutation(len(labels))]
    want_rows, want_ids = rows_of_labels(model, labels, d)
    rec, ids = h.reconstruct_from_offsets(labels)
    assert np.array_equal(ids, want_ids) and same_bits(rec, want_rows)
    none = labels == -1
    assert np.all(u32(rec[none]) == 0xffffffff) and np.all(ids[none] == -1)
    rec, ids = h.reconstruct_from_offsets(labels, want_ids=False)
    assert ids is None and same_bits(rec, want_rows)
    # one label that names nothing: refused, naming the position, the outputs untouched
    for bad in ((3 << 32) | len(model.ids[3]), (1 << 32) | 0, NLIST << 32, -2, (2 << 32) | 0xffffffff):
        lab = labels[:9].copy()
        lab[4] = bad
        sent, sent_ids = np.full((9, d), 4.5, np.float32), np.full(9, 99, np.int64)
        refused(capi, lambda: h.reconstruct_from_offsets(lab, out=sent, out_ids=sent_ids), "position 4")
        assert np.all(sent == 4.5) and np.all(sent_ids == 99)
    rec, ids = h.reconstruct_from_offsets([])
    assert rec.shape == (0, d)


# ------------------------------------------------------------------------------------------------ search and reconstruct
def expected_sar(h, model, x, k, nprobe, d):
    """(D, I) of the plain search, and the rows and ids of the positions a store_pairs search admits over the same coarse keys"""
    D, I = h.search(x, k, nprobe)
    cd, ck = h.coarse(x, nprobe, mode=0)
    Dp, P = h.search_preassigned(x, k, ck, cd, store_pairs=True)
    rows, ids = rows_of_labels(model, P, d)
    assert np.array_equal(u32(Dp), u32(D)) and np.array_equal(ids.reshape(I.shape), I)  # (the oracle pins both calls)
    return D, I, rows.reshape(len(x), k, d)


def check_sar(h, model, x, k, nprobe, d, what=""):
    D, I, R = expected_sar(h, model, x, k, nprobe, d)
    before = h.stats()
    d0, i0 = h.search(x, k, nprobe)
    mid = h.stats()
    D2, I2, R2 = h.search_and_reconstruct(x, k, nprobe)
    after = h.stats()
    assert np.array_equal(u32(D2), u32(D)) and np.array_equal(I2, I), what
    assert same_bits(R2, R), what
    assert np.all(u32(R2[I2 < 0]) == 0xffffffff), what
    assert {s: after[s] - mid[s] for s in mid} == {s: mid[s] - before[s] for s in mid}, what
    return D2, I2, R2


def byte_world(capi, d=128, metric=L2, seed=9):
    cen, assign, xb, xq = byte_case(d, NLIST, seed, nq=300, nb=NB)
    return make_handle(capi, metric, cen, xb, assign), Model(NLIST, d, xb, assign), xq, cen


def float_world(capi, name):
    metric, cen, assign, xb, xq = make_case(name)
    rs = np.random.RandomState(8)
    xq = np.vstack([xq, (cen[rs.randint(0, len(cen), size=44)] + 0.3 * rs.randn(44, xb.shape[1])).astype(np.float32)])
    return make_handle(capi, metric, cen, xb, assign), Model(cen.shape[0], xb.shape[1], xb, assign), xq


@pytest.mark.parametrize("world", ["bytes_l2", "bytes_ip", "ragged_l2", "ip_96", "odd_30"])
def test_search_and_reconstruct_equals_search_plus_the_admitted_rows(capi, world):
    if world.startswith("bytes"):
        h, model, xq, _ = byte_world(capi, metric=L2 if world == "bytes_l2" else IP)
        h.search(xq[:30], 5, 4)
        assert world != "bytes_l2" or h.scan_arith() == 2  # (the byte codes are in use: the rows still come back as stored floats)
    else:
        h, model, xq = float_world(capi, {"ragged_l2": "ragged"}.get(world, world))
    d = model.d
    # both sides of the 20-query and the 256-query regimes; a small call after a large one reuses the larger buffers
    for n in (300, 1, 19, 20):
        for k in (1, 10, 100):
            check_sar(h, model, xq[:n], k, 4, d, (world, n, k))
    check_sar(h, model, xq[:64], 10, NLIST, d, (world, "every list"))


def test_padding_duplicates_and_ties(capi):
    # k beyond what the probed lists hold: padding rows of 0xFF bytes behind ids of -1
    h, model, xb, cen = ragged_world(capi, 30, values="plain", seed=41)
    xq = (cen[[2, 3, 7, 8, 2, 12]] + 0.01).astype(np.float32)
    D, I, R = check_sar(h, model, xq, 100, 1, 30, "padding")
    assert (I < 0).any() and (I >= 0).any()
    # duplicate ids: the row is the admitted entry's, not the one the map would give
    h, model, dup, gone = duplicate_world(capi)
    where77 = [(l, o) for l in range(NLIST) for o, i in enumerate(model.ids[l]) if i == dup]
    xq = np.stack([model.codes[l][o] for l, o in where77]).astype(np.float32)
    D, I, R = check_sar(h, model, xq, 1, NLIST, 30, "duplicates")
    assert I[:, 0].tolist() == [dup] * 3 and same_bits(R[:, 0], xq)
    # ties: equidistant, different rows under different ids -- the row belongs to the returned id
    d, nl = 8, 8
    rs = np.random.RandomState(2)
    cen = (rs.randint(0, 2, size=(nl, d)) * 40).astype(np.float32)
    assign = rs.randint(0, nl, size=2000)
    xb = (cen[assign] + rs.randint(-1, 2, size=(2000, d))).astype(np.float32)  # (many entries at equal distances)
    xq = cen[rs.randint(0, nl, size=40)].astype(np.float32)
    h = make_handle(capi, L2, cen, xb, assign)
    model = Model(nl, d, xb, assign)
    for n in (5, 40):
        D, I, R = check_sar(h, model, xq[:n], 10, 4, d, "ties")
        assert same_bits(R, xb[I]) and (D[:, 1:] == D[:, :-1]).any()


def pinned(capi, shape, dtype):
    hip = capi.hip_runtime()
    p = C.c_void_p()
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert hip.hipHostMalloc(C.byref(p), C.c_size_t(nbytes), C.c_uint(0)) == 0
    buf = (C.c_char * nbytes).from_address(p.value)
    return np.frombuffer(buf, dtype=dtype).reshape(shape), p


def test_resident_clone_subset_and_pinned(capi):
    h, model, xq, cen = byte_world(capi, seed=17)
    d, n, k, nprobe = model.d, 120, 10, 4
    x = xq[:n]
    D, I, R = expected_sar(h, model, x, k, nprobe, d)
    # resident queries
    h.set_queries(xq)
    D2, I2, R2 = h.search_and_reconstruct_resident(0, n, k, nprobe)
    assert np.array_equal(u32(D2), u32(D)) and np.array_equal(I2, I) and same_bits(R2, R)
    D2, I2, R2 = h.search_and_reconstruct_resident(7, 20, k, nprobe)
    assert np.array_equal(u32(D2), u32(D[7:27])) and np.array_equal(I2, I[7:27]) and same_bits(R2, R[7:27])
    refused(capi, lambda: h.search_and_reconstruct_resident(len(xq) - 1, 2, k, nprobe), "range")
    # a clone: its own stream and workspaces over the owner's lists; the owner-only calls are refused there
    c = h.clone()
    D2, I2, R2 = c.search_and_reconstruct(x, k, nprobe)
    assert np.array_equal(u32(D2), u32(D)) and np.array_equal(I2, I) and same_bits(R2, R)
    rec, found = c.reconstruct_n(5, 9)
    assert found.all() and same_bits(rec, np.stack([last_rows(model)[i][0] for i in range(5, 14)]))
    refused(capi, c.make_direct_map, "amd_ivf_clone")
    refused(capi, lambda: c.reconstruct([0]), "amd_ivf_clone")
    c.close()
    # page-locked outputs: recons is written by the gather itself; pageable and page-locked results are the same bits
    bufs = [pinned(capi, (n, k), np.float32), pinned(capi, (n, k), np.int64), pinned(capi, (n, k, d), np.float32)]
    try:
        for direct in (1, 0):
            h.set_option("direct_out", direct)
            for a, _ in bufs:
                a.view(np.uint8)[...] = 0x5a
            D2, I2, R2 = h.search_and_reconstruct(x, k, nprobe, out=tuple(a for a, _ in bufs))
            assert np.array_equal(u32(D2), u32(D)) and np.array_equal(I2, I) and same_bits(R2, R), direct
    finally:
        h.set_option("direct_out", float("nan"))
        for _, p in bufs:
            capi.hip_runtime().hipHostFree(p)
    # a subset keeps no host rows: everything works on it, and equals an index built from the filtered lists
    sub = h.subset(capi.SUBSET_ID_MOD, 3, 1)
    fm = Model(NLIST, d, np.zeros((0, d), np.float32), np.zeros(0, np.int64))
    for l in range(NLIST):
        keep = model.ids[l] % 3 == 1
        fm.codes[l], fm.ids[l] = model.codes[l][keep], model.ids[l][keep]
    ref = capi.Handle(d, NLIST, L2, 0)
    ref.set_centroids(cen)
    set_model(ref, fm)
    assert sub.ntotal == ref.ntotal == sum(len(i) for i in fm.ids)
    D1, I1, R1 = sub.search_and_reconstruct(x, k, nprobe)
    Dr, Ir, Rr = ref.search_and_reconstruct(x, k, nprobe)
    assert np.array_equal(u32(D1), u32(Dr)) and np.array_equal(I1, Ir) and same_bits(R1, Rr)
    Ds, Is = sub.search(x, k, nprobe)
    cd, ck = sub.coarse(x, nprobe)
    _, P = sub.search_preassigned(x, k, ck, cd, store_pairs=True)
    rows, ids = rows_of_labels(fm, P, d)
    assert np.array_equal(u32(D1), u32(Ds)) and np.array_equal(I1, Is) and np.array_equal(ids.reshape(Is.shape), Is)
    assert same_bits(R1, rows.reshape(n, k, d))
    rec, found = sub.reconstruct_n(0, NB)
    want = last_rows(fm)
    assert sorted(np.nonzero(found)[0].tolist()) == sorted(want)
    assert all(same_bits(rec[i], want[i][0]) for i in want)
    refused(capi, sub.make_direct_map, "direct map supported only for")  # (ids 1, 4, 7, ...: not 0 .. ntotal - 1)
    sl = h.subset(capi.SUBSET_ID_RANGE, 0, 500)  # ids 0 .. 499: sequential from 0
    sl.make_direct_map()
    assert sl.direct_map_info() == [1, 500, 0, 1]
    allrows = last_rows(model)
    ids = np.random.RandomState(1).permutation(500)
    assert same_bits(sl.reconstruct(ids), np.stack([allrows[int(i)][0] for i in ids]))
    lab = [(l << 32) | 0 for l in range(NLIST) if sl.list_size(l)]
    rec, got = sl.reconstruct_from_offsets(lab)
    for r, g in zip(rec, got):
        assert 0 <= g < 500 and same_bits(r, allrows[int(g)][0])


def test_make_direct_map_with_tickets_out_is_refused(capi):
    h, model, xq, _ = byte_world(capi, seed=29)
    h.set_queries(xq)
    t = h.submit_search_resident(0, 64, 10, 4)
    try:
        refused(capi, h.make_direct_map, "tickets are still out")
    finally:
        h.wait(t)
    h.make_direct_map()
    assert h.direct_map_info()[:3] == [1, NB, 0]
