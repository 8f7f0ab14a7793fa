"""Search from and into device memory (include/auncel_amd.h: the `_dev` entry points).

Every comparison is of bytes, and the other side is always the host-pointer call on the same handle with x.cpu(): the `_dev` calls
run the same cores over rows that ingest_rows_kernel laid out instead of host_rows, so (D, I), the arithmetic the scan chose
(amd_ivf_scan_arith) and the adaptive call's my_nprobe / t_recalls must be the host call's, whatever the row stride, the element
type, the stream the rows were produced on or the place the results go to.  amd_ivf_last_dev_io says after every call that no query
row and no result byte crossed the bus.

Worlds: nlist 16, 2000 stored vectors, d in {8, 20, 128, 132} and 30 (the one at which rows are padded: dpad = 32), float lists and
uint8-valued lists, both metrics; calls of 1, 63, 64, 65 and 257 queries; k 1, 10 and 129.  The adaptive call needs
nlist > nlist / 8 + 20, so its world has 32 lists."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
L2, IP = 1, 0
NLIST, NB = 16, 2000
DS = (8, 20, 128, 132, 30)
NS = (1, 63, 64, 65, 257)
KS = (1, 10, 129)
FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def to_gpu(torch, a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def draw(rs, n, d, kind):
    if kind == "bytes":
        return np.floor(np.clip(rs.randn(n, d) * 40.0 + 120.0, 0, 255)).astype(np.float32)
    if kind == "unit":
        x = rs.randn(n, d)
        return (x / np.linalg.norm(x, axis=1, keepdims=True) * 0.9).astype(np.float32)
    return (rs.randn(n, d) * 1.5).astype(np.float32)


_WORLDS = {}


def world(d, metric, kind, nlist=NLIST):
    """stored rows, centroids, an assignment (nearest centroid, but list 0 keeps five rows: a query that is given list 0 alone cannot
    fill k = 10) and 257 query rows -- made once per shape and never changed"""
    key = (d, metric, kind, nlist)
    if key not in _WORLDS:
        rs = np.random.RandomState(1000 + 7 * d + 3 * metric + len(kind) + nlist)
        xb, xq = draw(rs, NB, d, kind), draw(rs, max(NS), d, kind)
        cen = xb[rs.choice(NB, nlist, replace=False)].copy()
        if metric == L2:
            dist = ((xb * xb).sum(1)[:, None] - 2.0 * xb @ cen.T + (cen * cen).sum(1)[None, :])
            assign = dist.argmin(1)
        else:
            assign = (xb @ cen.T).argmax(1)
        assign = assign.astype(np.int64)
        if nlist == NLIST:
            assign[assign == 0] = 1
            assign[:5] = 0
        for a in (xb, xq, cen, assign):
            a.setflags(write=False)
        _WORLDS[key] = dict(d=d, metric=metric, kind=kind, nlist=nlist, xb=xb, xq=xq, cen=cen, assign=assign)
    return _WORLDS[key]


def new_handle(capi, w):
    h = capi.Handle(w["d"], w["nlist"], w["metric"], 0)
    h.set_centroids(w["cen"])
    h.set_lists_from_assign(w["xb"], w["assign"])
    return h


def same(dev, host, tag):
    """(D, I) tensors of a `_dev` call against the host call's arrays, byte for byte"""
    D, I = dev[0].cpu().numpy(), dev[1].cpu().numpy()
    assert np.array_equal(I, host[1]), tag
    assert np.array_equal(bits(D), bits(host[0])), tag


def nothing_crossed(h, tag, stores=None):
    io = h.last_dev_io()
    assert io[0] == 0 and io[1] == 0, (tag, io)
    if stores is not None:
        assert io[3] == stores, (tag, io)
    return io


# ------------------------------------------------------------------------------------------------------------------------------
# 1. equality, every call
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["float", "bytes"])
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", DS)
def test_search_preassigned_and_exact_equal_the_host_calls(capi, torch, d, metric, kind):
    w = world(d, metric, kind)
    h = new_handle(capi, w)
    rs = np.random.RandomState(d)
    for n in NS:
        xq = w["xq"][:n]
        x = to_gpu(torch, xq)
        keys = np.stack([rs.permutation(NLIST)[:4] for _ in range(n)]).astype(np.int64)
        for k in KS:
            tag = (d, metric, kind, n, k)
            want = h.search(xq, k, 4)
            arith = h.scan_arith()
            same(h.search_dev(x, k, 4), want, tag)
            assert h.scan_arith() == arith, tag
            io = nothing_crossed(h, tag, stores=1)  # (the plain fixed-nprobe call: the selection stores into the caller's tensors)
            assert io[2] == 2, (tag, io)
            if kind == "bytes":
                assert arith == 2, tag
            want = h.search_preassigned(xq, k, keys)
            same(h.search_preassigned_dev(x, k, to_gpu(torch, keys)), want, tag + ("preassigned",))
            nothing_crossed(h, tag, stores=1)
            want = h.search_exact(xq, k)
            info = h.last_exact()
            same(h.search_exact_dev(x, k), want, tag + ("exact",))
            assert h.last_exact() == info, tag
            nothing_crossed(h, tag)
    h.close()


@gpu
@pytest.mark.parametrize("kind", ["float", "bytes"])
@pytest.mark.parametrize("metric", [L2, IP])
def test_resident_queries_equal_the_host_calls(capi, torch, metric, kind):
    """set_queries_dev, then slices of the resident set: the range of the set comes from the device"""
    for d in (20, 30):
        w = world(d, metric, kind)
        h = new_handle(capi, w)
        xq = w["xq"]
        n = len(xq)
        slices = ((0, n), (0, 1), (63, 2), (64, 65), (n - 63, 63))
        h.set_queries(xq)
        want = {(s, m, k): h.search_resident(s, m, k, 4) + (h.scan_arith(),) for s, m in slices for k in KS}
        h.set_queries(xq[:1] * 0.5)  # (what the host call left resident must not be what the device call searches)
        h.set_queries_dev(to_gpu(torch, xq))
        io = nothing_crossed(h, (d, "set_queries_dev"), stores=0)
        assert io[2] == 2
        for (s, m, k), (eD, eI, arith) in want.items():
            tag = (d, metric, kind, s, m, k)
            same(h.search_resident_dev(s, m, k, 4), (eD, eI), tag)
            assert h.scan_arith() == arith, tag
            io = nothing_crossed(h, tag, stores=1)
            assert io[2] == 0, (tag, io)
        # ... and the host call serves rows that came from the device
        for (s, m, k), (eD, eI, arith) in want.items():
            D, I = h.search_resident(s, m, k, 4)
            assert np.array_equal(I, eI) and np.array_equal(bits(D), bits(eD)) and h.scan_arith() == arith, (d, s, m, k)
        with pytest.raises(capi.EngineError):
            h.search_resident_dev(n - 1, 2, 1, 4)
        h.close()


def make_traces(rs, nlist):
    ntr = 1
    while (1 << ntr) <= nlist // 8:
        ntr += 1
    traces = []
    for _ in range(ntr):
        n = int(rs.randint(3, 60))
        x = np.sort(rs.rand(n) * 25.0).astype(np.float32)
        x += np.arange(n, dtype=np.float32) * 1e-3  # strictly ascending
        traces.append((x, (0.5 + rs.rand(n) * 2.5).astype(np.float32), (rs.rand(n) * 0.5).astype(np.float32)))
    return traces


@gpu
@pytest.mark.parametrize("metric,kind", [(L2, "float"), (L2, "bytes"), (IP, "unit")])
def test_adaptive_search_equals_the_host_call(capi, torch, metric, kind):
    """the tuner set as tests/test_gpu_random_adaptive.py sets it; (D, I), my_nprobe and t_recalls are the host call's"""
    d, nlist, K = 20, 32, 10
    w = world(d, metric, kind, nlist=nlist)
    h = new_handle(capi, w)
    rs = np.random.RandomState(77)
    h.set_interdis(None)
    h.set_tuner(K, make_traces(rs, nlist), capi.arcos_table())
    xq = w["xq"]
    n = len(xq)
    req = rs.choice([0.5, 0.8, 0.9, 0.95, 0.99], size=n).astype(np.float32)
    ran = 0
    for start, m in ((0, n), (0, 1), (60, 65), (64, 19)):
        for qk, mult, std_m in ((10, 1.0, 0.0), (3, 2.0, 1.0)):
            tag = (metric, kind, start, m, qk)
            np0, tr0 = np.zeros(n, np.uint64), np.zeros(n, np.float32)
            h.set_queries(xq)
            try:
                want, err = h.search_adaptive(start, m, qk, mult, std_m, req, np0, tr0), None
            except capi.EngineError as e:  # (the reference's own refusals are the same refusals from device memory)
                want, err = None, str(e)
            arith = h.scan_arith()
            np1, tr1 = np.zeros(n, np.uint64), np.zeros(n, np.float32)
            h.set_queries_dev(to_gpu(torch, xq))
            if err is not None:
                with pytest.raises(capi.EngineError) as got:
                    h.search_adaptive_dev(start, m, qk, mult, std_m, req, np1, tr1)
                assert str(got.value) == err, tag
                continue
            ran += 1
            same(h.search_adaptive_dev(start, m, qk, mult, std_m, req, np1, tr1), want, tag)
            assert np.array_equal(np1, np0) and np.array_equal(bits(tr1), bits(tr0)), tag
            assert h.scan_arith() == arith, tag
            nothing_crossed(h, tag, stores=1)
    assert ran > 0 or metric == IP
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the arithmetic choice
# ------------------------------------------------------------------------------------------------------------------------------
EDGES = [("bytes", None), ("255.5", 255.5), ("256", 256.0), ("4095", 4095.0), ("4097", 4097.0), ("-4095", -4095.0), ("-4097", -4097.0),
         ("-0.0", -0.0), ("nan", float("nan")), ("inf", float("inf"))]


@gpu
@pytest.mark.parametrize("d", [20, 30])
@pytest.mark.parametrize("metric", [L2, IP])
def test_the_arithmetic_choice_is_the_host_calls(capi, torch, metric, d):
    """one odd element among byte-valued queries, at every place a reduction can lose it: element 0, the last element of the last
    row, the last of row 63 and the first of row 64 (a wave's and a workgroup's edge), and the first element of the last row, which
    lies in the launch's last, partly filled workgroup"""
    w = world(d, metric, "bytes")
    h = new_handle(capi, w)
    n = 257
    assert (n * ((d + 3) // 4)) % 256 != 0
    places = [(0, 0), (n - 1, d - 1), (63, d - 1), (64, 0), (n - 1, 0)]
    seen = set()
    for name, v in EDGES:
        for r, c in (places if v is not None else places[:1]):
            xq = w["xq"][:n].copy()
            if v is not None:
                xq[r, c] = v
            tag = (metric, d, name, r, c)
            want = h.search(xq, 10, 4)
            arith = h.scan_arith()
            same(h.search_dev(to_gpu(torch, xq), 10, 4), want, tag)
            assert h.scan_arith() == arith, tag
            nothing_crossed(h, tag, stores=1)
            if name in ("bytes", "-0.0"):
                assert arith == 2, tag  # (fails if the range is not computed at all)
            if name in ("255.5", "4097", "-4097", "nan", "inf"):
                assert arith == 0, tag
            seen.add(arith)
    assert seen == {0, 1, 2}
    h.close()


@gpu
def test_the_range_of_a_grid_strided_launch(capi, torch):
    """more rows than one pass of the ingest grid covers (512 workgroups of 256 four-column groups): the odd element in the very
    last row still decides"""
    d, n = 20, 26300
    assert n * (d // 4) > 512 * 256
    w = world(d, L2, "bytes")
    h = new_handle(capi, w)
    xq = np.tile(w["xq"], (n // len(w["xq"]) + 1, 1))[:n].copy()
    for v, arith in ((None, 2), (255.5, 0), (300.0, 1)):
        if v is not None:
            xq[n - 1, d - 1] = v
        want = h.search(xq, 1, 1)
        assert h.scan_arith() == arith
        same(h.search_dev(to_gpu(torch, xq), 1, 1), want, v)
        assert h.scan_arith() == arith
        nothing_crossed(h, v, stores=1)
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the stride gap is not read, 4. half input
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["float", "bytes"])
@pytest.mark.parametrize("d", DS)
def test_the_stride_gap_is_not_read(capi, torch, d, kind):
    """x = big[:, a : a + d]: the other columns hold NaN and 0.5, either of which would change the choice (and NaN the bytes).  Widths
    and offsets for both forms of the kernel's loads: 16-byte groups (a = 0, width % 4 == 0) and single elements"""
    w = world(d, L2, kind)
    h = new_handle(capi, w)
    for n in (1, 65, 257):
        xq = w["xq"][:n]
        want = h.search(xq, 10, 4)
        arith = h.scan_arith()
        for width, a in ((d + 8, 0), (d + 8, 3), (d + 7, 0), (d + 1, 1)):
            big = torch.empty((n, width), dtype=torch.float32, device="cuda")
            big[:, 0::2] = float("nan")
            big[:, 1::2] = 0.5
            big[:, a:a + d] = to_gpu(torch, xq)
            x = big[:, a:a + d]
            assert x.stride(0) == width or n == 1
            tag = (d, kind, n, width, a)
            same(h.search_dev(x, 10, 4), want, tag)
            assert h.scan_arith() == arith, tag
            nothing_crossed(h, tag, stores=1)
            same(h.search_exact_dev(x, 10), h.search_exact(xq, 10), tag + ("exact",))
    h.close()


@gpu
@pytest.mark.parametrize("kind", ["float", "bytes"])
@pytest.mark.parametrize("d", DS)
def test_half_input(capi, torch, d, kind):
    """values fp16 holds exactly: the result is the host call's on x.half().float(), the arithmetic choice included"""
    w = world(d, L2, kind)
    h = new_handle(capi, w)
    for n in (1, 64, 257):
        xq = np.round(w["xq"][:n] * 8.0) / 8.0 if kind == "float" else w["xq"][:n]
        xh = to_gpu(torch, xq).half()
        back = xh.float().cpu().numpy()
        assert np.array_equal(back, xq)
        want = h.search(back, 10, 4)
        arith = h.scan_arith()
        if kind == "bytes":
            assert arith == 2
        same(h.search_dev(xh, 10, 4), want, (d, kind, n))
        assert h.scan_arith() == arith
        nothing_crossed(h, (d, kind, n), stores=1)
        wide = torch.zeros((n, d + 3), dtype=torch.float16, device="cuda") + 0.5  # (odd stride: element loads)
        wide[:, 1:1 + d] = xh
        same(h.search_dev(wide[:, 1:1 + d], 10, 4), want, (d, kind, n, "strided"))
        assert h.scan_arith() == arith
    h.set_queries(back)
    want = h.search_resident(0, n, 10, 4)
    h.set_queries_dev(xh)
    same(h.search_resident_dev(0, n, 10, 4), want, "resident")
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 5. output placement, 6. stream order
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_output_placement_and_padding(capi, torch, metric):
    """(D, I) are rows inside larger tensors whose other rows keep their sentinels; a query that is given the five-row list alone
    gets five results and the reference's padding: -1 and +-FLT_MAX"""
    d, n, k = 20, 65, 10
    w = world(d, metric, "float")
    h = new_handle(capi, w)
    xq = w["xq"][:n]
    x = to_gpu(torch, xq)
    keys = np.zeros((n, 1), np.int64)
    calls = [("search", lambda out: h.search_dev(x, k, 4, out=out), lambda: h.search(xq, k, 4)),
             ("preassigned", lambda out: h.search_preassigned_dev(x, k, to_gpu(torch, keys), out=out),
              lambda: h.search_preassigned(xq, k, keys)),
             ("exact", lambda out: h.search_exact_dev(x, k, out=out), lambda: h.search_exact(xq, k))]
    for name, dev, host in calls:
        bigD = torch.full((n + 6, k), 12345.5, dtype=torch.float32, device="cuda")
        bigI = torch.full((n + 6, k), -777, dtype=torch.int64, device="cuda")
        D, I = dev((bigD[3:3 + n], bigI[3:3 + n]))
        assert D.data_ptr() == bigD[3:].data_ptr() and I.data_ptr() == bigI[3:].data_ptr()
        want = host()
        same((bigD[3:3 + n], bigI[3:3 + n]), want, name)
        for sentinel in (bigD[:3], bigD[3 + n:]):
            assert bool((sentinel == 12345.5).all()), name
        for sentinel in (bigI[:3], bigI[3 + n:]):
            assert bool((sentinel == -777).all()), name
        nothing_crossed(h, name)
        if name == "preassigned":
            got = bigI[3:3 + n].cpu().numpy()
            assert (got[:, :5] >= 0).all() and (got[:, 5:] == -1).all()
            pad = bigD[3:3 + n, 5:].cpu().numpy()
            assert np.array_equal(bits(pad), bits(np.full_like(pad, FMAX if metric == L2 else -FMAX)))
    h.close()


@gpu
def test_stream_order(capi, torch):
    """x is the end of a chain of device work on a side stream and is searched from that stream with no host synchronisation in
    between: the engine's stream waits for the chain"""
    d, n = 128, 257
    w = world(d, L2, "bytes")
    h = new_handle(capi, w)
    xq = w["xq"][:n]
    want = h.search(xq, 10, 4)
    base = to_gpu(torch, xq)
    ballast = torch.ones((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        acc = ballast
        for _ in range(20):  # (tens of milliseconds of work in front of x)
            acc = (acc @ ballast).clamp_(0, 1)
        x = torch.full_like(base, float("nan"))
        x.copy_(base + acc[0, 0] - 1.0)  # (= base, once the chain has run: acc is all ones)
        for _ in range(50):
            x = x + 1.0
        x = x - 50.0
        out = h.search_dev(x, 10, 4)
    same(out, want, "side stream")
    assert h.scan_arith() == 2
    nothing_crossed(h, "side stream", stores=1)
    h.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 8. refusals, 9. a clone
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_the_results_untouched(capi, torch):
    d, n, k = 20, 8, 4
    w = world(d, L2, "float")
    h = new_handle(capi, w)
    L = capi.lib()
    x = to_gpu(torch, w["xq"][:n])
    xh = x.half()
    x_cpu = torch.from_numpy(w["xq"][:n].copy())
    D = torch.full((n, k), 3.25, dtype=torch.float32, device="cuda")
    I = torch.full((n, k), -5, dtype=torch.int64, device="cuda")
    D_cpu, I_cpu = torch.zeros((n, k)), torch.zeros((n, k), dtype=torch.int64)
    keys = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    sz, p = C.c_size_t, C.c_void_p
    stream = p(torch.cuda.current_stream().cuda_stream)

    def search(xp=x.data_ptr(), dtype=0, ldx=d, Dp=D.data_ptr(), Ip=I.data_ptr(), nn=n):
        return L.amd_ivf_search_dev(h._h, sz(nn), p(xp), dtype, sz(ldx), sz(k), sz(4), 0, p(Dp), p(Ip), stream)

    def refused(rc, word):
        assert rc == -2
        msg = L.amd_ivf_last_error()
        assert msg and word in msg, msg
        torch.cuda.synchronize()
        assert bool((D == 3.25).all()) and bool((I == -5).all())
        assert not D_cpu.any() and not I_cpu.any()

    refused(search(xp=x_cpu.data_ptr()), b"not a device pointer")
    refused(search(ldx=d - 1), b"ldx")
    refused(search(dtype=2), b"dtype")
    refused(search(dtype=-1), b"dtype")
    refused(search(xp=None), b"null pointer")
    refused(search(Dp=None), b"null pointer")
    refused(search(Ip=None), b"null pointer")
    refused(search(xp=x.data_ptr() + 1), b"misaligned")
    refused(search(xp=x.data_ptr() + 2), b"misaligned")
    refused(search(xp=xh.data_ptr() + 1, dtype=1), b"misaligned")
    refused(search(Dp=D.data_ptr() + 2), b"misaligned")
    refused(search(Ip=I.data_ptr() + 4), b"misaligned")
    refused(search(Dp=D_cpu.data_ptr()), b"not a device pointer")
    refused(search(Ip=I_cpu.data_ptr()), b"not a device pointer")
    refused(L.amd_ivf_search_exact_dev(h._h, sz(n), p(x_cpu.data_ptr()), 0, sz(d), sz(k), p(D.data_ptr()), p(I.data_ptr()), stream),
            b"not a device pointer")
    refused(L.amd_ivf_search_exact_dev(h._h, sz(n), p(x.data_ptr()), 0, sz(d), sz(0), p(D.data_ptr()), p(I.data_ptr()), stream), b"k must be positive")
    refused(L.amd_ivf_search_preassigned_dev(h._h, sz(n), p(x.data_ptr()), 0, sz(d), sz(k), sz(2), None, p(D.data_ptr()), p(I.data_ptr()), stream),
            b"null pointer")
    refused(L.amd_ivf_search_preassigned_dev(h._h, sz(n), p(x.data_ptr()), 0, sz(d - 1), sz(k), sz(2), p(keys.data_ptr()), p(D.data_ptr()),
                                             p(I.data_ptr()), stream), b"ldx")
    refused(L.amd_ivf_set_queries_dev(h._h, sz(n), p(x_cpu.data_ptr()), 0, sz(d), stream), b"not a device pointer")
    refused(L.amd_ivf_set_queries_dev(h._h, sz(n), p(x.data_ptr()), 3, sz(d), stream), b"dtype")
    h.set_queries_dev(x)
    refused(L.amd_ivf_search_resident_dev(h._h, sz(0), sz(n), sz(k), sz(4), 0, p(D_cpu.data_ptr()), p(I.data_ptr())), b"not a device pointer")
    refused(L.amd_ivf_search_resident_dev(h._h, sz(1), sz(n), sz(k), sz(4), 0, p(D.data_ptr()), p(I.data_ptr())), b"out of bounds")
    # the Python layer's own
    with pytest.raises(ValueError):
        h.search_dev(x.t().contiguous().t(), k, 4)  # (columns not contiguous)
    with pytest.raises(ValueError):
        h.search_dev(x_cpu, k, 4)
    with pytest.raises(ValueError):
        h.search_dev(x.double(), k, 4)
    # n = 0: nothing to do, nothing touched -- whatever the other arguments are
    assert search(nn=0, xp=None, Dp=None, Ip=None) == 0
    assert L.amd_ivf_set_queries_dev(h._h, sz(0), None, 0, sz(d), stream) == 0
    assert L.amd_ivf_search_exact_dev(h._h, sz(0), None, 0, sz(d), sz(k), None, None, stream) == 0
    eD, eI = h.search_dev(x[:0], k, 4)
    assert tuple(eD.shape) == (0, k) and tuple(eI.shape) == (0, k)
    assert bool((D == 3.25).all()) and bool((I == -5).all())
    # ... and the handle still serves
    same(h.search_dev(x, k, 4), h.search(w["xq"][:n], k, 4), "after the refusals")
    h.close()


@gpu
@pytest.mark.parametrize("kind", ["float", "bytes"])
def test_a_clone_serves_search_dev(capi, torch, kind):
    w = world(30, L2, kind)
    h = new_handle(capi, w)
    cl = h.clone()
    for n in (1, 257):
        xq = w["xq"][:n]
        x = to_gpu(torch, xq)
        want = h.search(xq, 10, 4)
        arith = h.scan_arith()
        same(cl.search_dev(x, 10, 4), want, (kind, n))
        assert cl.scan_arith() == arith
        nothing_crossed(cl, (kind, n), stores=1)
        same(cl.search_dev(x, 10, 4), cl.search(xq, 10, 4), (kind, n, "clone's own host call"))
        same(cl.search_exact_dev(x, 10), h.search_exact(xq, 10), (kind, n, "exact"))
    cl.close()
    h.close()
