"""ctypes binding of include/auncel_amd.h (the C-ABI drop-in boundary).

Fails loudly when libauncel_amd.so is missing: there is no CPU path in this package."""
import ctypes as C
import os

import numpy as np

from . import build as _build

METRIC_IP, METRIC_L2 = 0, 1
SUBSET_ID_RANGE, SUBSET_ID_MOD, SUBSET_SLICE, SUBSET_ID_BITS, SUBSET_ID_BATCH = 0, 1, 2, 5, 6
SELECTOR_AND, SELECTOR_OR, SELECTOR_ANDNOT, SELECTOR_NOT = 0, 1, 2, 3

_f32p = C.POINTER(C.c_float)
_i64p = C.POINTER(C.c_int64)
_u64p = C.POINTER(C.c_uint64)
_szp = C.POINTER(C.c_size_t)
_LIB = None

SYMBOLS = [
    "amd_ivf_last_error", "amd_ivf_device_count", "amd_ivf_create", "amd_ivf_clone", "amd_ivf_destroy", "amd_ivf_set_centroids",
    "amd_ivf_set_lists", "amd_ivf_add", "amd_ivf_ntotal", "amd_ivf_list_size", "amd_ivf_get_list", "amd_ivf_coarse",
    "amd_ivf_search_preassigned", "amd_ivf_search", "amd_ivf_scan_codes", "amd_ivf_scan_codes_at", "amd_ivf_scan_codes_range",
    "amd_ivf_scan_codes_range_results", "amd_ivf_distance_to_code", "amd_ivf_stats",
    "amd_ivf_set_queries", "amd_ivf_search_resident", "amd_ivf_search_resident_preassigned", "amd_ivf_coarse_resident", "amd_ivf_set_interdis", "amd_ivf_get_interdis",
    "amd_ivf_set_tuner", "amd_ivf_search_adaptive", "amd_ivf_search_adaptive_x", "amd_ivf_search_adaptive_pre", "amd_ivf_search_timed", "amd_ivf_search_timed_x",
    "amd_ivf_train_samples",
    "amd_ivf_train_samples_x", "amd_ivf_train_samples_pre", "amd_ivf_trace_sb", "amd_ivf_arcos_table", "amd_ivf_merge_tables",
    "amd_ivf_last_timing", "amd_ivf_last_timing_detail", "amd_ivf_last_scan_min_bytes", "amd_ivf_coarse_tie_rows", "amd_ivf_last_tie_fixed", "amd_ivf_last_filter", "amd_ivf_last_direct_out", "amd_ivf_last_coarse_pick", "amd_ivf_set_async_depth", "amd_ivf_submit_adaptive", "amd_ivf_submit_search_resident", "amd_ivf_submit_coarse_resident",
    "amd_ivf_submit_search_resident_preassigned", "amd_ivf_wait", "amd_ivf_async_counts", "amd_ivf_last_tie_redone", "amd_ivf_last_tie_patched", "amd_ivf_self_check", "amd_ivf_last_round_hints", "amd_ivf_set_byte_codes", "amd_ivf_set_option", "amd_ivf_get_option",
    "amd_ivf_kmeans",
    "amd_ivf_range_search_preassigned", "amd_ivf_range_search", "amd_ivf_range_results",
    "amd_ivf_scan_arith",
    "amd_ivf_update_lists", "amd_ivf_remove_ids", "amd_ivf_last_update", "amd_ivf_layout_digest",
    "amd_ivf_subset", "amd_ivf_last_subset", "amd_ivf_concat", "amd_ivf_last_concat",
    "amd_ivf_selector_create", "amd_ivf_selector_destroy", "amd_ivf_selector_info",
    "amd_ivf_search_selected", "amd_ivf_search_preassigned_selected", "amd_ivf_search_resident_selected",
    "amd_ivf_selector_combine", "amd_ivf_range_search_selected", "amd_ivf_range_search_preassigned_selected",
    "amd_ivf_submit_search_resident_selected",
    "amd_ivf_search_selected_each", "amd_ivf_search_preassigned_selected_each", "amd_ivf_search_resident_selected_each",
    "amd_ivf_search_adaptive_selected", "amd_ivf_search_adaptive_x_selected", "amd_ivf_search_adaptive_selected_each",
    "amd_ivf_train_samples_selected",
    "amd_ivf_search_exact", "amd_ivf_search_exact_resident", "amd_ivf_last_exact", "amd_ivf_last_exact_detail",
    "amd_ivf_search_exact_selected", "amd_ivf_search_exact_resident_selected",
    "amd_ivf_range_search_exact", "amd_ivf_range_search_exact_resident", "amd_ivf_range_search_exact_selected", "amd_ivf_last_range_exact",
    "amd_ivf_make_direct_map", "amd_ivf_direct_map_info", "amd_ivf_reconstruct", "amd_ivf_reconstruct_n", "amd_ivf_reconstruct_from_offsets",
    "amd_ivf_search_and_reconstruct", "amd_ivf_search_and_reconstruct_resident",
    "amd_ivf_set_queries_dev", "amd_ivf_search_dev", "amd_ivf_search_preassigned_dev", "amd_ivf_search_resident_dev",
    "amd_ivf_search_exact_dev", "amd_ivf_search_adaptive_dev", "amd_ivf_last_dev_io",
    "amd_ivf_read_fvecs", "amd_ivf_read_ivecs", "amd_ivf_read_fbin", "amd_ivf_read_ibin", "amd_ivf_free",
]


class Part(C.Structure):
    """amd_ivf_part_t (include/auncel_amd.h: amd_ivf_concat)"""
    _fields_ = [("h", C.c_void_p), ("begin", _u64p), ("end", _u64p), ("id_add", C.c_int64)]


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"auncel_amd error {code}: {msg}")
        self.code = code


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  A process that loads torch first runs this library on
    that runtime too (its hip* symbols bind to the copy already in the global scope); a process that creates an index first gets
    ROCm's copy for the library and torch's for torch -- and the second runtime to start finds no device ("No HIP GPUs are
    available").  So where torch is installed but not yet imported, its runtime is loaded first, globally, and both orders behave
    like the first.  (C and C++ callers link one runtime and have no such choice to make.)"""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("AUNCEL_AMD_OWN_HIP_RUNTIME"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    d = os.path.join(os.path.dirname(spec.origin), "lib")
    names = ("libhsa-runtime64.so", "libamdhip64.so")
    if not all(os.path.exists(os.path.join(d, n)) for n in names):
        return  # (a torch build without a bundled runtime: it uses ROCm's, like the engine)
    for name in names:
        try:
            _SHARED[name] = C.CDLL(os.path.join(d, name), mode=C.RTLD_GLOBAL)
        except OSError as e:
            # half a runtime (torch's HSA under ROCm's HIP) is worse than either: say so instead of going on
            raise ImportError(f"auncel_amd: torch's bundled {name} could not be loaded next to {sorted(_SHARED)} ({e}); set "
                              "AUNCEL_AMD_OWN_HIP_RUNTIME=1 to run the engine on ROCm's own runtime (and do not use torch's GPU "
                              "side in the same process)") from e
    if os.environ.get("AUNCEL_AMD_VERBOSE"):
        print(f"[auncel_amd] running on torch's bundled HIP runtime ({d}); AUNCEL_AMD_OWN_HIP_RUNTIME=1 keeps ROCm's", file=sys.stderr)


_SHARED = {}


def hip_runtime():
    """a ctypes handle on the HIP runtime this process uses (hipHostMalloc for page-locked result buffers, ...): torch's bundled
    copy where torch is loaded or was pre-loaded by lib(), else ROCm's -- never a second runtime beside the first"""
    import sys
    lib()
    if "libamdhip64.so" in _SHARED:
        return _SHARED["libamdhip64.so"]
    if "torch" in sys.modules:
        p = os.path.join(os.path.dirname(sys.modules["torch"].__file__), "lib", "libamdhip64.so")
        if os.path.exists(p):
            return C.CDLL(p)
    return C.CDLL("libamdhip64.so")


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_build.LIB):
            raise ImportError(f"{_build.LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950).  auncel_amd has no CPU fallback.")
        _share_torch_hip_runtime()
        L = C.CDLL(os.environ.get("AUNCEL_AMD_LIB", _build.LIB))  # AUNCEL_AMD_LIB: a differently built engine (kernel experiments)
        L.amd_ivf_last_error.restype = C.c_char_p
        for s in SYMBOLS[1:]:
            getattr(L, s).restype = C.c_int
        L.amd_ivf_free.restype = None
        _LIB = L
    return _LIB


def _chk(rc):
    if rc != 0:
        raise EngineError(rc, lib().amd_ivf_last_error().decode())


def _f(a):
    return a.ctypes.data_as(_f32p) if a is not None else None


def _i(a):
    return a.ctypes.data_as(_i64p) if a is not None else None


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def device_count():
    n = C.c_int(0)
    _chk(lib().amd_ivf_device_count(C.byref(n)))
    return n.value


def self_check(device=0):
    """include/auncel_amd.h: amd_ivf_self_check -> dict(adds, counted, wrong, xcd_mask)"""
    v = (C.c_uint64 * 4)()
    _chk(lib().amd_ivf_self_check(int(device), v))
    return {"adds": int(v[0]), "counted": int(v[1]), "wrong": int(v[2]), "xcd_mask": int(v[3])}


def kmeans(metric, x, k, niter=25, seed=1234, max_points_per_centroid=256, spherical=False, int_centroids=False, coarse_mode=0,
           device=0):
    """Clustering::train on the GPU (include/auncel_amd.h: amd_ivf_kmeans) -> centroids (k, d), objective per iteration"""
    x = f32(x)
    n, d = x.shape
    cen = np.zeros((k, d), np.float32)
    obj = np.zeros(niter, np.float32)
    _chk(lib().amd_ivf_kmeans(int(d), C.c_size_t(n), _f(x), C.c_size_t(k), int(metric), int(niter), C.c_long(seed),
                              C.c_size_t(max_points_per_centroid), int(spherical), int(int_centroids), int(coarse_mode), int(device),
                              _f(cen), _f(obj)))
    return cen, obj


def merge_tables(metric, all_D, all_I):
    all_D, all_I = f32(all_D), i64(all_I)
    nshard, n, k = all_D.shape
    D = np.empty((n, k), np.float32)
    I = np.empty((n, k), np.int64)
    _chk(lib().amd_ivf_merge_tables(metric, C.c_size_t(n), C.c_size_t(k), C.c_size_t(nshard), _f(all_D), _i(all_I), _f(D), _i(I)))
    return D, I


def trace_sb(raw_xy, bs=250):
    raw = f32(raw_xy)
    n = raw.shape[0]
    cap = n // bs + 2
    ox, oy, os_ = (np.zeros(cap, np.float32) for _ in range(3))
    nb = C.c_size_t(0)
    _chk(lib().amd_ivf_trace_sb(_f(raw), C.c_size_t(n), C.c_size_t(bs), _f(ox), _f(oy), _f(os_), C.byref(nb)))
    return ox[:nb.value].copy(), oy[:nb.value].copy(), os_[:nb.value].copy()


def _take(ptr, n, d, ctype, dtype):
    """copy a malloc'ed n x d matrix out of the library and release it"""
    try:
        out = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n * d,)).astype(dtype, copy=True).reshape(n, d) if n * d else np.zeros((n, d), dtype)
    finally:
        lib().amd_ivf_free(ptr)
    return out


def read_fvecs(path):
    """fvecs_read (Auncel/eval/bound.cpp:29-58) -> float32 (n, d)"""
    d, n, p = C.c_size_t(0), C.c_size_t(0), _f32p()
    _chk(lib().amd_ivf_read_fvecs(os.fsencode(path), C.byref(d), C.byref(n), C.byref(p)))
    return _take(p, n.value, d.value, C.c_float, np.float32)


def read_ivecs(path):
    """ivecs_read (Auncel/eval/bound.cpp:61-63) -> int32 (n, d)"""
    d, n, p = C.c_size_t(0), C.c_size_t(0), C.POINTER(C.c_int32)()
    _chk(lib().amd_ivf_read_ivecs(os.fsencode(path), C.byref(d), C.byref(n), C.byref(p)))
    return _take(p, n.value, d.value, C.c_int32, np.int32)


def read_fbin(path, num=0, nbytes=4):
    """fbin_read (Auncel/eval/bound.cpp:65-109): `num` rows (0: the header's count); nbytes 1 = signed chars widened, as the
    harness reads its u8 SIFT files -> float32 (rows, d), header row count"""
    d, n, p = C.c_size_t(0), C.c_size_t(0), _f32p()
    _chk(lib().amd_ivf_read_fbin(os.fsencode(path), C.c_size_t(num), int(nbytes), C.byref(d), C.byref(n), C.byref(p)))
    return _take(p, num if num else n.value, d.value, C.c_float, np.float32), n.value


def read_ibin(path, num=0):
    """ibin_read (Auncel/eval/bound.cpp:111-113) -> int32 (rows, d), header row count"""
    d, n, p = C.c_size_t(0), C.c_size_t(0), C.POINTER(C.c_int32)()
    _chk(lib().amd_ivf_read_ibin(os.fsencode(path), C.c_size_t(num), C.byref(d), C.byref(n), C.byref(p)))
    return _take(p, num if num else n.value, d.value, C.c_int32, np.int32), n.value


def arcos_table():
    """error_pro::construct_arcos (IVF_pro.cpp:151-160): 500-entry acos LUT, fp32"""
    out = np.zeros(500, np.float32)
    _chk(lib().amd_ivf_arcos_table(_f(out)))
    return out


class Selector:
    """thin owner of an amd_ivf_selector_t*: the keep bits of one id selector over one index (the arguments of Handle.subset).  It
    keeps its index's Handle alive and is closed before it; `with handle.selector(...) as s:` closes it on the way out."""

    def __init__(self, handle, kind, a1=0, a2=0, sel=None):
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.uint64 if kind == SUBSET_ID_BITS else np.int64)
        self._s = C.c_void_p()
        self._index = handle
        _chk(lib().amd_ivf_selector_create(handle._h, int(kind), C.c_int64(int(a1)), C.c_int64(int(a2)),
                                           sel.ctypes.data_as(C.c_void_p) if sel is not None else None,
                                           C.c_size_t(0 if sel is None else sel.shape[0]), C.byref(self._s)))

    def info(self):
        """(entries looked at, entries kept, host-to-device bytes, device bytes held)"""
        out = (C.c_uint64 * 4)()
        _chk(lib().amd_ivf_selector_info(self._s, out))
        return tuple(int(v) for v in out)

    def combine(self, op, other=None):
        """a new Selector of the same index from this one and `other` (SELECTOR_AND / OR / ANDNOT), or from this one alone
        (SELECTOR_NOT: every stored entry it does not keep); made on the device, and alive on its own"""
        out = Selector.__new__(Selector)
        out._s = C.c_void_p()
        out._index = self._index
        _chk(lib().amd_ivf_selector_combine(int(op), self._s, other._s if other is not None else None, C.byref(out._s)))
        return out

    def __and__(self, other):
        return self.combine(SELECTOR_AND, other)

    def __or__(self, other):
        return self.combine(SELECTOR_OR, other)

    def __sub__(self, other):
        return self.combine(SELECTOR_ANDNOT, other)

    def __invert__(self):
        return self.combine(SELECTOR_NOT)

    def close(self):
        if self._s:
            rc = lib().amd_ivf_selector_destroy(self._s)
            if rc == -2:  # (refused: tickets that search under it are still out -- the selector stays valid)
                raise EngineError(rc, lib().amd_ivf_last_error().decode())
            self._s = C.c_void_p()

    destroy = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Handle:
    """thin owner of an amd_ivf_t*"""

    def __init__(self, d, nlist, metric=METRIC_L2, device=0):
        self.d, self.nlist, self.metric, self.device = int(d), int(nlist), int(metric), int(device)
        self._h = C.c_void_p()
        _chk(lib().amd_ivf_create(self.d, C.c_size_t(self.nlist), self.metric, self.device, C.byref(self._h)))

    def clone(self):
        """a second search context over the same device-resident index (include/auncel_amd.h: amd_ivf_clone); the
        owner is kept alive by the clone"""
        c = Handle.__new__(Handle)
        c.d, c.nlist, c.metric, c.device = self.d, self.nlist, self.metric, self.device
        c._h = C.c_void_p()
        c._owner = self
        for attr in ("max_topk",):  # tuner geometry set on the owner by set_tuner
            if hasattr(self, attr):
                setattr(c, attr, getattr(self, attr))
        _chk(lib().amd_ivf_clone(self._h, C.byref(c._h)))
        return c

    def close(self):
        if self._h:
            rc = lib().amd_ivf_destroy(self._h)
            if rc == -2:  # (refused: selectors made on the index are still alive -- the handle stays valid)
                raise EngineError(rc, lib().amd_ivf_last_error().decode())
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- contents
    def set_centroids(self, c):
        c = f32(c)
        assert c.shape == (self.nlist, self.d)
        _chk(lib().amd_ivf_set_centroids(self._h, _f(c)))

    def set_lists(self, sizes, codes, ids):
        sizes = np.ascontiguousarray(sizes, dtype=np.uintp)
        codes = [f32(c) for c in codes]
        ids = [i64(i) for i in ids]
        cp = (_f32p * self.nlist)(*[_f(c) for c in codes])
        ip = (_i64p * self.nlist)(*[_i(i) for i in ids])
        _chk(lib().amd_ivf_set_lists(self._h, sizes.ctypes.data_as(_szp), cp, ip))

    def set_lists_from_assign(self, xb, assign, ids=None):
        """lists as IndexIVFFlat::add_core builds them: database order inside every list"""
        assign = np.asarray(assign, dtype=np.int64)
        gid = np.arange(len(assign), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
        keep = np.nonzero(assign >= 0)[0]
        order = keep[np.argsort(assign[keep], kind="stable")]
        sizes = np.bincount(assign[keep], minlength=self.nlist)
        off = np.concatenate([[0], np.cumsum(sizes)])
        xs, gs = f32(xb)[order], gid[order]
        self.set_lists(sizes, [xs[off[l]:off[l + 1]] for l in range(self.nlist)],
                       [gs[off[l]:off[l + 1]] for l in range(self.nlist)])

    def add(self, x, xids=None, precomputed_idx=None):
        x = f32(x)
        xi = i64(xids) if xids is not None else None
        pi = i64(precomputed_idx) if precomputed_idx is not None else None
        _chk(lib().amd_ivf_add(self._h, C.c_size_t(x.shape[0]), _f(x), _i(xi), _i(pi)))

    @property
    def ntotal(self):
        n = C.c_size_t(0)
        _chk(lib().amd_ivf_ntotal(self._h, C.byref(n)))
        return n.value

    def list_size(self, l):
        n = C.c_size_t(0)
        _chk(lib().amd_ivf_list_size(self._h, C.c_size_t(l), C.byref(n)))
        return n.value

    def get_list(self, l):
        n = self.list_size(l)
        codes = np.empty((n, self.d), np.float32)
        ids = np.empty(n, np.int64)
        _chk(lib().amd_ivf_get_list(self._h, C.c_size_t(l), _f(codes), _i(ids)))
        return codes, ids

    # ---- changes in place (include/auncel_amd.h: amd_ivf_update_lists ...)
    def update_lists(self, sizes, where, ids, codes):
        """new list sizes + written entries: where[i] = list << 32 | offset, ids[i], codes[i] (d floats)"""
        sizes = np.ascontiguousarray(sizes, dtype=np.uintp)
        assert sizes.shape == (self.nlist,)
        where = np.ascontiguousarray(where, dtype=np.uint64)
        ids, codes = i64(ids), f32(codes).reshape(-1, self.d)
        assert where.shape[0] == ids.shape[0] == codes.shape[0]
        _chk(lib().amd_ivf_update_lists(self._h, sizes.ctypes.data_as(_szp), C.c_size_t(where.shape[0]), where.ctypes.data_as(_u64p),
                                        _i(ids), _f(codes)))

    def remove_ids(self, ids):
        """IndexIVF::remove_ids with an IDSelectorBatch of `ids`; returns how many entries went"""
        ids = i64(ids)
        n = C.c_size_t(0)
        _chk(lib().amd_ivf_remove_ids(self._h, C.c_size_t(ids.shape[0]), _i(ids), C.byref(n)))
        return n.value

    def last_update(self):
        """(0 none / 1 incremental / 2 full, host-to-device bytes, entries written, blocks re-encoded) of the last refresh"""
        out = (C.c_uint64 * 4)()
        _chk(lib().amd_ivf_last_update(self._h, out))
        return tuple(int(v) for v in out)

    def layout_digest(self):
        """digests of the device layout: offsets, rows, ids, byte fragments, fp16 copy, fp32 copy, lane copy, flags"""
        out = (C.c_uint64 * 8)()
        _chk(lib().amd_ivf_layout_digest(self._h, out))
        return tuple(int(v) for v in out)

    # ---- a subset cut on the device (include/auncel_amd.h: amd_ivf_subset)
    def subset(self, kind, a1=0, a2=0, sel=None):
        """a read-only Handle over the members of every list, in order: SUBSET_ID_RANGE a1 <= id < a2, SUBSET_ID_MOD id % a1 == a2,
        SUBSET_SLICE entries [a1, a2) of the running count, SUBSET_ID_BITS sel = uint64 words (bit id set), SUBSET_ID_BATCH sel = ids"""
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.uint64 if kind == SUBSET_ID_BITS else np.int64)
        c = Handle.__new__(Handle)
        c.d, c.nlist, c.metric, c.device = self.d, self.nlist, self.metric, self.device
        c._h = C.c_void_p()
        if hasattr(self, "max_topk"):
            c.max_topk = self.max_topk
        _chk(lib().amd_ivf_subset(self._h, int(kind), C.c_int64(int(a1)), C.c_int64(int(a2)), sel.ctypes.data_as(C.c_void_p) if sel is not None else None,
                                  C.c_size_t(0 if sel is None else sel.shape[0]), C.byref(c._h)))
        return c

    def last_subset(self):
        """(entries looked at, entries kept, host-to-device bytes, device-to-host bytes) of the call that made this subset"""
        out = (C.c_uint64 * 4)()
        _chk(lib().amd_ivf_last_subset(self._h, out))
        return tuple(int(v) for v in out)

    # ---- resident indexes joined on the device (include/auncel_amd.h: amd_ivf_concat)
    @staticmethod
    def concat(parts):
        """a read-only Handle whose list l is, over `parts` in order, a run of each part's list l.  A part is a Handle (taken whole,
        ids unchanged) or a tuple (handle, begin, end, id_add): begin / end are nlist entry numbers each or None (0 / the list's
        size), id_add (optional) is added to every id taken.  The centroids, the Auncel state and the options are parts[0]'s."""
        parts = [p if isinstance(p, (tuple, list)) else (p,) for p in parts]
        arr = (Part * max(len(parts), 1))()
        keep = []  # (the run tables, as long as the call reads them)
        for a, p in zip(arr, parts):
            h, begin, end, id_add = (tuple(p) + (None, None, 0))[:4]
            a.h = h._h.value if h is not None else None
            for name, run in (("begin", begin), ("end", end)):
                if run is not None:
                    run = np.ascontiguousarray(run, dtype=np.uint64)
                    if h is not None and run.shape != (h.nlist,):
                        raise ValueError("a run table has one entry per list")
                    keep.append(run)
                    setattr(a, name, run.ctypes.data_as(_u64p))
            a.id_add = int(id_add or 0)
        first = parts[0][0] if parts else None
        c = Handle.__new__(Handle)
        c._h = C.c_void_p()
        _chk(lib().amd_ivf_concat(arr if parts else None, C.c_size_t(len(parts)), C.byref(c._h)))
        c.d, c.nlist, c.metric, c.device = first.d, first.nlist, first.metric, first.device
        if hasattr(first, "max_topk"):
            c.max_topk = first.max_topk
        return c

    def last_concat(self):
        """(entries taken, parts, host-to-device bytes, device-to-host bytes) of the call that made this joined index"""
        out = (C.c_uint64 * 4)()
        _chk(lib().amd_ivf_last_concat(self._h, out))
        return tuple(int(v) for v in out)

    # ---- search under an id selector (include/auncel_amd.h: amd_ivf_selector_create)
    def selector(self, kind, a1=0, a2=0, sel=None):
        """a Selector over this index's lists as they are now: the arguments of subset()"""
        return Selector(self, kind, a1, a2, sel)

    def search_selected(self, selector, x, k, nprobe, coarse_mode=0):
        x = f32(x)
        n = x.shape[0]
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_selected(self._h, selector._s, C.c_size_t(n), _f(x), C.c_size_t(k), C.c_size_t(nprobe), coarse_mode, _f(D), _i(I)))
        return D, I

    def search_preassigned_selected(self, selector, x, k, keys, coarse_dis=None):
        x, keys = f32(x), i64(keys)
        n, nprobe = keys.shape
        cd = f32(coarse_dis) if coarse_dis is not None else None
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_preassigned_selected(self._h, selector._s, C.c_size_t(n), _f(x), C.c_size_t(k), C.c_size_t(nprobe), _i(keys),
                                                       _f(cd), _f(D), _i(I)))
        return D, I

    def search_resident_selected(self, selector, start, n, k, nprobe, coarse_mode=0):
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_resident_selected(self._h, selector._s, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k), C.c_size_t(nprobe),
                                                    coarse_mode, _f(D), _i(I)))
        return D, I

    # ---- ... with a selector per query: a list of Selector objects of this index and, per query, the position of its selector in it
    @staticmethod
    def _each(sels, sel_of, n):
        """the table (an array of amd_ivf_selector_t*) and sel_of as uint32: one entry per query, as the ABI reads them"""
        table = (C.c_void_p * max(len(sels), 1))(*[s._s.value if s is not None else None for s in sels])
        sel_of = np.asarray(sel_of)
        if sel_of.shape != (n,):
            raise ValueError(f"sel_of wants one selector number per query: shape {sel_of.shape}, {n} queries")
        if n and (sel_of.min() < 0 or sel_of.max() > 0xffffffff):
            raise ValueError("sel_of holds a number that is not a uint32")
        sel_of = np.ascontiguousarray(sel_of, dtype=np.uint32)
        return table, C.c_size_t(len(sels)), sel_of, sel_of.ctypes.data_as(C.POINTER(C.c_uint32))

    def search_selected_each(self, sels, sel_of, x, k, nprobe, coarse_mode=0):
        """search_selected with a selector per query: row i is searched under sels[sel_of[i]] (amd_ivf_search_selected_each)"""
        x = f32(x)
        n = x.shape[0]
        table, nsel, sel_of, so = self._each(sels, sel_of, n)
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_selected_each(self._h, table, nsel, so, C.c_size_t(n), _f(x), C.c_size_t(k), C.c_size_t(nprobe), coarse_mode,
                                                _f(D), _i(I)))
        return D, I

    def search_preassigned_selected_each(self, sels, sel_of, x, k, keys, coarse_dis=None):
        x, keys = f32(x), i64(keys)
        n, nprobe = keys.shape
        table, nsel, sel_of, so = self._each(sels, sel_of, n)
        cd = f32(coarse_dis) if coarse_dis is not None else None
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_preassigned_selected_each(self._h, table, nsel, so, C.c_size_t(n), _f(x), C.c_size_t(k), C.c_size_t(nprobe),
                                                            _i(keys), _f(cd), _f(D), _i(I)))
        return D, I

    def search_resident_selected_each(self, sels, sel_of, start, n, k, nprobe, coarse_mode=0):
        table, nsel, sel_of, so = self._each(sels, sel_of, n)
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_resident_selected_each(self._h, table, nsel, so, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k),
                                                         C.c_size_t(nprobe), coarse_mode, _f(D), _i(I)))
        return D, I

    # ---- the adaptive rule and its training branch under a selector (include/auncel_amd.h: amd_ivf_search_adaptive_selected & co)
    def _adaptive_args(self, n, require_acc, my_nprobe, t_recalls, gt_D):
        assert my_nprobe.dtype == np.uint64 and t_recalls.dtype == np.float32
        K = self.max_topk
        return f32(require_acc), (f32(gt_D) if gt_D is not None else None), np.empty((n, K), np.float32), np.empty((n, K), np.int64)

    def search_adaptive_selected(self, selector, start, n, query_topk, multipler, std_m, require_acc, my_nprobe, t_recalls, gt_D=None,
                                 profile=0, coarse_mode=0):
        """search_adaptive over the selector's members: the bits of the same call on subset(the same selector)"""
        req, gt, D, I = self._adaptive_args(n, require_acc, my_nprobe, t_recalls, gt_D)
        _chk(lib().amd_ivf_search_adaptive_selected(self._h, selector._s, C.c_size_t(start), C.c_size_t(n), C.c_size_t(query_topk),
                                                    C.c_float(multipler), C.c_float(std_m), _f(req), _f(gt), int(profile), coarse_mode,
                                                    my_nprobe.ctypes.data_as(_u64p), _f(t_recalls), _f(D), _i(I)))
        return D, I

    def search_adaptive_x_selected(self, selector, x, id_offset, query_topk, multipler, std_m, require_acc, my_nprobe, t_recalls,
                                   gt_D=None, profile=0, coarse_mode=0):
        """... over the caller's query rows: row qi is query id_offset + qi of every per-query array"""
        x = f32(x)
        n = x.shape[0]
        req, gt, D, I = self._adaptive_args(n, require_acc, my_nprobe, t_recalls, gt_D)
        _chk(lib().amd_ivf_search_adaptive_x_selected(self._h, selector._s, C.c_size_t(n), _f(x), C.c_size_t(id_offset),
                                                      C.c_size_t(query_topk), C.c_float(multipler), C.c_float(std_m), _f(req), _f(gt),
                                                      int(profile), coarse_mode, my_nprobe.ctypes.data_as(_u64p), _f(t_recalls), _f(D),
                                                      _i(I)))
        return D, I

    def search_adaptive_selected_each(self, sels, sel_of, start, n, query_topk, multipler, std_m, require_acc, my_nprobe, t_recalls,
                                      gt_D=None, profile=0, coarse_mode=0):
        """... with a selector per query: resident query start + i is searched under sels[sel_of[i]]"""
        table, nsel, sel_of, so = self._each(sels, sel_of, n)
        req, gt, D, I = self._adaptive_args(n, require_acc, my_nprobe, t_recalls, gt_D)
        _chk(lib().amd_ivf_search_adaptive_selected_each(self._h, table, nsel, so, C.c_size_t(start), C.c_size_t(n), C.c_size_t(query_topk),
                                                         C.c_float(multipler), C.c_float(std_m), _f(req), _f(gt), int(profile),
                                                         coarse_mode, my_nprobe.ctypes.data_as(_u64p), _f(t_recalls), _f(D), _i(I)))
        return D, I

    def train_samples_selected(self, selector, start, n, max_topk, gt_D, train_num, raw, coarse_mode=0):
        """train_samples over the selector's members (gt_D: the filtered ground truth)"""
        gt = f32(gt_D)
        D = np.empty((n, max_topk), np.float32)
        I = np.empty((n, max_topk), np.int64)
        ptrs = (_f32p * len(raw))(*[_f(r) for r in raw])
        _chk(lib().amd_ivf_train_samples_selected(self._h, selector._s, C.c_size_t(start), C.c_size_t(n), C.c_size_t(max_topk), _f(gt),
                                                  C.c_size_t(train_num), coarse_mode, ptrs, _f(D), _i(I)))
        return D, I

    def range_search_selected(self, selector, x, radius, nprobe, keys=None, coarse_mode=0):
        """range_search over the selector's members -> lims (n + 1), labels, distances"""
        x = f32(x)
        n = x.shape[0]
        lims = np.zeros(n + 1, dtype=np.uintp)
        lp = lims.ctypes.data_as(_szp)
        if keys is None:
            _chk(lib().amd_ivf_range_search_selected(self._h, selector._s, C.c_size_t(n), _f(x), C.c_float(radius), C.c_size_t(nprobe),
                                                     coarse_mode, lp))
        else:
            keys = i64(keys)
            assert keys.shape == (n, nprobe)
            _chk(lib().amd_ivf_range_search_preassigned_selected(self._h, selector._s, C.c_size_t(n), _f(x), C.c_float(radius),
                                                                 C.c_size_t(nprobe), _i(keys), lp))
        tot = int(lims[n])
        labels = np.empty(max(tot, 1), np.int64)
        dist = np.empty(max(tot, 1), np.float32)
        _chk(lib().amd_ivf_range_results(self._h, _i(labels), _f(dist)))
        return lims.astype(np.int64), labels[:tot], dist[:tot]

    def submit_search_resident_selected(self, selector, start, n, k, nprobe, coarse_mode=0, out=None):
        """asynchronous search_resident_selected: returns a ticket for wait(); the selector cannot be closed before it"""
        if out is not None:
            D, I = out
        else:
            D = np.empty((n, k), np.float32)
            I = np.empty((n, k), np.int64)
        t = C.c_uint64(0)
        _chk(lib().amd_ivf_submit_search_resident_selected(self._h, selector._s, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k),
                                                           C.c_size_t(nprobe), coarse_mode, _f(D), _i(I), C.byref(t)))
        if not hasattr(self, "_tickets"):
            self._tickets = {}
        self._tickets[int(t.value)] = (selector, None, None, None, D, I)
        return int(t.value)

    # ---- search
    def coarse(self, x, nprobe, mode=0):
        x = f32(x)
        n = x.shape[0]
        D = np.empty((n, nprobe), np.float32)
        I = np.empty((n, nprobe), np.int64)
        _chk(lib().amd_ivf_coarse(self._h, C.c_size_t(n), _f(x), C.c_size_t(nprobe), _f(D), _i(I), mode))
        return D, I

    def search_preassigned(self, x, k, keys, coarse_dis=None, store_pairs=False, max_codes=0):
        x, keys = f32(x), i64(keys)
        n, nprobe = keys.shape
        cd = f32(coarse_dis) if coarse_dis is not None else None
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_preassigned(self._h, C.c_size_t(n), _f(x), C.c_size_t(k), C.c_size_t(nprobe), _i(keys),
                                              _f(cd), _f(D), _i(I), int(store_pairs), C.c_size_t(max_codes)))
        return D, I

    def search(self, x, k, nprobe, coarse_mode=0):
        x = f32(x)
        n = x.shape[0]
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search(self._h, C.c_size_t(n), _f(x), C.c_size_t(k), C.c_size_t(nprobe), coarse_mode, _f(D), _i(I)))
        return D, I

    # ---- stored vectors back (include/auncel_amd.h: amd_ivf_make_direct_map ...)
    def make_direct_map(self, enable=True):
        """the reference's direct_map on the device: one pass over the resident ids; EngineError -2 when an id lies outside [0, ntotal)"""
        _chk(lib().amd_ivf_make_direct_map(self._h, int(bool(enable))))

    def direct_map_info(self):
        """[alive, ids mapped, ids of [0, ntotal) without an entry, passes made]"""
        out = (C.c_uint64 * 4)()
        _chk(lib().amd_ivf_direct_map_info(self._h, out))
        return [int(v) for v in out]

    def reconstruct(self, ids, out=None):
        """IndexIVF::reconstruct for a batch of ids (needs make_direct_map): the stored rows, len(ids) x d.  out: filled in place"""
        ids = i64(ids).reshape(-1)
        rec = np.empty((ids.shape[0], self.d), np.float32) if out is None else out
        assert rec.dtype == np.float32 and rec.flags.c_contiguous and rec.size == ids.shape[0] * self.d
        _chk(lib().amd_ivf_reconstruct(self._h, C.c_size_t(ids.shape[0]), _i(ids), _f(rec)))
        return rec

    def reconstruct_n(self, i0, ni, out=None, want_found=True):
        """IndexIVF::reconstruct_n over the id window [i0, i0 + ni): (recons, found); slots whose id is not stored keep what `out`
        held (zeros without `out`) and have found 0"""
        rec = np.zeros((max(ni, 0), self.d), np.float32) if out is None else out
        assert rec.dtype == np.float32 and rec.flags.c_contiguous and rec.size == max(ni, 0) * self.d
        found = np.zeros(max(ni, 0), np.uint8) if want_found else None
        fp = found.ctypes.data_as(C.POINTER(C.c_uint8)) if found is not None else None
        _chk(lib().amd_ivf_reconstruct_n(self._h, C.c_int64(i0), C.c_int64(ni), _f(rec), fp))
        return rec, found

    def reconstruct_from_offsets(self, labels, want_ids=True, out=None, out_ids=None):
        """rows (and stored ids) of position labels list << 32 | offset, as a store_pairs search returns them; -1: 0xFF bytes, id -1"""
        labels = i64(labels).reshape(-1)
        n = labels.shape[0]
        rec = np.empty((n, self.d), np.float32) if out is None else out
        ids = (np.empty(n, np.int64) if out_ids is None else out_ids) if want_ids else None
        _chk(lib().amd_ivf_reconstruct_from_offsets(self._h, C.c_size_t(n), _i(labels), _f(rec), _i(ids)))
        return rec, ids

    def search_and_reconstruct(self, x, k, nprobe, coarse_mode=0, out=None):
        """search() plus the stored row of every admitted entry: (D, I, recons n x k x d).  out = (D, I, recons) to fill (e.g.
        page-locked arrays: recons is then written by the gather itself)"""
        x = f32(x)
        n = x.shape[0]
        D, I, R = out if out is not None else (np.empty((n, k), np.float32), np.empty((n, k), np.int64), np.empty((n, k, self.d), np.float32))
        _chk(lib().amd_ivf_search_and_reconstruct(self._h, C.c_size_t(n), _f(x), C.c_size_t(k), C.c_size_t(nprobe), coarse_mode, _f(D), _i(I),
                                                  _f(R)))
        return D, I, R

    def search_and_reconstruct_resident(self, start, n, k, nprobe, coarse_mode=0, out=None):
        D, I, R = out if out is not None else (np.empty((n, k), np.float32), np.empty((n, k), np.int64), np.empty((n, k, self.d), np.float32))
        _chk(lib().amd_ivf_search_and_reconstruct_resident(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k), C.c_size_t(nprobe),
                                                           coarse_mode, _f(D), _i(I), _f(R)))
        return D, I, R

    def search_exact(self, x, k):
        """exact top-k over every list (include/auncel_amd.h: amd_ivf_search_exact): search_preassigned with identity keys, bit for bit"""
        x = f32(x)
        n = x.shape[0]
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_exact(self._h, C.c_size_t(n), _f(x), C.c_size_t(k), _f(D), _i(I)))
        return D, I

    def search_exact_resident(self, start, n, k):
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_exact_resident(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k), _f(D), _i(I)))
        return D, I

    def search_exact_selected(self, selector, x, k):
        """search_exact over the selector's members only (include/auncel_amd.h: amd_ivf_search_exact_selected): search_exact of
        subset(the same selector), bit for bit, without the second index"""
        x = f32(x)
        n = x.shape[0]
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_exact_selected(self._h, selector._s, C.c_size_t(n), _f(x), C.c_size_t(k), _f(D), _i(I)))
        return D, I

    def search_exact_resident_selected(self, selector, start, n, k):
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_exact_resident_selected(self._h, selector._s, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k), _f(D), _i(I)))
        return D, I

    def last_exact(self):
        """(queries answered by the list pass, searched the general way because equal distances met, ... for any other reason,
        candidates the list pass emitted) of the last exact call"""
        out = (C.c_uint64 * 4)()
        _chk(lib().amd_ivf_last_exact(self._h, out))
        return tuple(int(v) for v in out)

    def last_exact_detail(self):
        """(which list pass the last exact call ran: 0 none, 1 bytes, 2 fp16 + rescoring, 3 wide fp16 + rescoring (option
        "exact_wide"), 4 wide bytes (option "exact_wide_bytes"); candidates emitted; candidates at or within the threshold after
        rescoring; the largest emitted count of one query)"""
        out = (C.c_uint64 * 4)()
        _chk(lib().amd_ivf_last_exact_detail(self._h, out))
        return tuple(int(v) for v in out)

    def _range_results(self, lims):
        n = len(lims) - 1
        tot = int(lims[n])
        labels = np.empty(max(tot, 1), np.int64)
        dist = np.empty(max(tot, 1), np.float32)
        _chk(lib().amd_ivf_range_results(self._h, _i(labels), _f(dist)))
        return lims.astype(np.int64), labels[:tot], dist[:tot]

    def range_search_exact(self, x, radius):
        """every entry within the radius, over every list (include/auncel_amd.h: amd_ivf_range_search_exact): range_search with
        nprobe = nlist and identity keys, bit for bit -> lims (n + 1), labels, distances"""
        x = f32(x)
        n = x.shape[0]
        lims = np.zeros(n + 1, dtype=np.uintp)
        _chk(lib().amd_ivf_range_search_exact(self._h, C.c_size_t(n), _f(x), C.c_float(radius), lims.ctypes.data_as(_szp)))
        return self._range_results(lims)

    def range_search_exact_resident(self, start, n, radius):
        lims = np.zeros(n + 1, dtype=np.uintp)
        _chk(lib().amd_ivf_range_search_exact_resident(self._h, C.c_size_t(start), C.c_size_t(n), C.c_float(radius), lims.ctypes.data_as(_szp)))
        return self._range_results(lims)

    def range_search_exact_selected(self, selector, x, radius):
        """range_search_exact over the selector's members only"""
        x = f32(x)
        n = x.shape[0]
        lims = np.zeros(n + 1, dtype=np.uintp)
        _chk(lib().amd_ivf_range_search_exact_selected(self._h, selector._s, C.c_size_t(n), _f(x), C.c_float(radius), lims.ctypes.data_as(_szp)))
        return self._range_results(lims)

    def last_range_exact(self):
        """(which list pass the last exact range call ran: 0 none, 1 bytes, 2 fp16 + rescoring, 3 wide fp16 + rescoring, 4 wide bytes; queries
        answered from the pass; queries searched the general way; the largest emitted candidate count of one query)"""
        out = (C.c_uint64 * 4)()
        _chk(lib().amd_ivf_last_range_exact(self._h, out))
        return tuple(int(v) for v in out)

    def range_search(self, x, radius, nprobe, keys=None, coarse_mode=0):
        """IndexIVF::range_search(_preassigned) -> lims (n + 1), labels, distances"""
        x = f32(x)
        n = x.shape[0]
        lims = np.zeros(n + 1, dtype=np.uintp)
        lp = lims.ctypes.data_as(_szp)
        if keys is None:
            _chk(lib().amd_ivf_range_search(self._h, C.c_size_t(n), _f(x), C.c_float(radius), C.c_size_t(nprobe), coarse_mode, lp))
        else:
            keys = i64(keys)
            assert keys.shape == (n, nprobe)
            _chk(lib().amd_ivf_range_search_preassigned(self._h, C.c_size_t(n), _f(x), C.c_float(radius), C.c_size_t(nprobe), _i(keys), lp))
        tot = int(lims[n])
        labels = np.empty(max(tot, 1), np.int64)
        dist = np.empty(max(tot, 1), np.float32)
        _chk(lib().amd_ivf_range_results(self._h, _i(labels), _f(dist)))
        return lims.astype(np.int64), labels[:tot], dist[:tot]

    def scan_codes(self, query, list_no, simi, idxi, store_pairs=False):
        query = f32(query)
        nup = C.c_size_t(0)
        _chk(lib().amd_ivf_scan_codes(self._h, _f(query), C.c_size_t(list_no), int(store_pairs), C.c_size_t(simi.shape[0]),
                                      _f(simi), _i(idxi), C.byref(nup)))
        return nup.value

    def scan_codes_at(self, query, list_no, offset, n, simi, idxi, store_pairs=False):
        """InvertedListScanner::scan_codes over vectors [offset, offset + n) of the list"""
        query = f32(query)
        nup = C.c_size_t(0)
        _chk(lib().amd_ivf_scan_codes_at(self._h, _f(query), C.c_size_t(list_no), C.c_size_t(offset), C.c_size_t(n), int(store_pairs),
                                         C.c_size_t(simi.shape[0]), _f(simi), _i(idxi), C.byref(nup)))
        return nup.value

    def scan_codes_range(self, query, list_no, offset, n, radius):
        """InvertedListScanner::scan_codes_range over the same kind of run: (positions counted from offset, distances), in order"""
        query = f32(query)
        cnt = C.c_size_t(0)
        _chk(lib().amd_ivf_scan_codes_range(self._h, _f(query), C.c_size_t(list_no), C.c_size_t(offset), C.c_size_t(n), C.c_float(radius),
                                            C.byref(cnt)))
        pos = np.empty(cnt.value, np.uint32)
        dis = np.empty(cnt.value, np.float32)
        if cnt.value:
            _chk(lib().amd_ivf_scan_codes_range_results(self._h, pos.ctypes.data_as(C.POINTER(C.c_uint32)), _f(dis)))
        return pos, dis

    def distance_to_code(self, query, list_no, offset):
        query = f32(query)
        out = C.c_float(0)
        _chk(lib().amd_ivf_distance_to_code(self._h, _f(query), C.c_size_t(list_no), C.c_size_t(offset), C.byref(out)))
        return np.float32(out.value)

    def stats(self, reset=False):
        st = (C.c_size_t * 4)()
        _chk(lib().amd_ivf_stats(self._h, st, int(reset)))
        return dict(nq=st[0], nlist=st[1], ndis=st[2], nheap_updates=st[3])

    def set_queries(self, x):
        x = f32(x)
        _chk(lib().amd_ivf_set_queries(self._h, C.c_size_t(x.shape[0]), _f(x)))

    def search_resident(self, start, n, k, nprobe, coarse_mode=0):
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_resident(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k), C.c_size_t(nprobe),
                                           coarse_mode, _f(D), _i(I)))
        return D, I

    # ---- from and into device memory: torch tensors on the handle's device (include/auncel_amd.h: the `_dev` calls)
    def _dev_rows(self, x):
        """(pointer, dtype, ldx) of a [n, d] fp32 / fp16 tensor whose columns are contiguous; rows may be strided (a column slice)"""
        import torch
        if not (x.is_cuda and x.device.index == self.device):
            raise ValueError("x must be a tensor on the handle's device")
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"x must be [n, {self.d}]")
        if x.dtype not in (torch.float32, torch.float16):
            raise ValueError("x must be float32 or float16")
        if x.shape[1] > 1 and x.stride(1) != 1:
            raise ValueError("the columns of x must be contiguous (x.stride(1) == 1)")
        ldx = x.stride(0) if x.shape[0] > 1 else max(x.stride(0), self.d)  # (the stride of a single row means nothing)
        return C.c_void_p(x.data_ptr()), 0 if x.dtype == torch.float32 else 1, C.c_size_t(ldx)

    def _dev_out(self, n, k, out):
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            return torch.empty((n, k), dtype=torch.float32, device=dev), torch.empty((n, k), dtype=torch.int64, device=dev)
        D, I = out
        if not (D.shape == (n, k) and D.dtype == torch.float32 and D.is_contiguous() and D.device == dev):
            raise ValueError(f"out[0] must be a contiguous float32 [{n}, {k}] tensor on the handle's device")
        if not (I.shape == (n, k) and I.dtype == torch.int64 and I.is_contiguous() and I.device == dev):
            raise ValueError(f"out[1] must be a contiguous int64 [{n}, {k}] tensor on the handle's device")
        return D, I

    def _dev_stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_queries_dev(self, x):
        p, dtype, ldx = self._dev_rows(x)
        _chk(lib().amd_ivf_set_queries_dev(self._h, C.c_size_t(x.shape[0]), p, dtype, ldx, self._dev_stream()))

    def search_dev(self, x, k, nprobe, coarse_mode=0, out=None):
        """search() for a query tensor on the GPU; (D, I) are GPU tensors (out: the tensors to fill).  Ordered behind the current
        torch stream; the results may be read from any stream on return."""
        p, dtype, ldx = self._dev_rows(x)
        n = x.shape[0]
        D, I = self._dev_out(n, k, out)
        _chk(lib().amd_ivf_search_dev(self._h, C.c_size_t(n), p, dtype, ldx, C.c_size_t(k), C.c_size_t(nprobe), coarse_mode,
                                      C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr()), self._dev_stream()))
        return D, I

    def search_preassigned_dev(self, x, k, keys, out=None):
        """keys: an int64 [n, nprobe] tensor on the handle's device"""
        import torch
        p, dtype, ldx = self._dev_rows(x)
        n = x.shape[0]
        if not (keys.dtype == torch.int64 and keys.dim() == 2 and keys.shape[0] == n and keys.is_contiguous() and keys.is_cuda
                and keys.device.index == self.device):
            raise ValueError("keys must be a contiguous int64 [n, nprobe] tensor on the handle's device")
        D, I = self._dev_out(n, k, out)
        _chk(lib().amd_ivf_search_preassigned_dev(self._h, C.c_size_t(n), p, dtype, ldx, C.c_size_t(k), C.c_size_t(keys.shape[1]),
                                                  C.c_void_p(keys.data_ptr()), C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr()),
                                                  self._dev_stream()))
        return D, I

    def search_resident_dev(self, start, n, k, nprobe, coarse_mode=0, out=None):
        import torch
        D, I = self._dev_out(n, k, out)
        if out is not None:
            torch.cuda.current_stream(self.device).synchronize()  # (the call takes no stream: whatever still uses `out` ends first)
        _chk(lib().amd_ivf_search_resident_dev(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k), C.c_size_t(nprobe), coarse_mode,
                                               C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr())))
        return D, I

    def search_exact_dev(self, x, k, out=None):
        p, dtype, ldx = self._dev_rows(x)
        n = x.shape[0]
        D, I = self._dev_out(n, k, out)
        _chk(lib().amd_ivf_search_exact_dev(self._h, C.c_size_t(n), p, dtype, ldx, C.c_size_t(k), C.c_void_p(D.data_ptr()),
                                            C.c_void_p(I.data_ptr()), self._dev_stream()))
        return D, I

    def search_adaptive_dev(self, start, n, query_topk, multipler, std_m, require_acc, my_nprobe, t_recalls, gt_D=None, profile=False,
                            coarse_mode=0, out=None):
        """search_adaptive() with (D, I) as GPU tensors; require_acc, my_nprobe, t_recalls and gt_D stay numpy arrays"""
        import torch
        req = f32(require_acc)
        gt = f32(gt_D) if gt_D is not None else None
        assert my_nprobe.dtype == np.uint64 and t_recalls.dtype == np.float32
        D, I = self._dev_out(n, self.max_topk, out)
        if out is not None:
            torch.cuda.current_stream(self.device).synchronize()
        _chk(lib().amd_ivf_search_adaptive_dev(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(query_topk), C.c_float(multipler),
                                               C.c_float(std_m), _f(req), _f(gt), int(profile), coarse_mode,
                                               my_nprobe.ctypes.data_as(_u64p), _f(t_recalls), C.c_void_p(D.data_ptr()),
                                               C.c_void_p(I.data_ptr())))
        return D, I

    def last_dev_io(self):
        """[query-row bytes host -> device, (D, I) bytes across the bus, ingest launches, 1 kernels stored the results / 2 a device
        copy did] of the handle's last `_dev` call"""
        out = (C.c_uint64 * 4)()
        _chk(lib().amd_ivf_last_dev_io(self._h, out))
        return [int(v) for v in out]

    # ---- Auncel
    def set_interdis(self, table=None):
        t = f32(table) if table is not None else None
        _chk(lib().amd_ivf_set_interdis(self._h, _f(t)))

    def get_interdis(self):
        t = np.empty(self.nlist * (self.nlist - 1) // 2, np.float32)
        _chk(lib().amd_ivf_get_interdis(self._h, _f(t)))
        return t

    def set_tuner(self, max_topk, traces, arcos):
        """traces: list of (x, y, std)"""
        n = len(traces)
        lens = np.array([len(t[0]) for t in traces], dtype=np.uintp)
        xs, ys, ss = [f32(t[0]) for t in traces], [f32(t[1]) for t in traces], [f32(t[2]) for t in traces]
        arcos = f32(arcos)
        _chk(lib().amd_ivf_set_tuner(self._h, C.c_size_t(max_topk), C.c_size_t(n), lens.ctypes.data_as(_szp),
                                     (_f32p * n)(*[_f(a) for a in xs]), (_f32p * n)(*[_f(a) for a in ys]),
                                     (_f32p * n)(*[_f(a) for a in ss]), _f(arcos)))
        self.max_topk = max_topk

    def search_adaptive(self, start, n, query_topk, multipler, std_m, require_acc, my_nprobe, t_recalls, gt_D=None,
                        profile=False, coarse_mode=0, out=None):
        """out: optional (D, I) arrays to fill -- a caller that hands over page-locked memory gets its results by direct DMA"""
        req = f32(require_acc)
        gt = f32(gt_D) if gt_D is not None else None
        assert my_nprobe.dtype == np.uint64 and t_recalls.dtype == np.float32
        K = self.max_topk
        if out is not None:
            D, I = out
            assert D.shape == (n, K) and D.dtype == np.float32 and D.flags.c_contiguous
            assert I.shape == (n, K) and I.dtype == np.int64 and I.flags.c_contiguous
        else:
            D = np.empty((n, K), np.float32)
            I = np.empty((n, K), np.int64)
        _chk(lib().amd_ivf_search_adaptive(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(query_topk),
                                           C.c_float(multipler), C.c_float(std_m), _f(req), _f(gt), int(profile), coarse_mode,
                                           my_nprobe.ctypes.data_as(_u64p), _f(t_recalls), _f(D), _i(I)))
        return D, I

    def set_async_depth(self, depth):
        """searches amd_ivf_submit_adaptive keeps running at a time (internal contexts; fixed by the first submit)"""
        _chk(lib().amd_ivf_set_async_depth(self._h, int(depth)))

    def submit_adaptive(self, start, n, query_topk, multipler, std_m, require_acc, my_nprobe, t_recalls, gt_D=None, profile=False,
                        coarse_mode=0, out=None):
        """asynchronous search_adaptive: returns a ticket for wait(); every array passed stays referenced until then"""
        req = f32(require_acc)
        gt = f32(gt_D) if gt_D is not None else None
        assert my_nprobe.dtype == np.uint64 and t_recalls.dtype == np.float32
        K = self.max_topk
        if out is not None:
            D, I = out
            assert D.shape == (n, K) and D.dtype == np.float32 and D.flags.c_contiguous
            assert I.shape == (n, K) and I.dtype == np.int64 and I.flags.c_contiguous
        else:
            D = np.empty((n, K), np.float32)
            I = np.empty((n, K), np.int64)
        t = C.c_uint64(0)
        _chk(lib().amd_ivf_submit_adaptive(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(query_topk), C.c_float(multipler),
                                           C.c_float(std_m), _f(req), _f(gt), int(profile), coarse_mode,
                                           my_nprobe.ctypes.data_as(_u64p), _f(t_recalls), _f(D), _i(I), C.byref(t)))
        if not hasattr(self, "_tickets"):
            self._tickets = {}
        self._tickets[int(t.value)] = (req, gt, my_nprobe, t_recalls, D, I)
        return int(t.value)

    def submit_search_resident(self, start, n, k, nprobe, coarse_mode=0, out=None):
        """asynchronous search_resident: returns a ticket for wait()"""
        if out is not None:
            D, I = out
        else:
            D = np.empty((n, k), np.float32)
            I = np.empty((n, k), np.int64)
        t = C.c_uint64(0)
        _chk(lib().amd_ivf_submit_search_resident(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k), C.c_size_t(nprobe), coarse_mode,
                                                  _f(D), _i(I), C.byref(t)))
        if not hasattr(self, "_tickets"):
            self._tickets = {}
        self._tickets[int(t.value)] = (None, None, None, None, D, I)
        return int(t.value)

    def submit_coarse_resident(self, start, n, nprobe, mode=0, want_dis=False):
        """asynchronous coarse_resident: wait() returns (coarse_dis or None, keys) in place of (D, I)"""
        keys = np.empty((n, nprobe), np.int64)
        dis = np.empty((n, nprobe), np.float32) if want_dis else None
        t = C.c_uint64(0)
        _chk(lib().amd_ivf_submit_coarse_resident(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(nprobe), _f(dis), _i(keys), mode,
                                                  C.byref(t)))
        if not hasattr(self, "_tickets"):
            self._tickets = {}
        self._tickets[int(t.value)] = (None, None, None, None, dis, keys)
        return int(t.value)

    def submit_search_resident_preassigned(self, start, n, k, keys, out=None):
        """asynchronous search_resident_preassigned (keys: n x nprobe, kept alive until wait())"""
        keys = i64(keys)
        assert keys.shape[0] == n
        if out is not None:
            D, I = out
        else:
            D = np.empty((n, k), np.float32)
            I = np.empty((n, k), np.int64)
        t = C.c_uint64(0)
        _chk(lib().amd_ivf_submit_search_resident_preassigned(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k), C.c_size_t(keys.shape[1]),
                                                              _i(keys), _f(D), _i(I), C.byref(t)))
        if not hasattr(self, "_tickets"):
            self._tickets = {}
        self._tickets[int(t.value)] = (keys, None, None, None, D, I)
        return int(t.value)

    def async_counts(self):
        """(tickets served by the asynchronous entry points, passes that served them)"""
        out = (C.c_uint64 * 2)()
        _chk(lib().amd_ivf_async_counts(self._h, out))
        return int(out[0]), int(out[1])

    def wait(self, ticket):
        """blocks until the search of `ticket` has ended; returns (D, I, timing dict, diag dict); raises as the synchronous call"""
        tm = (C.c_double * 9)()
        dg = (C.c_uint64 * 4)()
        rc = lib().amd_ivf_wait(self._h, C.c_uint64(ticket), tm, dg)
        held = self._tickets.pop(ticket, None) if hasattr(self, "_tickets") else None
        _chk(rc)
        keys = ("coarse_ms", "scan_ms", "select_ms", "total_ms", "scan_launches", "scan_bytes", "slot_efficiency", "rounds", "scan_min_bytes")
        timing = {k: float(tm[i]) for i, k in enumerate(keys)}
        diag = {"hinted_launches": int(dg[0]), "short_hints": int(dg[1]), "tie_redone": int(dg[2]), "direct_out": bool(dg[3])}
        D, I = (held[4], held[5]) if held else (None, None)
        return D, I, timing, diag

    def search_adaptive_pre(self, x, id_offset, keys, coarse_dis, query_topk, multipler, std_m, require_acc, my_nprobe, t_recalls,
                            gt_D=None, profile=False):
        """search_preassigned with tune on over the caller's coarse ranking (keys / coarse_dis rows, nprobe entries each)"""
        x, keys, cd = f32(x), i64(keys), f32(coarse_dis)
        n, nprobe = keys.shape
        req = f32(require_acc)
        gt = f32(gt_D) if gt_D is not None else None
        assert my_nprobe.dtype == np.uint64 and t_recalls.dtype == np.float32
        K = self.max_topk
        D = np.empty((n, K), np.float32)
        I = np.empty((n, K), np.int64)
        _chk(lib().amd_ivf_search_adaptive_pre(self._h, C.c_size_t(n), _f(x), C.c_size_t(id_offset), C.c_size_t(nprobe), _i(keys), _f(cd),
                                               C.c_size_t(query_topk), C.c_float(multipler), C.c_float(std_m), _f(req), _f(gt),
                                               int(profile), my_nprobe.ctypes.data_as(_u64p), _f(t_recalls), _f(D), _i(I)))
        return D, I

    def train_samples_pre(self, x, id_offset, keys, coarse_dis, max_topk, gt_D, train_num, raw):
        """the training branch over the caller's coarse ranking"""
        x, keys, cd, gt = f32(x), i64(keys), f32(coarse_dis), f32(gt_D)
        n, nprobe = keys.shape
        D = np.empty((n, max_topk), np.float32)
        I = np.empty((n, max_topk), np.int64)
        ptrs = (_f32p * len(raw))(*[_f(r) for r in raw])
        _chk(lib().amd_ivf_train_samples_pre(self._h, C.c_size_t(n), _f(x), C.c_size_t(id_offset), C.c_size_t(nprobe), _i(keys), _f(cd),
                                             C.c_size_t(max_topk), _f(gt), C.c_size_t(train_num), ptrs, _f(D), _i(I)))
        return D, I

    def search_timed(self, start, n, k, nprobe, budget_ms, coarse_mode=0):
        """Error_sys::time_search over resident queries [start, start+n); budget_ms is indexed by absolute query id.
        Returns (D, I, nprobe_used)."""
        b = f32(budget_ms)
        assert b.size >= start + n
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        used = np.zeros(n, np.uint64)
        _chk(lib().amd_ivf_search_timed(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k), C.c_size_t(nprobe), _f(b), coarse_mode,
                                        used.ctypes.data_as(_u64p), _f(D), _i(I)))
        return D, I, used

    def search_timed_x(self, x, id_offset, k, nprobe, budget_ms, coarse_mode=0):
        x = f32(x)
        n = x.shape[0]
        b = f32(budget_ms)
        assert b.size >= id_offset + n
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        used = np.zeros(n, np.uint64)
        _chk(lib().amd_ivf_search_timed_x(self._h, C.c_size_t(n), _f(x), C.c_size_t(id_offset), C.c_size_t(k), C.c_size_t(nprobe), _f(b),
                                          coarse_mode, used.ctypes.data_as(_u64p), _f(D), _i(I)))
        return D, I, used

    def train_samples(self, start, n, max_topk, gt_D, train_num, raw, coarse_mode=0):
        gt = f32(gt_D)
        D = np.empty((n, max_topk), np.float32)
        I = np.empty((n, max_topk), np.int64)
        ptrs = (_f32p * len(raw))(*[_f(r) for r in raw])
        _chk(lib().amd_ivf_train_samples(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(max_topk), _f(gt),
                                         C.c_size_t(train_num), coarse_mode, ptrs, _f(D), _i(I)))
        return D, I

    def train_samples_x(self, x, id_offset, max_topk, gt_D, train_num, raw, coarse_mode=0):
        """train_samples over the caller's query rows: row qi is query id_offset + qi of gt_D and of raw"""
        x, gt = f32(x), f32(gt_D)
        n = x.shape[0]
        D = np.empty((n, max_topk), np.float32)
        I = np.empty((n, max_topk), np.int64)
        ptrs = (_f32p * len(raw))(*[_f(r) for r in raw])
        _chk(lib().amd_ivf_train_samples_x(self._h, C.c_size_t(n), _f(x), C.c_size_t(id_offset), C.c_size_t(max_topk), _f(gt),
                                           C.c_size_t(train_num), coarse_mode, ptrs, _f(D), _i(I)))
        return D, I

    def scan_arith(self):
        """0 fp32 reference order, 1 fp32 fused, 2 byte codes (include/auncel_amd.h)"""
        return int(lib().amd_ivf_scan_arith(self._h))

    def last_timing(self):
        t = (C.c_double * 8)()
        lib().amd_ivf_last_timing(self._h, t)
        mb = C.c_double(0)
        lib().amd_ivf_last_scan_min_bytes(self._h, C.byref(mb))
        return dict(coarse_ms=t[0], scan_ms=t[1], select_ms=t[2], total_ms=t[3], scan_launches=t[4], scan_bytes=t[5],
                    slot_efficiency=t[6], rounds=t[7], scan_min_bytes=mb.value)

    PHASES = ("coarse", "scan_dense", "select_dense", "scan_thr", "select_thr", "tie_fix", "plan")

    def last_timing_detail(self):
        """{phase: (ms, launches)} of the last search on this handle (include/auncel_amd.h: amd_ivf_last_timing_detail)"""
        t = (C.c_double * 16)()
        lib().amd_ivf_last_timing_detail(self._h, t)
        d = {p: (t[2 * i], t[2 * i + 1]) for i, p in enumerate(self.PHASES)}
        d["min_bytes_dense"], d["min_bytes_thr"] = t[14], t[15]
        return d

    def coarse_tie_rows(self):
        """coarse rankings re-run through the reference's heap so far (runs of equal distances, include/auncel_amd.h)"""
        v = C.c_uint64(0)
        _chk(lib().amd_ivf_coarse_tie_rows(self._h, C.byref(v)))
        return int(v.value)

    def coarse_resident(self, start, n, nprobe, mode=0, want_dis=True):
        """the coarse ranking of resident queries [start, start + n) -> (coarse_dis or None, keys)"""
        keys = np.empty((n, nprobe), np.int64)
        dis = np.empty((n, nprobe), np.float32) if want_dis else None
        _chk(lib().amd_ivf_coarse_resident(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(nprobe), _f(dis), _i(keys), mode))
        return dis, keys

    def search_resident_preassigned(self, start, n, k, keys, out=None):
        """search_preassigned over resident queries [start, start + n) with the caller's keys (n x nprobe)"""
        keys = i64(keys)
        assert keys.shape[0] == n
        if out is not None:
            D, I = out
        else:
            D = np.empty((n, k), np.float32)
            I = np.empty((n, k), np.int64)
        _chk(lib().amd_ivf_search_resident_preassigned(self._h, C.c_size_t(start), C.c_size_t(n), C.c_size_t(k), C.c_size_t(keys.shape[1]),
                                                       _i(keys), _f(D), _i(I)))
        return D, I

    def last_round_hints(self):
        """(scan launches of the last search sized from the previous search's counts, those whose hint was too small)"""
        v = (C.c_uint64 * 2)()
        _chk(lib().amd_ivf_last_round_hints(self._h, v))
        return int(v[0]), int(v[1])

    def last_tie_redone(self):
        """queries the last adaptive call searched again with the reference's coarse tie order (AUNCEL_AMD_COARSE_TIES=redo)"""
        v = C.c_uint64(0)
        _chk(lib().amd_ivf_last_tie_redone(self._h, C.byref(v)))
        return int(v.value)

    def last_tie_patched(self):
        """rankings of the last adaptive call whose order the reference's heap changed while its one pass was under way"""
        v = C.c_uint64(0)
        _chk(lib().amd_ivf_last_tie_patched(self._h, C.byref(v)))
        return int(v.value)

    def last_tie_fixed(self):
        """queries of the last search whose result came from the heap replayed over their admission log (include/auncel_amd.h)"""
        v = C.c_uint64(0)
        _chk(lib().amd_ivf_last_tie_fixed(self._h, C.byref(v)))
        return int(v.value)

    def last_filter(self):
        """(threshold rounds of the last search that ran as matrix-core filter + exact recomputation, candidates the last one kept)"""
        v = (C.c_uint64 * 2)()
        _chk(lib().amd_ivf_last_filter(self._h, v))
        return int(v[0]), int(v[1])

    def last_direct_out(self):
        """True if the last search wrote (D, I) straight into the caller's (page-locked) buffers (include/auncel_amd.h)"""
        return bool(lib().amd_ivf_last_direct_out(self._h))

    def last_coarse_pick(self):
        """rankings of the last coarse call that came from matrix-core distances + exact recomputation (include/auncel_amd.h)"""
        v = C.c_uint64(0)
        _chk(lib().amd_ivf_last_coarse_pick(self._h, C.byref(v)))
        return int(v.value)

    def set_byte_codes(self, enable):
        """False: scan the fp32 lists even where the byte codes qualify (same results)"""
        lib().amd_ivf_set_byte_codes(self._h, int(bool(enable)))

    def set_option(self, key, value):
        """include/auncel_amd.h: amd_ivf_set_option (None returns the key to "unset")"""
        _chk(lib().amd_ivf_set_option(self._h, key.encode(), C.c_double(float("nan") if value is None else float(value))))

    def get_option(self, key):
        v = C.c_double(0)
        _chk(lib().amd_ivf_get_option(self._h, key.encode(), C.byref(v)))
        return v.value
