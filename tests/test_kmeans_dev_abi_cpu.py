"""CPU-side checks of amd_ivf_kmeans_dev (include/auncel_amd.h): exported, declared, bound; every refusal of its arguments is -2 with
its message before any device is touched; without a device the answer to valid arguments is -4, never a CPU path."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_LINE = "int amd_ivf_kmeans_dev(int d, size_t n, const void* d_x, int dtype, size_t ldx, size_t k, int metric, int niter, long seed,"
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def L():
    from auncel_amd import capi
    return capi.lib()


def call(L, d=8, n=100, x=64, dtype=0, ldx=8, k=4, max_pts=256, cen=64):
    """(`x` and `cen` are made-up addresses that are never followed: another argument is refused first, or there is no device)"""
    return L.amd_ivf_kmeans_dev(d, C.c_size_t(n), C.c_void_p(x), dtype, C.c_size_t(ldx), C.c_size_t(k), 1, 2, C.c_long(1234),
                                C.c_size_t(max_pts), 0, 0, 0, 0, C.c_void_p(cen), None, None)


def test_exported_declared_and_bound(L):
    from auncel_amd import build, capi
    assert HEADER_LINE in open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    assert hasattr(L, "amd_ivf_kmeans_dev") and "amd_ivf_kmeans_dev" in capi.SYMBOLS and L.amd_ivf_kmeans_dev.restype is C.c_int
    assert callable(capi.kmeans_dev) and "ivf_kmeans_dev.hip" in build.SOURCES


@pytest.mark.parametrize("args,message", [
    (dict(x=None), b"null"),
    (dict(cen=None), b"null"),
    (dict(d=0), b"bad dimension"),
    (dict(k=0), b"bad dimension"),
    (dict(n=3), b"at least as large as number of clusters"),
    (dict(n=INT_MAX + 1), b"int permutation"),
    (dict(max_pts=0), b"max_points_per_centroid must be positive"),
    (dict(dtype=2), b"dtype must be 0 (fp32) or 1 (fp16)"),
    (dict(dtype=-1), b"dtype must be 0 (fp32) or 1 (fp16)"),
    (dict(ldx=7), b"ldx must be at least d"),
])
def test_refusals(L, args, message):
    assert call(L, **args) == -2 and message in L.amd_ivf_last_error(), L.amd_ivf_last_error()


def test_no_cpu_fallback(L):
    """valid arguments, no device: -4 (a machine with a GPU would look the pointers up: skipped there)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert call(L) == -4
