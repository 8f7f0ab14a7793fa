"""CPU-side checks of amd_ivf_assign / amd_ivf_assign_dev / amd_ivf_last_assign (include/auncel_amd.h): exported, declared, bound;
a null argument is refused with -2 before anything else is looked at; without a device the answer is -4, never a CPU path."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_LINES = (
    "int amd_ivf_assign(amd_ivf_t* h, size_t n, const float* x, int64_t* assign, float* dis);",
    "int amd_ivf_assign_dev(amd_ivf_t* h, size_t n, const void* d_x, int dtype, size_t ldx, int64_t* d_assign, float* d_dis /* may be NULL */, void* stream);",
    "int amd_ivf_last_assign(amd_ivf_t* h, uint64_t out[4]);",
)


@pytest.fixture(scope="module")
def L():
    from auncel_amd import capi
    return capi.lib()


def test_exported_declared_and_bound(L):
    from auncel_amd import build, capi
    header = open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    for line in HEADER_LINES:
        assert line in header, line
        s = line.split("(")[0].split()[-1]
        assert hasattr(L, s) and s in capi.SYMBOLS and getattr(L, s).restype is C.c_int
    assert all(callable(getattr(capi.Handle, m)) for m in ("assign", "assign_dev", "last_assign"))
    assert "ivf_assign.hip" in build.SOURCES


def test_null_arguments_are_refused(L):
    x, a, out4 = (C.c_float * 64)(), (C.c_int64 * 8)(), (C.c_uint64 * 4)()
    two, some = C.c_size_t(2), C.c_void_p(64)  # (`some` is never followed: another argument is refused first)
    for rc in (L.amd_ivf_assign(None, two, x, a, None), L.amd_ivf_assign(some, two, None, a, None), L.amd_ivf_assign(some, two, x, None, None),
               L.amd_ivf_assign_dev(None, two, some, 0, two, some, None, None), L.amd_ivf_assign_dev(some, two, None, 0, two, some, None, None),
               L.amd_ivf_assign_dev(some, two, some, 0, two, None, None, None), L.amd_ivf_last_assign(None, out4),
               L.amd_ivf_last_assign(some, None)):
        assert rc == -2 and b"null" in L.amd_ivf_last_error(), (rc, L.amd_ivf_last_error())


def test_no_cpu_fallback(L):
    """valid arguments, no device: -4 before the handle is read (a machine with a GPU would follow the pointer: skipped there)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x, a, out4 = (C.c_float * 64)(), (C.c_int64 * 8)(), (C.c_uint64 * 4)()
    two, some = C.c_size_t(2), C.c_void_p(64)
    assert L.amd_ivf_assign(some, two, x, a, None) == -4
    assert L.amd_ivf_assign_dev(some, two, some, 0, two, some, None, None) == -4
    assert L.amd_ivf_last_assign(some, out4) == -4
