"""CPU-side checks of the subset entry points (include/auncel_amd.h: amd_ivf_subset, amd_ivf_last_subset): they are exported and
bound, the subset kinds are named in the header, and they refuse a missing handle before anything touches a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_subset", "amd_ivf_last_subset"]
KINDS = {"AMD_IVF_SUBSET_ID_RANGE": 0, "AMD_IVF_SUBSET_ID_MOD": 1, "AMD_IVF_SUBSET_SLICE": 2, "AMD_IVF_SUBSET_ID_BITS": 5,
         "AMD_IVF_SUBSET_ID_BATCH": 6}


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import build, capi
    build.build()
    return capi


def test_new_entry_points_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert hasattr(L, s) and s in capi.SYMBOLS
    for m in ("subset", "last_subset"):
        assert callable(getattr(capi.Handle, m))


def test_subset_kinds_are_in_the_header(capi):
    hdr = open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    for name, value in KINDS.items():
        m = re.search(r"#define\s+%s\s+(\d+)\b" % name, hdr)
        assert m and int(m.group(1)) == value, name
        assert getattr(capi, name[len("AMD_IVF_"):]) == value


def test_refuse_without_a_handle(capi):
    L = capi.lib()
    out = C.c_void_p()
    out4 = (C.c_uint64 * 4)()
    assert L.amd_ivf_subset(None, 0, C.c_int64(0), C.c_int64(10), None, C.c_size_t(0), C.byref(out)) == -2
    assert b"null" in L.amd_ivf_last_error()
    assert L.amd_ivf_last_subset(None, out4) == -2
    assert b"null" in L.amd_ivf_last_error()
