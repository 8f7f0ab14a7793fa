"""CPU-side checks of the in-place update entry points (include/auncel_amd.h: amd_ivf_update_lists, amd_ivf_remove_ids,
amd_ivf_last_update, amd_ivf_layout_digest): they are exported and bound, the option that selects them is documented, and they
refuse a missing handle or argument before anything touches a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_update_lists", "amd_ivf_remove_ids", "amd_ivf_last_update", "amd_ivf_layout_digest"]


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import build, capi
    build.build()
    return capi


def test_new_entry_points_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert hasattr(L, s) and s in capi.SYMBOLS
    for m in ("update_lists", "remove_ids", "last_update", "layout_digest"):
        assert callable(getattr(capi.Handle, m))


def test_incremental_option_is_documented():
    hdr = open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    assert '"incremental"' in hdr[hdr.index(" *   key "):hdr.index("amd_ivf_set_option(h, key, NAN)")]


def test_refuse_without_a_handle(capi):
    L = capi.lib()
    sizes = (C.c_size_t * 4)(1, 2, 3, 4)
    out4, out8 = (C.c_uint64 * 4)(), (C.c_uint64 * 8)()
    n = C.c_size_t(7)
    ids = (C.c_int64 * 2)(1, 2)
    assert L.amd_ivf_update_lists(None, sizes, C.c_size_t(0), None, None, None) == -2
    assert L.amd_ivf_remove_ids(None, C.c_size_t(2), ids, C.byref(n)) == -2
    assert L.amd_ivf_last_update(None, out4) == -2
    assert L.amd_ivf_layout_digest(None, out8) == -2
    assert b"null" in L.amd_ivf_last_error()
