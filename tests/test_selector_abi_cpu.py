"""CPU-side checks of the selector entry points (include/auncel_amd.h: amd_ivf_selector_create ... amd_ivf_search_resident_selected):
they are exported and bound, and they refuse a missing handle, selector or result pointer before anything touches a device."""
import ctypes as C

import pytest

NEW = ["amd_ivf_selector_create", "amd_ivf_selector_destroy", "amd_ivf_selector_info", "amd_ivf_search_selected",
       "amd_ivf_search_preassigned_selected", "amd_ivf_search_resident_selected"]


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import build, capi
    build.build()
    return capi


def test_new_entry_points_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert hasattr(L, s) and s in capi.SYMBOLS
    for m in ("selector", "search_selected", "search_preassigned_selected", "search_resident_selected"):
        assert callable(getattr(capi.Handle, m))
    for m in ("info", "close", "__enter__", "__exit__"):
        assert callable(getattr(capi.Selector, m))


def test_refuse_without_a_handle_a_selector_or_a_result(capi):
    L = capi.lib()
    out = C.c_void_p()
    out4 = (C.c_uint64 * 4)()
    z, i0 = C.c_size_t(0), C.c_int64(0)
    some = C.c_void_p(64)  # (never followed: the other argument is missing)

    def refused(rc):
        assert rc == -2
        assert b"null" in L.amd_ivf_last_error()

    refused(L.amd_ivf_selector_create(None, 0, i0, C.c_int64(10), None, z, C.byref(out)))
    refused(L.amd_ivf_selector_create(some, 0, i0, C.c_int64(10), None, z, None))
    refused(L.amd_ivf_selector_destroy(None))
    refused(L.amd_ivf_selector_info(None, out4))
    refused(L.amd_ivf_selector_info(some, None))
    for h, s in ((None, some), (some, None), (None, None)):
        refused(L.amd_ivf_search_selected(h, s, z, None, z, z, 0, None, None))
        refused(L.amd_ivf_search_preassigned_selected(h, s, z, None, z, z, None, None, None, None))
        refused(L.amd_ivf_search_resident_selected(h, s, z, z, z, z, 0, None, None))
