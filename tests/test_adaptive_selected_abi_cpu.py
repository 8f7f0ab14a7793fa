"""CPU-side checks of the entry points that run the adaptive rule and its training branch under an id selector
(include/auncel_amd.h: amd_ivf_search_adaptive_selected, amd_ivf_search_adaptive_x_selected, amd_ivf_search_adaptive_selected_each,
amd_ivf_train_samples_selected): they are exported, declared in the header and bound, and they refuse a missing argument, an empty
table and the overhead profile before anything touches a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_search_adaptive_selected", "amd_ivf_search_adaptive_x_selected", "amd_ivf_search_adaptive_selected_each",
       "amd_ivf_train_samples_selected"]


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import build, capi
    build.build()
    return capi


def test_new_entry_points_are_exported_declared_and_bound(capi):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    for s in NEW:
        assert hasattr(L, s) and s in capi.SYMBOLS
        assert getattr(L, s).restype is C.c_int
        assert re.search(r"^int %s\(" % s, header, re.M), s
    for m in ("search_adaptive_selected", "search_adaptive_x_selected", "search_adaptive_selected_each", "train_samples_selected"):
        assert callable(getattr(capi.Handle, m))
    assert "selected_skip_empty" in header


def test_refuse_every_missing_argument_without_a_device(capi):
    L = capi.lib()
    z, one = C.c_size_t(0), C.c_size_t(1)
    f1 = C.c_float(1.0)
    some = C.c_void_p(64)  # (never followed: another argument is missing)

    def refused(rc, word=b"null"):
        assert rc == -2
        assert word in L.amd_ivf_last_error()

    # one selector: (h, s, require_acc, my_nprobe, t_recalls, D, I); gt_D may be null
    for missing in ([0], [1], [2], [3], [4], [5], [6], [0, 1], [5, 6], list(range(7))):
        h, s, req, np_, tr, D, I = [None if i in missing else some for i in range(7)]
        for n in (z, one):
            refused(L.amd_ivf_search_adaptive_selected(h, s, z, n, one, f1, f1, req, None, 0, 0, np_, tr, D, I))
            refused(L.amd_ivf_search_adaptive_x_selected(h, s, n, some, z, one, f1, f1, req, None, 0, 0, np_, tr, D, I))
    refused(L.amd_ivf_search_adaptive_x_selected(some, some, one, None, z, one, f1, f1, some, None, 0, 0, some, some, some, some))
    # a selector per query: (h, sels, sel_of, require_acc, my_nprobe, t_recalls, D, I)
    for missing in ([0], [1], [2], [3], [4], [5], [6], [7], [0, 1], [6, 7], list(range(8))):
        h, sels, so, req, np_, tr, D, I = [None if i in missing else some for i in range(8)]
        for n in (z, one):
            refused(L.amd_ivf_search_adaptive_selected_each(h, sels, one, so, z, n, one, f1, f1, req, None, 0, 0, np_, tr, D, I))
    # no selectors for some queries
    refused(L.amd_ivf_search_adaptive_selected_each(some, some, z, some, z, one, one, f1, f1, some, None, 0, 0, some, some, some, some),
            b"nsel == 0")
    # the training call: (h, s, gt_D, raw, D, I)
    for missing in ([0], [1], [2], [3], [4], [5], [0, 1], [4, 5], list(range(6))):
        h, s, gt, raw, D, I = [None if i in missing else some for i in range(6)]
        for n in (z, one):
            refused(L.amd_ivf_train_samples_selected(h, s, z, n, C.c_size_t(20), gt, C.c_size_t(8), 0, raw, D, I))
    # profile bit 1 (overhead_profile) is not offered under a selector
    for profile in (2, 3):
        refused(L.amd_ivf_search_adaptive_selected(some, some, z, one, one, f1, f1, some, None, profile, 0, some, some, some, some),
                b"overhead_profile")
        refused(L.amd_ivf_search_adaptive_x_selected(some, some, one, some, z, one, f1, f1, some, None, profile, 0, some, some, some, some),
                b"overhead_profile")
        refused(L.amd_ivf_search_adaptive_selected_each(some, some, one, some, z, one, one, f1, f1, some, None, profile, 0, some, some,
                                                        some, some), b"overhead_profile")
