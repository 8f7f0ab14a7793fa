"""CPU-side checks of the entry points that search one batch under a selector per query (include/auncel_amd.h:
amd_ivf_search_selected_each, amd_ivf_search_preassigned_selected_each, amd_ivf_search_resident_selected_each): they are exported,
declared in the header and bound, and they refuse a missing handle, table, index array or result pointer before anything touches a
device.  The host-only part -- the checks of the table and of sel_of, the resident range -- runs as a program of its own
(tests/cpp/selector_each_main.cpp, which is also what the address and undefined-behaviour sanitizers are pointed at)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_search_selected_each", "amd_ivf_search_preassigned_selected_each", "amd_ivf_search_resident_selected_each"]


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
    for m in ("search_selected_each", "search_preassigned_selected_each", "search_resident_selected_each"):
        assert callable(getattr(capi.Handle, m))


def test_refuse_without_a_handle_a_table_an_index_array_or_a_result(capi):
    L = capi.lib()
    z, one = C.c_size_t(0), C.c_size_t(1)
    some = C.c_void_p(64)  # (never followed: another argument is missing)

    def refused(rc):
        assert rc == -2
        assert b"null" in L.amd_ivf_last_error()

    # (h, sels, sel_of, D, I) with one or more of them missing, with and without queries
    full = [some] * 5
    for missing in ([0], [1], [2], [3], [4], [0, 1], [3, 4], [0, 1, 2, 3, 4]):
        h, sels, sel_of, D, I = [None if i in missing else p for i, p in enumerate(full)]
        for n in (z, one):
            refused(L.amd_ivf_search_selected_each(h, sels, one, sel_of, n, some, one, one, 0, D, I))
            refused(L.amd_ivf_search_preassigned_selected_each(h, sels, one, sel_of, n, some, one, one, some, None, D, I))
            refused(L.amd_ivf_search_resident_selected_each(h, sels, one, sel_of, z, n, one, one, 0, D, I))
    # null queries with n > 0 (behind the pointers above: still nothing is followed)
    refused(L.amd_ivf_search_selected_each(some, some, one, some, one, None, one, one, 0, some, some))
    refused(L.amd_ivf_search_preassigned_selected_each(some, some, one, some, one, None, one, one, some, None, some, some))
    # no selectors for some queries
    for rc in (L.amd_ivf_search_selected_each(some, some, z, some, one, some, one, one, 0, some, some),
               L.amd_ivf_search_preassigned_selected_each(some, some, z, some, one, some, one, one, some, None, some, some),
               L.amd_ivf_search_resident_selected_each(some, some, z, some, z, one, one, one, 0, some, some)):
        assert rc == -2 and b"nsel == 0" in L.amd_ivf_last_error()


def test_the_host_part_as_a_program(tmp_path):
    """selector_args.h's checks of a call under a selector per query (null, foreign and stale entries by position, an index out of
    range by query, a resident range that wraps) as the stand-alone program; its header says how to build it with
    -fsanitize=address,undefined"""
    exe = str(tmp_path / "selector_each_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", os.path.join(ROOT, "tests", "cpp", "selector_each_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().strip().endswith("DONE"), p.stdout.decode()
