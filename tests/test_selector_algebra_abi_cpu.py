"""CPU-side checks of the selector algebra's entry points (include/auncel_amd.h: amd_ivf_selector_combine, amd_ivf_range_search_selected,
amd_ivf_range_search_preassigned_selected, amd_ivf_submit_search_resident_selected): they are exported, declared in the header and
bound, and they refuse a missing handle, selector or result pointer before anything touches a device.  The host-only part of the
combine -- the operand checks and the rule that says which bits of a keep word stand for entries -- runs as a program of its own
(tests/cpp/selector_combine_main.cpp, which is also what the address and undefined-behaviour sanitizers are pointed at)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_selector_combine", "amd_ivf_range_search_selected", "amd_ivf_range_search_preassigned_selected",
       "amd_ivf_submit_search_resident_selected"]


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
    for name, value in (("AND", 0), ("OR", 1), ("ANDNOT", 2), ("NOT", 3)):
        assert re.search(r"^#define AMD_IVF_SELECTOR_%s %d\b" % (name, value), header, re.M), name
        assert getattr(capi, "SELECTOR_" + name) == value
    for m in ("range_search_selected", "submit_search_resident_selected"):
        assert callable(getattr(capi.Handle, m))
    for m in ("combine", "destroy", "__and__", "__or__", "__sub__", "__invert__"):
        assert callable(getattr(capi.Selector, m))


def test_refuse_without_a_handle_a_selector_or_a_result(capi):
    L = capi.lib()
    out = C.c_void_p()
    t = C.c_uint64(77)
    z = C.c_size_t(0)
    r = C.c_float(1.0)
    some = C.c_void_p(64)  # (never followed: the other argument is missing)

    def refused(rc):
        assert rc == -2
        assert b"null" in L.amd_ivf_last_error()

    for op in (0, 1, 2, 3, 9):
        refused(L.amd_ivf_selector_combine(op, None, some, C.byref(out)))
        refused(L.amd_ivf_selector_combine(op, None, None, C.byref(out)))
        refused(L.amd_ivf_selector_combine(op, some, some, None))
        refused(L.amd_ivf_selector_combine(op, some, None, None))
    assert not out.value
    lims = (C.c_size_t * 1)()
    for h, s in ((None, some), (some, None), (None, None)):
        refused(L.amd_ivf_range_search_selected(h, s, z, None, r, C.c_size_t(1), 0, lims))
        refused(L.amd_ivf_range_search_preassigned_selected(h, s, z, None, r, C.c_size_t(1), None, lims))
        refused(L.amd_ivf_submit_search_resident_selected(h, s, z, z, z, z, 0, None, None, C.byref(t)))
    assert t.value == 77, "a ticket was issued"


def test_the_host_part_of_the_combine_as_a_program(tmp_path):
    """selector_args.h's combine checks and selector_valid_word (list lengths 0, 1, 63, 64, 65, 127, 128 and 70, whose block count is
    odd) as the stand-alone program; its header says how to build it with -fsanitize=address,undefined"""
    exe = str(tmp_path / "selector_combine_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", os.path.join(ROOT, "tests", "cpp", "selector_combine_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().strip().endswith("DONE"), p.stdout.decode()
