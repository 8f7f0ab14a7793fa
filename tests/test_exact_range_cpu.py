"""CPU-side checks of the exact range search's entry points (include/auncel_amd.h: amd_ivf_range_search_exact, _resident, _selected,
amd_ivf_last_range_exact): they are exported, declared in the header and bound, and they refuse a missing handle, lims, query rows
or selector and a resident range that wraps round before anything touches a device; with valid arguments and no device they fail
with -4 before the handle is read.  The host-only part -- the argument checks, the threshold the byte list pass is given for a
radius (NaN, +-inf, +-1e30, the kernel's guard), the strict range test and the candidates' sort key -- runs as a program of its own
(tests/cpp/exact_range_main.cpp, which is also what the address and undefined-behaviour sanitizers are pointed at)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_range_search_exact", "amd_ivf_range_search_exact_resident", "amd_ivf_range_search_exact_selected", "amd_ivf_last_range_exact"]


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
    for m in ("range_search_exact", "range_search_exact_resident", "range_search_exact_selected", "last_range_exact"):
        assert callable(getattr(capi.Handle, m))
    mirror = open(os.path.join(ROOT, "auncel_amd", "csrc", "host", "IndexIVFFlat.h")).read()
    for m in ("range_search_exact(", "range_search_exact_selected(", "range_exact_info("):
        assert m in mirror, m


def test_refuse_bad_arguments_before_the_device(capi):
    L = capi.lib()
    lims = (C.c_size_t * 8)()
    x = (C.c_float * 64)()
    out4 = (C.c_uint64 * 4)()
    z, two = C.c_size_t(0), C.c_size_t(2)
    r = C.c_float(1.0)
    some = C.c_void_p(64)  # (never followed: another argument is refused first)
    big = C.c_size_t(2 ** 64 - 1)

    def refused(rc, word):
        assert rc == -2
        assert word in L.amd_ivf_last_error(), L.amd_ivf_last_error()

    refused(L.amd_ivf_range_search_exact(None, two, x, r, lims), b"null handle")
    refused(L.amd_ivf_range_search_exact(some, two, x, r, None), b"null lims")
    refused(L.amd_ivf_range_search_exact(some, z, None, r, None), b"null lims")
    refused(L.amd_ivf_range_search_exact(some, two, None, r, lims), b"null")
    refused(L.amd_ivf_range_search_exact_resident(None, z, two, r, lims), b"null handle")
    refused(L.amd_ivf_range_search_exact_resident(some, z, two, r, None), b"null lims")
    refused(L.amd_ivf_range_search_exact_resident(some, big, two, r, lims), b"out of bounds")
    refused(L.amd_ivf_range_search_exact_selected(some, None, two, x, r, lims), b"null selector")
    refused(L.amd_ivf_range_search_exact_selected(some, None, z, None, r, None), b"null selector")
    refused(L.amd_ivf_range_search_exact_selected(None, some, two, x, r, lims), b"null handle")
    refused(L.amd_ivf_range_search_exact_selected(some, some, two, x, r, None), b"null lims")
    refused(L.amd_ivf_range_search_exact_selected(some, some, two, None, r, lims), b"null")
    refused(L.amd_ivf_last_range_exact(None, out4), b"null")
    refused(L.amd_ivf_last_range_exact(some, None), b"null")


def test_no_cpu_fallback(capi):
    """valid arguments, no device: -4 before the handle is read (a machine with a GPU would follow the pointer: skipped there)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = capi.lib()
    lims = (C.c_size_t * 8)()
    x = (C.c_float * 64)()
    out4 = (C.c_uint64 * 4)()
    two = C.c_size_t(2)
    some = C.c_void_p(64)
    assert L.amd_ivf_range_search_exact(some, two, x, C.c_float(1.0), lims) == -4
    assert L.amd_ivf_range_search_exact(some, C.c_size_t(0), None, C.c_float(1.0), lims) == -4
    assert L.amd_ivf_range_search_exact_resident(some, C.c_size_t(0), two, C.c_float(1.0), lims) == -4
    assert L.amd_ivf_last_range_exact(some, out4) == -4


def test_the_host_part_as_a_program(tmp_path):
    """exact_args.h's range part -- NaN maps to none; +-inf and +-1e30 map to finite thresholds of the right side for both metrics; a
    threshold inside the range comes back unchanged; every threshold passes the kernel's guard |t| <= 2^30 -- as the stand-alone
    program; its header says how to build it with -fsanitize=address,undefined"""
    exe = str(tmp_path / "exact_range_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", os.path.join(ROOT, "tests", "cpp", "exact_range_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().strip().endswith("DONE"), p.stdout.decode()
