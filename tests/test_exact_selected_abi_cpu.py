"""CPU-side checks of the exact search under an id selector (include/auncel_amd.h: amd_ivf_search_exact_selected,
amd_ivf_search_exact_resident_selected): the two entry points are exported, declared in the header and bound, and they refuse a
missing handle, selector or result pointer, k = 0 and a resident range that wraps round before anything touches a device.  The
host-only part -- the mask of a block's live slots that the block table writes and the list pass reads, the seed's nprobe under a
selector, the argument checks -- runs as a program of its own (tests/cpp/exact_selected_main.cpp), built with the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_search_exact_selected", "amd_ivf_search_exact_resident_selected"]


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
        assert re.search(r"^int %s\(amd_ivf_t\* h, const amd_ivf_selector_t\* s, " % s, header, re.M), s
    for m in ("search_exact_selected", "search_exact_resident_selected"):
        assert callable(getattr(capi.Handle, m))
    mirror = open(os.path.join(ROOT, "auncel_amd", "csrc", "host", "IndexIVFFlat.h")).read()
    assert re.search(r"void search_exact_selected\(idx_t n, const float\* x, idx_t k, float\* distances, idx_t\* labels, const IDSelector& sel\) const;", mirror)


def test_refuse_bad_arguments_before_the_device(capi):
    L = capi.lib()
    D, I = (C.c_float * 8)(), (C.c_int64 * 8)()
    x = (C.c_float * 64)()
    z, one, two = C.c_size_t(0), C.c_size_t(1), C.c_size_t(2)
    some = C.c_void_p(64)  # (never followed: another argument is refused first)
    big = C.c_size_t(2 ** 64 - 1)

    def refused(rc, word):
        assert rc == -2
        assert word in L.amd_ivf_last_error(), L.amd_ivf_last_error()

    refused(L.amd_ivf_search_exact_selected(some, None, two, x, two, D, I), b"null selector")
    refused(L.amd_ivf_search_exact_selected(some, None, z, None, two, None, None), b"null selector")
    refused(L.amd_ivf_search_exact_selected(None, some, two, x, two, D, I), b"null handle")
    refused(L.amd_ivf_search_exact_selected(None, None, two, x, two, D, I), b"null")
    refused(L.amd_ivf_search_exact_selected(some, some, two, None, two, D, I), b"null")
    refused(L.amd_ivf_search_exact_selected(some, some, two, x, two, None, I), b"null")
    refused(L.amd_ivf_search_exact_selected(some, some, two, x, two, D, None), b"null")
    refused(L.amd_ivf_search_exact_selected(some, some, two, x, z, D, I), b"k must be positive")
    refused(L.amd_ivf_search_exact_resident_selected(some, None, z, two, two, D, I), b"null selector")
    refused(L.amd_ivf_search_exact_resident_selected(None, some, z, two, two, D, I), b"null handle")
    refused(L.amd_ivf_search_exact_resident_selected(some, some, z, two, two, None, I), b"null")
    refused(L.amd_ivf_search_exact_resident_selected(some, some, z, two, two, D, None), b"null")
    refused(L.amd_ivf_search_exact_resident_selected(some, some, z, two, z, D, I), b"k must be positive")
    refused(L.amd_ivf_search_exact_resident_selected(some, some, big, two, one, D, I), b"range")


def test_the_host_part_as_a_program_under_the_sanitizers(tmp_path):
    """exact_args.h's valid mask against a bit-by-bit loop (left 0, 1, 31, 32, 40, ...; keep halves of 0, all ones, random), the
    seed rule and the new argument checks, as the stand-alone program built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "exact_selected_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "exact_selected_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().strip().endswith("DONE"), p.stdout.decode()
