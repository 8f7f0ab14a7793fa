"""CPU-side checks of the exact search's entry points (include/auncel_amd.h: amd_ivf_search_exact, amd_ivf_search_exact_resident,
amd_ivf_last_exact): they are exported, declared in the header and bound, the option that goes with them is documented, and they
refuse a missing handle or result pointer, k = 0 and a resident range that wraps round before anything touches a device; with valid
arguments and no device they fail with -4 before the handle is read.  The host-only part -- the argument checks and the tie rule over
a query's sorted candidates -- runs as a program of its own (tests/cpp/exact_args_main.cpp, which is also what the address and
undefined-behaviour sanitizers are pointed at)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_search_exact", "amd_ivf_search_exact_resident", "amd_ivf_last_exact"]


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
    for m in ("search_exact", "search_exact_resident", "last_exact"):
        assert callable(getattr(capi.Handle, m))
    assert '"exact_seed_nprobe"' in header[header.index(" *   key "):header.index("amd_ivf_set_option(h, key, NAN)")]
    assert "ivf_exact.hip" in __import__("auncel_amd.build", fromlist=["SOURCES"]).SOURCES


def test_refuse_bad_arguments_before_the_device(capi):
    L = capi.lib()
    D, I = (C.c_float * 8)(), (C.c_int64 * 8)()
    x = (C.c_float * 64)()
    out4 = (C.c_uint64 * 4)()
    z, one, two = C.c_size_t(0), C.c_size_t(1), C.c_size_t(2)
    some = C.c_void_p(64)  # (never followed: another argument is refused first)
    big = C.c_size_t(2 ** 64 - 1)

    def refused(rc, word):
        assert rc == -2
        assert word in L.amd_ivf_last_error(), L.amd_ivf_last_error()

    refused(L.amd_ivf_search_exact(None, two, x, two, D, I), b"null")
    refused(L.amd_ivf_search_exact(some, two, None, two, D, I), b"null")
    refused(L.amd_ivf_search_exact(some, two, x, two, None, I), b"null")
    refused(L.amd_ivf_search_exact(some, two, x, two, D, None), b"null")
    refused(L.amd_ivf_search_exact(some, two, x, z, D, I), b"k must be positive")
    refused(L.amd_ivf_search_exact(some, z, None, z, None, None), b"k must be positive")
    refused(L.amd_ivf_search_exact_resident(None, z, two, two, D, I), b"null")
    refused(L.amd_ivf_search_exact_resident(some, z, two, two, None, I), b"null")
    refused(L.amd_ivf_search_exact_resident(some, z, two, two, D, None), b"null")
    refused(L.amd_ivf_search_exact_resident(some, z, two, z, D, I), b"k must be positive")
    refused(L.amd_ivf_search_exact_resident(some, big, two, one, D, I), b"range")
    refused(L.amd_ivf_last_exact(None, out4), b"null")
    refused(L.amd_ivf_last_exact(some, None), b"null")


def test_no_cpu_fallback(capi):
    """valid arguments, no device: -4 before the handle is read (a machine with a GPU would follow the pointer: skipped there)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = capi.lib()
    D, I = (C.c_float * 8)(), (C.c_int64 * 8)()
    x = (C.c_float * 64)()
    out4 = (C.c_uint64 * 4)()
    two = C.c_size_t(2)
    some = C.c_void_p(64)
    assert L.amd_ivf_search_exact(some, two, x, two, D, I) == -4
    assert L.amd_ivf_search_exact_resident(some, C.c_size_t(0), two, two, D, I) == -4
    assert L.amd_ivf_last_exact(some, out4) == -4


def test_the_host_part_as_a_program(tmp_path):
    """exact_args.h's argument checks and the tie rule -- a tie at positions 0, k - 2, k - 1 and k, fewer than k + 1 entries, exactly k,
    k = 1 -- as the stand-alone program; its header says how to build it with -fsanitize=address,undefined"""
    exe = str(tmp_path / "exact_args_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", os.path.join(ROOT, "tests", "cpp", "exact_args_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().strip().endswith("DONE"), p.stdout.decode()
