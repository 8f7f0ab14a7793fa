"""CPU-side checks of handing stored vectors back (include/auncel_amd.h: amd_ivf_make_direct_map, amd_ivf_direct_map_info,
amd_ivf_reconstruct, _reconstruct_n, _reconstruct_from_offsets, amd_ivf_search_and_reconstruct, _resident): the seven entry points
are exported, declared in the header and bound, the class mirror declares its four, and every call refuses a missing handle, a
missing input or output with work to do, k = 0, a negative or overflowing id window and a resident range that wraps round before
anything touches a device.  The host-only part -- what a position label means against the list sizes, the id window's arithmetic,
the argument checks -- runs as a program of its own (tests/cpp/reconstruct_args_main.cpp), built with the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_make_direct_map", "amd_ivf_direct_map_info", "amd_ivf_reconstruct", "amd_ivf_reconstruct_n",
       "amd_ivf_reconstruct_from_offsets", "amd_ivf_search_and_reconstruct", "amd_ivf_search_and_reconstruct_resident"]


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
        assert re.search(r"^int %s\(amd_ivf_t\* h, " % s, header, re.M), s
    for m in ("make_direct_map", "direct_map_info", "reconstruct", "reconstruct_n", "reconstruct_from_offsets", "search_and_reconstruct",
              "search_and_reconstruct_resident"):
        assert callable(getattr(capi.Handle, m))
    assert "ivf_reconstruct.hip" in __import__("auncel_amd.build", fromlist=["SOURCES"]).SOURCES
    mirror = open(os.path.join(ROOT, "auncel_amd", "csrc", "host", "IndexIVFFlat.h")).read()
    subset = mirror[mirror.index("struct IndexIVFFlatSubset"):]
    for decl in (r"void make_direct_map\(bool new_maintain_direct_map = true\);",
                 r"void reconstruct\(idx_t key, float\* recons\) const override;",
                 r"void reconstruct_n\(idx_t i0, idx_t ni, float\* recons\) const override;",
                 r"void search_and_reconstruct\(idx_t n, const float\* x, idx_t k, float\* distances, idx_t\* labels, float\* recons\) const override;"):
        assert re.search(decl, subset), decl
    # what is deliberately not offered is said where the calls are declared
    section = header[header.index("stored vectors back"):header.index("int amd_ivf_make_direct_map")]
    for word in ("Not offered", "selector", "exact", "adaptive", "tickets"):
        assert word in section, word


def test_refuse_bad_arguments_before_the_device(capi):
    L = capi.lib()
    D, I = (C.c_float * 8)(), (C.c_int64 * 8)()
    R = (C.c_float * 64)()
    x = (C.c_float * 64)()
    ids = (C.c_int64 * 8)()
    info = (C.c_uint64 * 4)()
    found = (C.c_uint8 * 8)()
    z, one, two = C.c_size_t(0), C.c_size_t(1), C.c_size_t(2)
    some = C.c_void_p(64)  # (never followed: another argument is refused first)
    big = C.c_size_t(2 ** 64 - 1)
    i64max = 2 ** 63 - 1
    q = C.c_int64

    def refused(rc, word):
        assert rc == -2
        assert word in L.amd_ivf_last_error(), L.amd_ivf_last_error()

    refused(L.amd_ivf_make_direct_map(None, 1), b"null handle")
    refused(L.amd_ivf_make_direct_map(None, 0), b"null handle")
    refused(L.amd_ivf_direct_map_info(None, info), b"null")
    refused(L.amd_ivf_direct_map_info(some, None), b"null")

    refused(L.amd_ivf_reconstruct(None, two, ids, R), b"null handle")
    refused(L.amd_ivf_reconstruct(some, two, None, R), b"null argument")
    refused(L.amd_ivf_reconstruct(some, two, ids, None), b"null argument")

    refused(L.amd_ivf_reconstruct_n(None, q(0), q(2), R, found), b"null handle")
    refused(L.amd_ivf_reconstruct_n(some, q(0), q(2), None, found), b"null argument")
    refused(L.amd_ivf_reconstruct_n(some, q(0), q(-1), R, found), b"negative")
    refused(L.amd_ivf_reconstruct_n(some, q(5), q(-(2 ** 63)), R, None), b"negative")
    refused(L.amd_ivf_reconstruct_n(some, q(i64max), q(1), R, found), b"overflows")
    refused(L.amd_ivf_reconstruct_n(some, q(1), q(i64max), R, found), b"overflows")

    refused(L.amd_ivf_reconstruct_from_offsets(None, two, ids, R, I), b"null handle")
    refused(L.amd_ivf_reconstruct_from_offsets(some, two, None, R, I), b"null argument")
    refused(L.amd_ivf_reconstruct_from_offsets(some, two, ids, None, I), b"null argument")

    refused(L.amd_ivf_search_and_reconstruct(None, two, x, two, two, 0, D, I, R), b"null handle")
    refused(L.amd_ivf_search_and_reconstruct(some, two, None, two, two, 0, D, I, R), b"null argument")
    refused(L.amd_ivf_search_and_reconstruct(some, two, x, two, two, 0, None, I, R), b"null argument")
    refused(L.amd_ivf_search_and_reconstruct(some, two, x, two, two, 0, D, None, R), b"null argument")
    refused(L.amd_ivf_search_and_reconstruct(some, two, x, two, two, 0, D, I, None), b"null argument")
    refused(L.amd_ivf_search_and_reconstruct(some, two, x, z, two, 0, D, I, R), b"k must be positive")
    refused(L.amd_ivf_search_and_reconstruct(some, z, None, z, two, 0, None, None, None), b"k must be positive")

    refused(L.amd_ivf_search_and_reconstruct_resident(None, z, two, two, two, 0, D, I, R), b"null handle")
    refused(L.amd_ivf_search_and_reconstruct_resident(some, z, two, two, two, 0, None, I, R), b"null argument")
    refused(L.amd_ivf_search_and_reconstruct_resident(some, z, two, two, two, 0, D, None, R), b"null argument")
    refused(L.amd_ivf_search_and_reconstruct_resident(some, z, two, two, two, 0, D, I, None), b"null argument")
    refused(L.amd_ivf_search_and_reconstruct_resident(some, z, two, z, two, 0, D, I, R), b"k must be positive")
    refused(L.amd_ivf_search_and_reconstruct_resident(some, big, two, one, two, 0, D, I, R), b"range")
    # nothing was written on the way
    assert not any(R) and not any(D) and not any(I) and not any(found)


def test_the_host_part_as_a_program_under_the_sanitizers(tmp_path):
    """reconstruct_args.h's label decoding against a brute-force loop (list sizes 0, 1, 31, 32, 33, 65), the window arithmetic at the
    int64 edges and the argument checks, as the stand-alone program built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "reconstruct_args_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "reconstruct_args_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().strip().endswith("DONE"), p.stdout.decode()
