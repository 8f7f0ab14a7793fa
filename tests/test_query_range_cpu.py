"""CPU-side checks of the `_dev` entry points (include/auncel_amd.h: amd_ivf_set_queries_dev, amd_ivf_search_dev & co): the seven
entry points are exported, declared in the header and bound, the class mirror declares search_dev twice, and a missing handle is
refused.  The host-compilable half of the feature -- query_range.h's element rule and the merge of partial ranges against a literal
restatement of IntRange::add, dev_io_args.h's refusals -- runs as a program of its own (tests/cpp/query_range_main.cpp), built with
the address and undefined-behaviour sanitizers and run directly."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_set_queries_dev", "amd_ivf_search_dev", "amd_ivf_search_preassigned_dev", "amd_ivf_search_resident_dev",
       "amd_ivf_search_exact_dev", "amd_ivf_search_adaptive_dev", "amd_ivf_last_dev_io"]


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import build, capi
    build.build()
    return capi


def test_dev_entry_points_are_exported_declared_and_bound(capi):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    for s in NEW:
        assert hasattr(L, s) and s in capi.SYMBOLS
        assert getattr(L, s).restype is C.c_int
        assert re.search(r"^int %s\(amd_ivf_t\* h, " % s, header, re.M), s
    for m in ("set_queries_dev", "search_dev", "search_preassigned_dev", "search_resident_dev", "search_exact_dev", "search_adaptive_dev",
              "last_dev_io"):
        assert callable(getattr(capi.Handle, m))
    sources = __import__("auncel_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "ivf_ingest.hip" in sources
    mirror = open(os.path.join(ROOT, "auncel_amd", "csrc", "host", "IndexIVFFlat.h")).read()
    decl = r"void search_dev\(idx_t n, const float\* d_x, idx_t k, float\* d_D, idx_t\* d_I, void\* stream = nullptr\) const;"
    subset = mirror.index("struct IndexIVFFlatSubset")
    assert re.search(decl, mirror[:subset]) and re.search(decl, mirror[subset:])
    # the element rule lives once: the engine's kernel file and the stand-alone program read the same header
    kernel = open(os.path.join(ROOT, "auncel_amd", "csrc", "ivf_ingest.hip")).read()
    assert "query_range_add" in kernel and "truncf" not in kernel and "4095" not in kernel


def test_a_missing_handle_is_refused(capi):
    L = capi.lib()
    z, two = C.c_size_t(0), C.c_size_t(2)
    some = C.c_void_p(64)  # (never followed: the handle is refused first)
    out = (C.c_uint64 * 4)()

    def refused(rc):
        assert rc == -2
        assert b"null handle" in L.amd_ivf_last_error() or b"null argument" in L.amd_ivf_last_error(), L.amd_ivf_last_error()

    refused(L.amd_ivf_set_queries_dev(None, two, some, 0, two, None))
    refused(L.amd_ivf_search_dev(None, two, some, 0, two, two, two, 0, some, some, None))
    refused(L.amd_ivf_search_preassigned_dev(None, two, some, 0, two, two, two, some, some, some, None))
    refused(L.amd_ivf_search_resident_dev(None, z, two, two, two, 0, some, some))
    refused(L.amd_ivf_search_exact_dev(None, two, some, 0, two, two, some, some, None))
    refused(L.amd_ivf_search_adaptive_dev(None, z, two, two, C.c_float(1), C.c_float(1), None, None, 0, 0, None, None, some, some))
    refused(L.amd_ivf_last_dev_io(None, out))


def test_the_host_part_as_a_program_under_the_sanitizers(tmp_path):
    """query_range.h against IntRange::add restated word for word -- random arrays, every edge value of the arithmetic choice at
    every block boundary, all-integer arrays split everywhere, +-1e30 / Inf / NaN (for which the cast in IntRange::add is undefined:
    there the program asserts ok == false) -- and dev_io_args.h's refusals, as the stand-alone program built with
    -fsanitize=address,undefined"""
    exe = str(tmp_path / "query_range_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "query_range_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().strip().endswith("DONE"), p.stdout.decode()
