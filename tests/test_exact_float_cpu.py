"""CPU-side checks of the exact search's fp16 list pass over float lists: amd_ivf_last_exact_detail is exported, declared, bound (the
Python handle and the class mirror) and refuses a missing handle or result pointer before anything touches a device; the option that
switches the pass on is accepted and documented; and the keep rule the kernel compiles (auncel_amd/csrc/exact_args.h) keeps every
pair whose reference distance is at or within the threshold -- tests/cpp/exact_float_main.cpp, a program of its own, built plain."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import build, capi
    build.build()
    return capi


def test_the_detail_entry_point_and_the_option_exist(capi):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    assert hasattr(L, "amd_ivf_last_exact_detail") and "amd_ivf_last_exact_detail" in capi.SYMBOLS
    assert L.amd_ivf_last_exact_detail.restype is C.c_int
    assert re.search(r"^int amd_ivf_last_exact_detail\(amd_ivf_t\* h, uint64_t out\[4\]\);", header, re.M)
    assert callable(capi.Handle.last_exact_detail)
    assert '"exact_float"' in header[header.index(" *   key "):header.index("amd_ivf_set_option(h, key, NAN)")]
    engine = open(os.path.join(ROOT, "auncel_amd", "csrc", "ivf_engine.hip")).read()
    assert '{"exact_float", "AUNCEL_AMD_EXACT_FLOAT", nullptr}' in engine
    mirror = open(os.path.join(ROOT, "auncel_amd", "csrc", "host", "IndexIVFFlat.h")).read()
    assert mirror.count("void exact_detail(uint64_t out[4]) const;") == 2  # (IndexIVFFlat and IndexIVFFlatSubset)
    # "Not offered" no longer names the float pass
    assert "Not offered: d > 128 in the pass" in header


def test_refuses_bad_arguments_before_the_device(capi):
    L = capi.lib()
    out4 = (C.c_uint64 * 4)()
    some = C.c_void_p(64)  # (never followed: refused, or no device, first)
    for args in ((None, out4), (some, None)):
        assert L.amd_ivf_last_exact_detail(*args) == -2
        assert b"null" in L.amd_ivf_last_error()
    assert L.amd_ivf_set_option(None, b"exact_float", C.c_double(0)) == -2 and b"null" in L.amd_ivf_last_error()


def test_the_keep_rule_as_a_program(tmp_path):
    exe = str(tmp_path / "exact_float_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "exact_float_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0 and out.strip().endswith("DONE"), out
    assert re.search(r"kept \d+ of \d+ ", out)
