"""CPU-side checks of amd_ivf_build_dev / amd_ivf_last_build (include/auncel_amd.h): exported, declared, bound, a missing handle or
result slot is refused; and the host half of the call -- build_args.h's refusals and the chunk cut -- as a program of its own
(tests/cpp/build_args_main.cpp) built with the address and undefined-behaviour sanitizers and run directly."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported_declared_bound_and_refuse_null_arguments():
    from auncel_amd import build, capi
    build.build()
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    for s in ("amd_ivf_build_dev", "amd_ivf_last_build"):
        assert hasattr(L, s) and s in capi.SYMBOLS and getattr(L, s).restype is C.c_int
    assert re.search(r"^int amd_ivf_build_dev\(amd_ivf_t\* q, size_t n, const void\* d_x, int dtype, size_t ldx, const int64_t\* d_ids, "
                     r"int64_t id_base,\s+const int64_t\* d_assign, int coarse_mode, void\* stream, amd_ivf_t\*\* out\);", header, re.M)
    assert "int amd_ivf_last_build(amd_ivf_t* built, uint64_t out[4]);" in header
    assert callable(capi.Handle.build_dev) and callable(capi.Handle.last_build) and "ivf_build.hip" in build.SOURCES
    some, out = C.c_void_p(64), C.c_void_p(7)  # (`some` is never followed: the handle is refused first)
    assert L.amd_ivf_build_dev(None, C.c_size_t(2), some, 0, C.c_size_t(2), None, C.c_int64(0), None, 0, None, C.byref(out)) == -2
    assert b"null argument" in L.amd_ivf_last_error() and out.value is None
    assert L.amd_ivf_build_dev(None, C.c_size_t(2), some, 0, C.c_size_t(2), None, C.c_int64(0), None, 0, None, None) == -2
    assert L.amd_ivf_last_build(None, (C.c_uint64 * 4)()) == -2 and b"null argument" in L.amd_ivf_last_error()


def test_the_host_part_as_a_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "build_args_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "build_args_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().strip().endswith("DONE"), p.stdout.decode()
