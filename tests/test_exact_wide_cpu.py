"""CPU-side checks of the exact search's fp16 list pass beyond 128 dimensions (option "exact_wide"): the option is in
the header's and the engine's table and refuses a missing handle before anything touches a device; the header still names what is not
offered; and the pass decision exact_slice makes (auncel_amd/csrc/exact_args.h: exact_pass_kind) with the wide tile's host helpers
runs as a program of its own -- tests/cpp/exact_wide_main.cpp -- built plain and under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import build, capi
    build.build()
    return capi


def test_the_option_exists_and_refuses_a_null_handle(capi):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    table = header[header.index(" *   key "):header.index("amd_ivf_set_option(h, key, NAN)")]
    assert '"exact_wide"' in table and "AUNCEL_AMD_EXACT_WIDE" in table
    engine = open(os.path.join(ROOT, "auncel_amd", "csrc", "ivf_engine.hip")).read()
    assert '{"exact_wide", "AUNCEL_AMD_EXACT_WIDE", nullptr}' in engine
    assert engine.index('{"exact_float", "AUNCEL_AMD_EXACT_FLOAT", nullptr}') < engine.index('{"exact_wide", "AUNCEL_AMD_EXACT_WIDE", nullptr}')
    assert L.amd_ivf_set_option(None, b"exact_wide", C.c_double(1)) == -2 and b"null" in L.amd_ivf_last_error()
    # the pinned words of the exact section, and the new value of the detail
    assert "Not offered: d > 128 in the pass" in header
    assert "3 wide fp16 + rescoring" in header
    assert "exact_pass_kind(" in engine and "launch_scan_all_wide_f16(" in engine


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_the_pass_decision_as_a_program(tmp_path, flags):
    exe = str(tmp_path / "exact_wide_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1"] + flags + [os.path.join(ROOT, "tests", "cpp", "exact_wide_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0 and out.strip().endswith("DONE"), out
    assert "failures 0" in out


@pytest.mark.parametrize("metric,d,W,mid,seed", __import__("exact_wide_cases").BOUND_CASES)
def test_the_bound_cases_separate_the_real_constant_from_the_fp32_one(metric, d, W, mid, seed):
    """the preconditions of test_gpu_exact_wide.py's bound test, on the numpy model: exact_float_constant(d, false) loses nothing at
    either seed depth and overflows no slots; (2 d + 32) 2^-24 alone loses a neighbour in at least 128 queries at the tight seed
    and answers at least 32 queries wrongly at the mid seed"""
    import coarse_pick_cases as cp
    import exact_wide_cases as wc
    import filter_bound_cases as fb
    c = fb.case(metric, d, W, seed=seed)
    real, fp32 = cp.half_constant(d, False), (2 * d + 32) * 2.0 ** -24
    for depth in (fb.TIGHT, mid):
        r = fb.report(c, depth, real)
        print(metric, d, "depth", depth, "real constant", r)
        assert r["lost"] == 0 and r["most"] <= fb.CAP // 4, r
    tight, at_mid = fb.report(c, fb.TIGHT, fp32), fb.report(c, mid, fp32)
    print(metric, d, "fp32 constant: tight", tight, "mid", at_mid)
    assert tight["lost"] >= wc.LOST_FLOOR, tight
    assert at_mid["wrong"] >= wc.WRONG_FLOOR, at_mid
