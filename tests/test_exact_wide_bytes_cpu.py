"""CPU-side checks of the exact search's byte list pass beyond 128 dimensions (option "exact_wide_bytes"): the option is
in the header's and the engine's table and refuses a missing handle before anything touches a device; the pass decision
(auncel_amd/csrc/exact_args.h: exact_pass_kind_bytes) runs as a program of its own -- tests/cpp/exact_wide_bytes_main.cpp -- built plain
and under the address and undefined-behaviour sanitizers; and the data of test_gpu_exact_wide_bytes.py (exact_wide_bytes_cases.py)
has the properties that file's assertions lean on, counted with exact integers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exact_wide_bytes_cases as wb
from test_gpu_exact import IP, L2
from test_gpu_exact_range import emitted, int_dis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 1 << 24


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import build, capi
    build.build()
    return capi


def test_the_option_exists_and_refuses_a_null_handle(capi):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    table = header[header.index(" *   key "):header.index("amd_ivf_set_option(h, key, NAN)")]
    assert '"exact_wide_bytes"' in table and "AUNCEL_AMD_EXACT_WIDE_BYTES" in table
    engine = open(os.path.join(ROOT, "auncel_amd", "csrc", "ivf_engine.hip")).read()
    assert '{"exact_wide_bytes", "AUNCEL_AMD_EXACT_WIDE_BYTES", nullptr}' in engine
    assert engine.index('{"exact_wide", "AUNCEL_AMD_EXACT_WIDE", nullptr}') < engine.index('{"exact_wide_bytes", "AUNCEL_AMD_EXACT_WIDE_BYTES", nullptr}')
    assert L.amd_ivf_set_option(None, b"exact_wide_bytes", C.c_double(1)) == -2 and b"null" in L.amd_ivf_last_error()
    assert "4 wide bytes" in header
    assert "exact_pass_kind_bytes(" in engine and "launch_scan_all_wide_i8(" in engine


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_the_pass_decision_as_a_program(tmp_path, flags):
    exe = str(tmp_path / "exact_wide_bytes_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1"] + flags + [os.path.join(ROOT, "tests", "cpp", "exact_wide_bytes_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0 and out.strip().endswith("DONE"), out
    assert "failures 0" in out


def byte_rule(d, *arrays):
    m = max(float(a.max()) for a in arrays)
    lo = min(float(a.min()) for a in arrays)
    assert lo >= 0 and m <= 255 and all(np.array_equal(a, np.floor(a)) for a in arrays)
    assert d * m * m <= LIMIT, (d, m)
    return int(m)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", wb.STAGE_D)
def test_the_stage_cases_hold_the_byte_rule_and_half_of_every_batch_is_free_of_ties(d, metric):
    cen, assign, xb, xq = wb.stage_case(d, metric)
    m = byte_rule(d, xb, xq)
    assert m == wb.top_of(d) and xb.max() == m and xq.max() == m
    assert m == 255 if d <= 258 else d * (m + 1) * (m + 1) > LIMIT
    if d == 1024:
        assert d * m * m == LIMIT
    for n, k in wb.BATCHES:
        tied, within = wb.ties_within(metric, xb, xq[:n], k)
        print(d, metric, n, k, "ties", int(tied.sum()), "largest within", int(within.max()))
        assert n - int(tied.sum()) >= (n + 1) // 2 and within.max() < wb.CAP


@pytest.mark.parametrize("metric", [L2, IP])
def test_the_other_cases(metric):
    for sizes, nblk in wb.TAIL_SIZES:
        assert sum(2 * -(-s // 64) for s in sizes) == nblk
        cen, assign, xb, xq, last = wb.tail_case(sizes, metric)
        byte_rule(200, xb, xq)
        tied, within = wb.ties_within(metric, xb, xq, 10)
        E = wb.exact_table(metric, xq, xb)
        best = np.argsort(E if metric == L2 else -E, axis=1, kind="stable")[:, :10]
        assert (assign[best] == last).all()  # the neighbours are entries of the last list, whose blocks are the stream's last
        print("tail", sizes, metric, "ties", int(tied.sum()), "largest within", int(within.max()))
        assert 2 * int(tied.sum()) <= len(xq) and within.max() < wb.CAP
    for d in (200, 192):
        cen, assign, xb, xq = wb.last_dims_case(d, metric)
        byte_rule(d, xb, xq)
        assert np.array_equal(xb[:, :d - 8], cen[assign][:, :d - 8])
        tied, within = wb.ties_within(metric, xb, xq, 10)
        print("last dimensions", d, metric, "ties", int(tied.sum()), "largest within", int(within.max()))
        assert 2 * int(tied.sum()) <= len(xq) and within.max() < wb.CAP
    cen, assign, xb, xq, tied, within = wb.small_range_case(metric)
    byte_rule(136, xb, xq)
    print("values 0 .. 8", metric, "queries", len(xq), "ties", int(tied.sum()), "largest within", int(within.max()))
    assert len(xq) == 200 and 0 < int(tied.sum()) <= 100 and within.max() <= wb.CAP // 2
    for d in (200, 960):
        cen, assign, xb, xq = wb.range_case(d, metric)
        byte_rule(d, xb, xq)
        dis = int_dis(metric, xb, xq)
        v = float(np.sort(dis[0])[15] if metric == L2 else -np.sort(-dis[0])[15])
        assert (dis[0] == v).sum() >= 1 and float(np.float32(v)) == v
        most = int(emitted(metric, dis, v).sum(1).max())
        print("range", d, metric, "radius", v, "largest emitted", most)
        assert most < wb.CAP
