"""CPU-side checks of the join entry points (include/auncel_amd.h: amd_ivf_concat, amd_ivf_last_concat): they are exported and bound,
capi's struct has the header's layout, and they refuse missing arguments before anything touches a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amd_ivf_concat", "amd_ivf_last_concat"]
CTYPES = {"amd_ivf_t*": C.c_void_p, "const uint64_t*": C.POINTER(C.c_uint64), "int64_t": C.c_int64}


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import build, capi
    build.build()
    return capi


def test_new_entry_points_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert hasattr(L, s) and s in capi.SYMBOLS
    for m in ("concat", "last_concat"):
        assert callable(getattr(capi.Handle, m))


def test_part_struct_matches_the_header(capi):
    hdr = open(os.path.join(ROOT, "include", "auncel_amd.h")).read()
    m = re.search(r"typedef struct \{(.*?)\}\s*amd_ivf_part_t;", hdr, re.S)
    assert m, "amd_ivf_part_t is not in the header"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            typ, name = decl.rsplit(" ", 1)
            fields.append((name, CTYPES[typ]))
    assert [n for n, _ in fields] == ["h", "begin", "end", "id_add"]
    assert [(n, t) for n, t in capi.Part._fields_] == fields
    # four 8-byte members, no padding: what a C compiler lays out for the header's struct on this ABI
    assert C.sizeof(capi.Part) == 32
    assert [getattr(capi.Part, n).offset for n, _ in fields] == [0, 8, 16, 24]
    assert "int amd_ivf_concat(const amd_ivf_part_t* parts, size_t nparts, amd_ivf_t** out);" in hdr
    assert "int amd_ivf_last_concat(amd_ivf_t* joined, uint64_t out[4]);" in hdr


def test_refuse_missing_arguments(capi):
    L = capi.lib()
    out = C.c_void_p()
    out4 = (C.c_uint64 * 4)()
    one = (capi.Part * 1)()  # (a part whose handle is null)
    for args in ((None, C.c_size_t(1), C.byref(out)), (one, C.c_size_t(1), None), (one, C.c_size_t(0), C.byref(out)),
                 (one, C.c_size_t(65), C.byref(out)), (one, C.c_size_t(1), C.byref(out))):
        L.amd_ivf_last_error()
        assert L.amd_ivf_concat(*args) == -2, args
        assert L.amd_ivf_last_error().decode() != ""
        assert not out.value
    assert L.amd_ivf_concat(None, C.c_size_t(1), C.byref(out)) == -2 and b"null" in L.amd_ivf_last_error()
    assert L.amd_ivf_concat(one, C.c_size_t(0), C.byref(out)) == -2 and b"parts" in L.amd_ivf_last_error()
    assert L.amd_ivf_concat(one, C.c_size_t(1), C.byref(out)) == -2 and b"part 0 is null" in L.amd_ivf_last_error()
    assert L.amd_ivf_last_concat(None, out4) == -2 and b"null" in L.amd_ivf_last_error()
    with pytest.raises(capi.EngineError) as e:
        capi.Handle.concat([])
    assert e.value.code == -2
