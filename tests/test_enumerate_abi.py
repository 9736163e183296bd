"""rh_store_enumerate_segments / rh_sstore_enumerate_segments at the C boundary, without a GPU: both
are exported and declared, refuse a NULL store (and the other argument errors that are checked before
any device call) with RH_ERR_ARG, and rh_enumerated has the header's layout in rsos_hip/_abi.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsos_hip.h")
ENTRY_POINTS = ("rh_store_enumerate_segments", "rh_sstore_enumerate_segments")


def test_both_entry_points_are_declared_and_exported(rsos_hip_lib):
    from rsos_hip import _abi as A
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = C.CDLL(A.LIB_PATH)
    declared = {name: (res, args) for name, res, args in A.SIGNATURES}
    for name in ENTRY_POINTS:
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not in the header"
        assert len(m.group(1).split(",")) == 4
        assert getattr(raw, name)  # AttributeError: the library does not export it
        res, args = declared[name]
        assert res is C.c_int and len(args) == 4 and args[2] is C.c_uint64


def test_rh_enumerated_has_the_headers_layout(rsos_hip_lib):
    from rsos_hip import _abi as A
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct rh_enumerated\s*\{(.*?)\}\s*rh_enumerated\s*;", header, flags=re.S).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.replace("*", " * ").split())
        if decl:
            typ, name = decl.rsplit(" ", 1)
            c_fields.append((name, typ))
    assert c_fields == [("first_ranks", "const uint64_t *"), ("offsets", "const uint64_t *"), ("keys", "const void *"),
                        ("n", "size_t"), ("rows", "uint64_t")]
    want = {"const uint64_t *": C.c_void_p, "const void *": C.c_void_p, "size_t": C.c_size_t, "uint64_t": C.c_uint64}
    assert [(n, want[t]) for n, t in c_fields] == list(A.Enumerated._fields_)
    assert C.sizeof(A.Enumerated) == 40 and A.Enumerated.rows.offset == 32


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_any_device_call(rsos_hip_lib, name):
    from rsos_hip import _abi as A
    fn = getattr(A.lib(), name)
    kinds = np.zeros(1, np.uint8)
    seg = A.Segments(kinds.ctypes.data, None, kinds.ctypes.data, None, None, 1, 1)
    out = A.Enumerated(1, 1, 1, 1, 1)
    assert fn(None, C.byref(seg), 0, C.byref(out)) == A.ERR_ARG  # a NULL store
    assert "NULL" in A.lib().rh_last_error().decode()
    assert fn(None, None, 0, C.byref(out)) == A.ERR_ARG
    assert fn(None, C.byref(seg), 0, None) == A.ERR_ARG
