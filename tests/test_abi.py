"""CPU tests of the drop-in boundary: librsos_hip.so loads, exports every entry point
include/rsos_hip.h declares, and its host-only helpers behave (no GPU compute here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from records_common import M256

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsos_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(rh_[a-z0-9_]+)\s*\(", text))
    return sorted(names)


def test_header_declares_the_boundary():
    names = declared_symbols()
    for must in ["rh_lift_records_async", "rh_lift_dual_async", "rh_lift_encoded_async",
                 "rh_range_aggregates_async", "rh_combine_aggregates_async", "rh_store_create",
                 "rh_store_aggregate", "rh_store_rank", "rh_store_select", "rh_store_apply", "rh_last_error"]:
        assert must in names


def test_library_exports_every_declared_symbol(rsos_hip_lib):
    from rsos_hip import _abi
    L = _abi.lib()
    missing = [n for n in declared_symbols() if not hasattr(L, n)]
    assert not missing, missing
    # and the python binding declares a signature for each of them
    bound = {name for name, _, _ in _abi.SIGNATURES}
    assert set(declared_symbols()) <= bound


def test_rust_ffi_declares_every_symbol():
    """The Rust crate's FFI block (source only here) transcribes the whole header."""
    ffi = open(os.path.join(ROOT, "reconcile-rs_amd", "rust", "rsos-hip", "src", "ffi.rs")).read()
    declared = set(re.findall(r"pub fn (rh_[a-z0-9_]+)\s*\(", ffi))
    missing = [n for n in declared_symbols() if n not in declared]
    assert not missing, missing


def test_abi_version_and_enums(rsos_hip_lib, oracle_lib):
    from rsos_hip import _abi as A
    assert A.lib().rh_abi_version() == 1
    O = oracle_lib
    assert (A.KEY_UNIT, A.KEY_U32, A.KEY_U64, A.KEY_BYTES) == (O.KEY_UNIT, O.KEY_U32, O.KEY_U64, O.KEY_BYTES)
    assert (A.REC_PLAIN, A.REC_DATED, A.REC_PROJECTION) == (O.REC_PLAIN, O.REC_DATED, O.REC_PROJECTION)
    text = open(HEADER).read()
    assert "#define RH_BLOCK 256" in text and "#define RH_SUPER 65536" in text


def test_schema_support_and_lengths(rsos_hip_lib):
    from rsos_hip import RecordSchema
    s = RecordSchema.dated("bytes16", "bytes64")
    assert s.supported()
    assert s.record_len() == 120 and s.record_len(tombstone=True) == 48
    assert RecordSchema.projection("bytes16", "bytes64").record_len() == 100
    assert RecordSchema.dated("bytes16", "bytes1024").record_len() == 1080
    assert RecordSchema.plain("u32", "u32").record_len() == 8
    assert not RecordSchema.plain("bytes12", "bytes100").supported()


def test_bad_schema_is_an_error_not_a_crash(rsos_hip_lib):
    from rsos_hip import _abi as A
    bad = A.Schema(9, 4, 1, 4, 0, 0)
    assert A.lib().rh_schema_supported(C.byref(bad)) == A.ERR_ARG
    assert b"key_kind" in A.lib().rh_last_error()
    with pytest.raises(A.RsosHipError):
        A.check(A.lib().rh_schema_supported(C.byref(bad)), "x")


def test_host_fingerprint_group(rsos_hip_lib, golden):
    from rsos_hip import _abi as A
    L = A.lib()
    for kat in golden["reference"]["carry_borrow"]:
        a = np.array([int(x, 16) for x in kat["a"]], np.uint64)
        b = np.array([int(x, 16) for x in kat["b"]], np.uint64)
        out = np.zeros(4, np.uint64)
        fn = L.rh_fp_add if kat["op"] == "add" else L.rh_fp_sub
        fn(a.ctypes.data, b.ctypes.data, out.ctypes.data)
        assert [int(x) for x in out] == [int(x, 16) for x in kat["out"]]
    rng = np.random.default_rng(0)
    for _ in range(200):
        a = rng.integers(0, 2**64, 4, dtype=np.uint64, endpoint=False)
        b = rng.integers(0, 2**64, 4, dtype=np.uint64, endpoint=False)
        s, d, back = np.zeros(4, np.uint64), np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        L.rh_fp_add(a.ctypes.data, b.ctypes.data, s.ctypes.data)
        L.rh_fp_sub(s.ctypes.data, b.ctypes.data, back.ctypes.data)
        assert (back == a).all()
        ai = sum(int(x) << (64 * i) for i, x in enumerate(a))
        bi = sum(int(x) << (64 * i) for i, x in enumerate(b))
        assert sum(int(x) << (64 * i) for i, x in enumerate(s)) == (ai + bi) % M256


def test_python_value_types_mirror_reference(rsos_hip_lib):
    from rsos_hip import Aggregate, Fingerprint
    all_ones = Fingerprint((2**64 - 1,) * 4)
    assert all_ones + Fingerprint((1, 0, 0, 0)) == Fingerprint.ZERO
    assert Fingerprint.ZERO - Fingerprint((1, 0, 0, 0)) == all_ones
    f = Fingerprint((1, 2, 3, 4))
    assert -(-f) == f and f + (-f) == Fingerprint.ZERO
    assert Fingerprint.from_le_bytes(f.to_le_bytes()) == f
    assert str(f) == "0000000000000004000000000000000300000000000000020000000000000001"
    z = Aggregate(2, f + (-f))
    assert not z.is_empty() and Aggregate.ZERO.is_empty()


def test_encoded_lift_rejects_unpadded_length(rsos_hip_lib):
    """bytes_len must be a multiple of 4: checked before anything is launched."""
    from rsos_hip import _abi as A
    buf = (C.c_uint64 * 8)()
    rc = A.lib().rh_lift_encoded_async(C.addressof(buf), 7, C.addressof(buf), 1, C.addressof(buf), None, None)
    assert rc == A.ERR_ARG and b"multiple of 4" in A.lib().rh_last_error()


def test_fixed_lift_rejects_short_buffer(rsos_hip_lib):
    """n * record_len must fit in bytes_len: checked before anything is launched."""
    from rsos_hip import _abi as A
    buf = (C.c_uint64 * 8)()
    rc = A.lib().rh_lift_fixed_async(C.addressof(buf), 64, 120, 1, C.addressof(buf), None, None)
    assert rc == A.ERR_ARG and b"exceeds" in A.lib().rh_last_error()


def test_last_error_is_shared_by_every_source(rsos_hip_lib):
    """The thread's error string has one definition (csrc/rsos_hip_abi.hip): an entry point of each source
    file of the library, refused on an argument check before any HIP call, leaves its own message for
    rh_last_error; a thread that made no failing call reads an empty string."""
    import threading
    from rsos_hip import _abi as A
    L = A.lib()
    good = A.Schema(A.KEY_U32, 4, A.VAL_U32, 4, A.REC_PLAIN, 0)
    bad_key, bad_value = A.Schema(9, 4, 1, 4, 0, 0), A.Schema(1, 4, 9, 4, 0, 0)
    out, n64, buf = C.c_void_p(), C.c_uint64(), (C.c_uint64 * 8)()
    one_device, r_out, consumed = (C.c_int * 1)(0), C.c_size_t(), C.c_size_t()
    calls = [  # (source file, call, status, a piece of its message)
        ("rsos_hip_abi.hip (store)", lambda: L.rh_store_create(0, C.byref(bad_key), C.byref(out)), A.ERR_ARG,
         b"bad key_kind"),
        ("rsos_hip_abi.hip (estore)", lambda: L.rh_estore_create(0, None), A.ERR_ARG, b"out is NULL"),
        ("rsos_hip_abi.hip (snapshot)", lambda: L.rh_snapshot_header(C.addressof(buf), 4, C.byref(n64)), A.ERR_DATA,
         b"shorter than the 8-byte format header"),
        ("rsos_hip_abi.hip (lift)", lambda: L.rh_lift_encoded_async(C.addressof(buf), 7, C.addressof(buf), 1,
                                                                    C.addressof(buf), None, None),
         A.ERR_ARG, b"multiple of 4"),
        ("sharded_store.hip", lambda: L.rh_sstore_create(one_device, 0, C.byref(good), C.byref(out)), A.ERR_ARG,
         b"sstore: bad arguments"),
        ("shard_route.hip", lambda: L.rh_route_columns_device(C.byref(bad_value), None, 1, None, None, 0, None, None, 0, None,
                                                              None, None), A.ERR_ARG, b"bad value_kind"),
        ("wire_codec.cpp", lambda: L.rh_wire_decode_range_aggregates(C.byref(good), A.FORM_ARRAY, -1, None, 8, 0, None, None,
                                                                     None, None, None, C.byref(r_out), C.byref(consumed)),
         A.ERR_ARG, b"input is NULL"),
    ]
    for source, call, status, piece in calls:
        assert call() == status, source
        assert piece in L.rh_last_error(), (source, L.rh_last_error())
    seen = []
    t = threading.Thread(target=lambda: seen.append(L.rh_last_error()))
    t.start()
    t.join()
    assert seen == [b""]
    assert b"input is NULL" in L.rh_last_error()  # and this thread's is still its own


def test_product_fails_loudly_without_the_library(tmp_path):
    """No CPU fallback: with librsos_hip.so missing, the binding raises instead of computing."""
    import subprocess
    import sys
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import rsos_hip._abi as A\n"
        "A.LIB_PATH = %r\n"
        "try:\n"
        "    A.lib()\n"
        "except RuntimeError as e:\n"
        "    print('raised:', e)\n"
        "    sys.exit(0)\n"
        "sys.exit(1)\n"
    ) % (os.path.join(ROOT, "reconcile-rs_amd"), str(tmp_path / "missing.so"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HIP path is the only path" in r.stdout


def test_host_tensors_are_rejected(rsos_hip_lib):
    """The device entry points take HBM-resident columns; host tensors are an error, not a CPU path."""
    import torch
    from rsos_hip import RecordSchema, lift_records
    s = RecordSchema.plain("u32", "u32")
    cols = {"keys": torch.zeros((4, 4), dtype=torch.uint8), "values": torch.zeros((4, 4), dtype=torch.uint8)}
    with pytest.raises((ValueError, RuntimeError)):
        lift_records(s, cols)


def test_apply_device_many_argument_checks(rsos_hip_lib):
    """rh_store_apply_device_many refuses a NULL store, and NULL column / size arrays for k > 0,
    before touching a device."""
    from rsos_hip import _abi as A
    L = A.lib()
    assert L.rh_store_apply_device_many(None, None, None, None, 0, None, None) == A.ERR_ARG
    assert L.rh_store_apply_device_many(None, None, None, None, 3, None, None) == A.ERR_ARG


def test_store_row_cap_is_refused_at_the_boundary(rsos_hip_lib):
    """One rh_store holds fewer than 2^31 rows (include/rsos_hip.h "Row cap"; the reference's
    Rsos::size() is a usize, rsos/src/rsos_trait.rs:44).  A reservation or load of 2^31 rows is
    refused with RH_ERR_ARG and a message naming the sharded store, before any device is touched
    (the cap is checked on the arguments first), and the header and the Rust FFI state it."""
    from rsos_hip import _abi as A
    L = A.lib()
    for rows, batch in ((1 << 31, 0), (10, 1 << 31), (1 << 40, 0)):
        assert L.rh_store_reserve(None, rows, batch) == A.ERR_ARG
        msg = L.rh_last_error().decode()
        assert "2^31 rows" in msg and "rh_sstore" in msg, msg
    cols = A.Columns()
    assert L.rh_store_load(None, C.byref(cols), 1 << 31) == A.ERR_ARG
    assert "2^31 rows" in L.rh_last_error().decode()
    assert L.rh_store_load_device(None, C.byref(cols), 1 << 31, None) == A.ERR_ARG
    assert "2^31 rows" in L.rh_last_error().decode()
    assert L.rh_store_reserve(None, (1 << 31) - 1, 0) == A.ERR_ARG  # under the cap: the NULL store
    assert "NULL" in L.rh_last_error().decode()
    header = open(HEADER).read()
    assert "#define RH_STORE_MAX_ROWS 2147483648" in header and "Row cap" in header
    ffi = open(os.path.join(ROOT, "reconcile-rs_amd", "rust", "rsos-hip", "src", "ffi.rs")).read()
    assert "pub const RH_STORE_MAX_ROWS: u64 = 2147483648;" in ffi
    assert "2³¹" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- the Rust FFI block against the header, signature by signature -------------------------------
# (the crate cannot be compiled in this image: no cargo / rustc; this is the check a
# compiler would make at the boundary -- arity, pointer depth and constness, integer width)
_C_BASE = {"int": "i32", "int32_t": "i32", "unsigned": "u32", "uint32_t": "u32", "uint64_t": "u64",
           "int64_t": "i64", "size_t": "usize", "uint8_t": "u8", "int8_t": "i8", "char": "i8", "void": "void",
           "double": "f64", "float": "f32", "uint16_t": "u16", "int16_t": "i16"}
_R_BASE = {"c_int": "i32", "i32": "i32", "u32": "u32", "u64": "u64", "i64": "i64", "usize": "usize", "u8": "u8",
           "i8": "i8", "c_char": "i8", "c_void": "void", "f64": "f64", "f32": "f32", "u16": "u16", "i16": "i16",
           "()": "void"}


def _c_type(t: str):
    """(base, [const-ness of each pointer level's pointee, outermost first]) of a C parameter type"""
    t = t.replace("*", " * ").split()
    # split into pointer levels: the tokens before the first '*' are the base (+ its const)
    levels, cur = [], []
    for tok in t:
        if tok == "*":
            levels.append(cur)
            cur = []
        else:
            cur.append(tok)
    levels.append(cur)  # trailing qualifiers of the outermost pointer itself (ignored)
    base_toks = [x for x in levels[0] if x not in ("const", "struct", "unsigned")] or ["unsigned"]
    if "unsigned" in levels[0] and base_toks == ["int"]:
        base_toks = ["unsigned"]
    base = base_toks[-1]
    base = _C_BASE.get(base, base)
    # pointee constness per level: level 0's const applies to the innermost pointee
    consts = ["const" in lv for lv in levels[:-1]]
    return base, list(reversed(consts))


def _c_param(p: str):
    p = p.strip()
    arr = re.search(r"\[\s*\d*\s*\]$", p)
    if arr:  # `const uint64_t a[4]`: a pointer
        p = p[:arr.start()].strip()
        p = re.sub(r"\b(\w+)$", r"* \1", p)
    name = re.search(r"(\w+)$", p).group(1)
    return _c_type(p[: len(p) - len(name)])


def _r_type(t: str):
    t = t.strip()
    consts = []
    while t.startswith("*"):
        m = re.match(r"\*\s*(const|mut)\s+", t)
        consts.append(m.group(1) == "const")
        t = t[m.end():]
    return _R_BASE.get(t, t), consts


def _c_prototypes():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.strip().startswith("#"))
    text = re.sub(r"typedef struct[^;]*?\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(rh_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        ps = [] if params in ("", "void") else [_c_param(p) for p in params.split(",")]
        out[name] = (_c_type(ret), ps)
    return out


def _rust_prototypes():
    ffi = open(os.path.join(ROOT, "reconcile-rs_amd", "rust", "rsos-hip", "src", "ffi.rs")).read()
    ffi = re.sub(r"//[^\n]*", "", ffi)
    out = {}
    for m in re.finditer(r"pub fn (rh_\w+)\s*\(([^)]*)\)\s*(->\s*([^;]+))?;", ffi, flags=re.S):
        name, params, ret = m.group(1), m.group(2), (m.group(4) or "()").strip()
        ps = [_r_type(p.split(":", 1)[1]) for p in params.split(",") if p.strip()]
        out[name] = (_r_type(ret), ps)
    return out


def test_rust_ffi_signatures_match_the_header():
    """Every extern "C" fn of ffi.rs has its header prototype's arity, and per parameter and return
    value the same pointer depth, pointee constness at every level and base type width (c_int =
    int = i32, size_t = usize, char = c_char, void = c_void / ())."""
    c, r = _c_prototypes(), _rust_prototypes()
    assert set(c) == set(declared_symbols())
    assert set(r) == set(c), (set(c) ^ set(r))
    bad = []
    for name, (cret, cps) in sorted(c.items()):
        rret, rps = r[name]
        if len(cps) != len(rps):
            bad.append((name, "arity", len(cps), len(rps)))
            continue
        if cret != rret:
            bad.append((name, "return", cret, rret))
        for i, (cp, rp) in enumerate(zip(cps, rps)):
            if cp != rp:
                bad.append((name, "param %d" % i, cp, rp))
    assert not bad, bad


def test_signature_parser_catches_mismatches():
    """The parser above distinguishes what a compiler would: width, pointer depth, constness."""
    assert _c_param("const uint8_t *const *dev_ops") == ("u8", [True, True])
    assert _r_type("*const *const u8") == ("u8", [True, True])
    assert _c_param("uint64_t *n_new") == ("u64", [False])
    assert _r_type("*mut u64") == ("u64", [False])
    assert _c_param("size_t n") == ("usize", []) != _c_param("uint32_t n")
    assert _c_param("const uint64_t a[4]") == ("u64", [True]) == _r_type("*const u64")
    assert _c_param("void *stream") == _r_type("*mut c_void")
    assert _c_param("const void *keys") != _r_type("*mut c_void")


# ---- the Rust FFI block against the header, data layout and constants ---------------------------
def _c_structs(text=None):
    """{name: [(field, base, pointer depth, pointee constness per level, array length)]} of every
    `typedef struct name { ... } name;` in the header"""
    text = re.sub(r"/\*.*?\*/", "", text if text is not None else open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"typedef struct (\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in m.group(2).split(";"):
            decl = decl.strip()
            if not decl:
                continue
            typ, names = re.match(r"(.*?)(\**\s*\w+(?:\s*\[\s*\d+\s*\])?(?:\s*,\s*\**\s*\w+(?:\s*\[\s*\d+\s*\])?)*)$",
                                  decl, flags=re.S).groups()
            for nm in names.split(","):
                nm = nm.strip()
                stars = nm.count("*")
                nm = nm.replace("*", "").strip()
                arr = re.search(r"\[\s*(\d+)\s*\]", nm)
                n_arr = int(arr.group(1)) if arr else 0
                nm = re.sub(r"\[.*\]", "", nm).strip()
                base, consts = _c_type(typ + " " + "*" * stars)
                fields.append((nm, base, len(consts), consts, n_arr))
        out[m.group(3)] = fields
    return out


def _rust_structs(ffi=None):
    ffi = ffi if ffi is not None else open(os.path.join(ROOT, "reconcile-rs_amd", "rust", "rsos-hip", "src", "ffi.rs")).read()
    ffi = re.sub(r"//[^\n]*", "", ffi)
    out = {}
    for m in re.finditer(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct (\w+)\s*\{(.*?)\}", ffi, flags=re.S):
        fields = []
        for decl in m.group(2).split(","):
            decl = decl.strip()
            if not decl or decl.startswith("_private"):
                continue
            nm, ty = [x.strip() for x in re.sub(r"^pub\s+", "", decl).split(":", 1)]
            arr = re.match(r"\[(.*);\s*(\d+)\]$", ty)
            n_arr = int(arr.group(2)) if arr else 0
            base, consts = _r_type(arr.group(1) if arr else ty)
            fields.append((nm, base, len(consts), consts, n_arr))
        out[m.group(1)] = fields
    return out


def _c_consts(text=None):
    text = re.sub(r"/\*.*?\*/", "", text if text is not None else open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"typedef enum \w+\s*\{(.*?)\}", text, flags=re.S):
        for item in m.group(1).split(","):
            kv = re.match(r"\s*(RH_\w+)\s*=\s*(-?\d+)", item)
            if kv:
                out[kv.group(1)] = int(kv.group(2))
    for m in re.finditer(r"#define (RH_\w+) (-?\d+)", text):
        out[m.group(1)] = int(m.group(2))
    return out


def _rust_consts(ffi=None):
    ffi = ffi if ffi is not None else open(os.path.join(ROOT, "reconcile-rs_amd", "rust", "rsos-hip", "src", "ffi.rs")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"pub const (RH_\w+):\s*\w+\s*=\s*(-?\d+)\s*;", ffi)}


def _layout_mismatches(ffi=None):
    c, r = _c_structs(), _rust_structs(ffi)
    bad = []
    for name, fields in c.items():
        if name not in r:
            bad.append((name, "missing in ffi.rs"))
        elif r[name] != fields:
            bad.append((name, fields, r[name]))
    cc, rc = _c_consts(), _rust_consts(ffi)
    for k, v in cc.items():
        if rc.get(k) != v:
            bad.append((k, v, rc.get(k)))
    for k in rc:
        if k not in cc:
            bad.append((k, "not in the header"))
    return bad


def test_rust_ffi_layout_and_constants_match_the_header():
    """Every `typedef struct` of the header has a #[repr(C)] twin in ffi.rs with the same fields in
    the same order (name, base type width, pointer depth, pointee constness, array length), and every
    enumerator / #define of the header is a `pub const` of ffi.rs with the same value (and no other)."""
    c = _c_structs()
    assert {"rh_schema", "rh_columns", "rh_aggregate", "rh_snapshot_info", "rh_segments", "rh_round_outcome"} <= set(c)
    assert c["rh_aggregate"] == [("fingerprint", "u64", 0, [], 4), ("size", "u64", 0, [], 0)]
    assert len(_c_consts()) >= 25
    assert _layout_mismatches() == []


def test_layout_check_catches_a_swapped_field_and_a_wrong_constant():
    """The check above fails on the mistakes it exists for: two fields swapped, a field's width
    changed, a pointer's constness flipped, a renumbered constant."""
    ffi = open(os.path.join(ROOT, "reconcile-rs_amd", "rust", "rsos-hip", "src", "ffi.rs")).read()
    swapped = ffi.replace("    pub fingerprint: [u64; 4],\n    pub size: u64,", "    pub size: u64,\n    pub fingerprint: [u64; 4],")
    assert swapped != ffi and _layout_mismatches(swapped)
    narrowed = ffi.replace("    pub key_len: u32,", "    pub key_len: u64,")
    assert narrowed != ffi and _layout_mismatches(narrowed)
    mutable = ffi.replace("    pub phys: *const u64,", "    pub phys: *mut u64,")
    assert mutable != ffi and _layout_mismatches(mutable)
    renumbered = ffi.replace("pub const RH_REC_DATED: i32 = 1;", "pub const RH_REC_DATED: i32 = 2;")
    assert renumbered != ffi and _layout_mismatches(renumbered)
