"""Snapshot save: rh_snapshot_encode_device (csrc/snap_encode.hip) turns device columns into the
RCNL v1 header and entries, the inverse of the ragged decode; rsos_hip.snapshot adds the tail's
encoder and the file write.

Expected bytes come from the pure-Python writer of tests/ragged_snapshot_common.py (write_snapshot,
tail_bytes), read back by its sequential parser where a case has no writer-side expectation.
"""
import ctypes as C
import functools
import ipaddress
import os
import re
import struct

import numpy as np
import pytest

from ragged_snapshot_common import (DECODE_SHAPES, MEMBERS, SHAPES, gen_records, key_rows, ordered, parse_snapshot, schemas,
                                    tail_bytes, write_snapshot)
from records_common import key_width, val_width

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(0, 0.0), (1, 0.0), (1, 1.0), (63, 0.25), (64, 0.25), (65, 0.25), (777, 0.25), (20000, 0.1), (5000, 1.0)]
GUARD = 64
FORMS = {"array": 0, "vec": 1}


# ---- columns of a record list ---------------------------------------------------------------------

def host_columns(shape, recs):
    """The column form of `recs` as the decode gives it: a tombstone's value row zeroed, its
    VARBYTES span empty."""
    n = len(recs)
    vw = val_width(SHAPES[shape][1])
    cols = {"keys": np.ascontiguousarray(key_rows(shape, recs)),
            "phys": np.array([r[1][0] for r in recs], np.uint64).view(np.int64),
            "logical": np.array([r[1][1] for r in recs], np.uint32).view(np.int32),
            "node": np.array([r[1][2] for r in recs], np.uint64).view(np.int64),
            "tags": np.array([r[2] for r in recs], np.uint8)}
    if vw is None:
        offs = np.zeros(n + 1, np.int64)
        offs[1:] = np.cumsum([len(r[3]) for r in recs])
        cols["values"] = (np.frombuffer(b"".join(r[3] for r in recs), np.uint8), offs)
    else:
        cols["values"] = np.frombuffer(b"".join(r[3] if not r[2] else bytes(vw) for r in recs),
                                       np.uint8).reshape(n, vw)
    return cols


def to_cuda(cols):
    import torch

    def up(a):
        return torch.from_numpy(np.array(a)).cuda()
    return {k: (tuple(up(x) for x in v) if isinstance(v, tuple) else up(v)) for k, v in cols.items()}


def encode_raw(shape, cols, out, cap, form=None):
    """rh_snapshot_encode_device as the C ABI gives it: (status, SnapshotInfo).  out: a device
    tensor or None."""
    import torch
    from rsos_hip import _abi as A
    from rsos_hip.snapshot import _encode_columns
    sd, _, kf = schemas(shape)
    c, n, _, held = _encode_columns(sd, cols)
    s, info = sd.c(), A.SnapshotInfo()
    rc = A.lib().rh_snapshot_encode_device(C.byref(s), FORMS[kf] if form is None else form, C.byref(c), n,
                                           None if out is None else out.data_ptr(), cap, C.byref(info), None)
    torch.cuda.synchronize()
    del held
    return rc, info


def guarded(end):
    import torch
    return torch.full((end + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")


@functools.lru_cache(maxsize=4)
def expected(shape, n, tomb):
    recs = gen_records(shape, n, tomb)
    data, end, _ = write_snapshot(shape, recs)
    return recs, data[:end]


# ---- CPU ----------------------------------------------------------------------------------------

def test_header_and_library_have_the_entry_point(rsos_hip_lib):
    from rsos_hip import _abi as A
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsos_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+rh_snapshot_encode_device\s*\(", text)
    assert hasattr(A.lib(), "rh_snapshot_encode_device")
    assert "rh_snapshot_encode_device" in {name for name, _, _ in A.SIGNATURES}


def test_argument_errors_need_no_device(rsos_hip_lib):
    from rsos_hip import RecordSchema, _abi as A
    L = A.lib()
    none = A.Columns()
    info = A.SnapshotInfo()

    def call(schema, form, n, info_ref):
        return L.rh_snapshot_encode_device(C.byref(schema), form, C.byref(none), n, None, 0, info_ref, None)
    b16 = RecordSchema.dated("bytes16", "bytes64").c()
    str31 = RecordSchema.dated("str31", "var").c()
    assert call(b16, 4, 0, C.byref(info)) == A.ERR_ARG and b"bad key_form" in L.rh_last_error()
    assert call(b16, -1, 0, C.byref(info)) == A.ERR_ARG and b"bad key_form" in L.rh_last_error()
    assert call(str31, A.FORM_ARRAY, 0, C.byref(info)) == A.ERR_ARG
    assert call(str31, A.FORM_ARRAY | A.FORM_RAGGED, 0, C.byref(info)) == A.ERR_ARG
    assert call(RecordSchema.plain("bytes16", "bytes64").c(), 0, 0, C.byref(info)) == A.ERR_ARG
    assert call(RecordSchema.projection("bytes16", "bytes64").c(), 0, 0, C.byref(info)) == A.ERR_ARG
    assert call(A.Schema(A.KEY_STR, 32, A.VAL_BYTES, 64, A.REC_DATED, 0), A.FORM_VEC, 0,
                C.byref(info)) == A.ERR_UNSUPPORTED
    assert call(A.Schema(9, 4, 1, 4, A.REC_DATED, 0), 0, 0, C.byref(info)) == A.ERR_ARG
    assert call(b16, 0, 1 << 31, C.byref(info)) == A.ERR_ARG
    assert call(b16, 0, 0, None) == A.ERR_ARG
    for schema, form in ((b16, 0), (b16, A.FORM_VEC | A.FORM_RAGGED), (str31, A.FORM_VEC)):
        info = A.SnapshotInfo(9, 9, 9, 9)
        assert call(schema, form, 0, C.byref(info)) == A.OK
        assert (info.entries, info.tombstones, info.entries_end, info.keys) == (0, 0, 16, 0)
    # an unaligned output is refused before anything is launched
    assert L.rh_snapshot_encode_device(C.byref(b16), 0, C.byref(none), 0, 8, 64, C.byref(info), None) == A.ERR_ARG


PEERS = {ipaddress.ip_address("10.1.2.3"): 5, ipaddress.ip_address("fe80::1"): 2**40}


@pytest.mark.parametrize("shape", ["b16_b64", "b16v_b64", "str31_var"])
def test_encode_tail_is_the_inverse_of_decode_tail(rsos_hip_lib, shape):
    from rsos_hip import pack_str_keys
    from rsos_hip.snapshot import decode_tail, encode_tail
    sd, _, form = schemas(shape)
    W = key_width(SHAPES[shape][0])
    if shape.startswith("str"):
        file_keys = [b"", b"k", bytes(range(1, W))]
        assert [len(k) for k in file_keys] == [0, 1, W - 1]
        rows = [r.tobytes() for r in pack_str_keys(file_keys, W)]
    else:
        file_keys = [bytes(range(i, i + W)) for i in (0, 100)]
        rows = file_keys
    acks = {k: ({} if i == 1 else PEERS) for i, k in enumerate(rows)}
    got = encode_tail(MEMBERS, acks, sd, form, ragged=True)
    assert got == tail_bytes(shape, MEMBERS, {k: acks[r] for k, r in zip(file_keys, rows)})
    mem, back = decode_tail(bytes(16) + got, 16, sd, form, ragged=True)
    assert mem == [ipaddress.ip_address(m) for m in MEMBERS] and back == acks
    assert encode_tail([], None, sd, form) == bytes(16) == tail_bytes(shape, [], None)
    with pytest.raises(ValueError):
        encode_tail([], {b"short": {}}, sd, form)


def test_file_helper_replaces_the_file_and_leaves_no_tmp(tmp_path):
    from rsos_hip.snapshot import write_snapshot_file
    path = tmp_path / "map.rcnl"
    path.write_bytes(b"the previous snapshot, longer than the next one")
    (tmp_path / "map.rcnl.tmp").write_bytes(b"left by a crash")
    write_snapshot_file(path, b"RCNL", b"", b"-head", b"-tail")
    assert path.read_bytes() == b"RCNL-head-tail"
    assert sorted(os.listdir(tmp_path)) == ["map.rcnl"]
    write_snapshot_file(str(path), b"again")
    assert path.read_bytes() == b"again" and sorted(os.listdir(tmp_path)) == ["map.rcnl"]
    cwd = os.getcwd()
    os.chdir(tmp_path)  # a bare file name: no directory to sync
    try:
        write_snapshot_file("bare.rcnl", b"x")
    finally:
        os.chdir(cwd)
    assert (tmp_path / "bare.rcnl").read_bytes() == b"x"


# ---- GPU ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,tomb", SIZES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_encode_is_bit_exact(gpu, shape, n, tomb):
    from rsos_hip.snapshot import encode_entries_device
    recs, want = expected(shape, n, tomb)
    sd, _, form = schemas(shape)
    got, info = encode_entries_device(sd, to_cuda(host_columns(shape, recs)), form)
    assert (info.entries, info.tombstones, info.entries_end, info.keys) == (n, sum(r[2] for r in recs), len(want), n)
    assert got.numel() == len(want)
    assert got.cpu().numpy().tobytes() == want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["u64_var", "str63_var"])
def test_long_values(gpu, shape):
    """Values of 4095, 4096, 4097 and 70000 bytes (more than one LDS window) between empty values
    and tombstones."""
    from rsos_hip.snapshot import encode_entries_device
    rng = np.random.default_rng(11)
    base = gen_records(shape, 40, 0.0, seed=5, unique=True)
    lens = [4095, 0, 4096, None, 4097, 0, 70000, None, 1, 70000, 4096, None, 0, 4095]
    recs = []
    for i, r in enumerate(base):
        ln = lens[i % len(lens)] if i < 2 * len(lens) else len(r[3])
        recs.append((r[0], r[1], 1, b"") if ln is None else (r[0], r[1], 0, rng.bytes(ln)))
    data, end, _ = write_snapshot(shape, recs)
    sd, _, form = schemas(shape)
    got, info = encode_entries_device(sd, to_cuda(host_columns(shape, recs)), form)
    assert (info.entries, info.tombstones, info.entries_end) == (40, sum(r[2] for r in recs), end)
    assert got.cpu().numpy().tobytes() == data[:end]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["str31_var", "b16_b64", "u32_u32"])
def test_bounds(gpu, shape):
    from rsos_hip import _abi as A
    recs, want = expected(shape, 777, 0.25)
    end = len(want)
    cols = to_cuda(host_columns(shape, recs))
    tomb = sum(r[2] for r in recs)
    # cap = end: exact, and nothing behind it
    out = guarded(end)
    rc, info = encode_raw(shape, cols, out, end)
    assert rc == A.OK and (info.entries, info.tombstones, info.entries_end, info.keys) == (777, tomb, end, 777)
    host = out.cpu().numpy()
    assert host[:end].tobytes() == want and (host[end:] == 0xA5).all()
    # the ragged bit changes no byte
    out = guarded(end)
    rc, _ = encode_raw(shape, cols, out, end, form=FORMS[SHAPES[shape][2]] | A.FORM_RAGGED)
    assert rc == A.OK and out.cpu().numpy()[:end].tobytes() == want
    # cap = end - 1: refused, the length reported, nothing written from end - 1 on
    out = guarded(end)
    rc, info = encode_raw(shape, cols, out, end - 1)
    assert rc == A.ERR_ARG and info.entries_end == end and info.tombstones == tomb
    assert (out.cpu().numpy()[end - 1:] == 0xA5).all()
    # no output: the length only
    rc, info = encode_raw(shape, cols, None, 0)
    assert rc == A.OK and (info.entries, info.tombstones, info.entries_end, info.keys) == (777, tomb, end, 777)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["str15_var", "b16_b64"])
def test_no_tags_means_all_present(gpu, shape):
    import torch
    from rsos_hip.snapshot import encode_entries_device
    recs = gen_records(shape, 300, 0.0)
    sd, _, form = schemas(shape)
    cols = to_cuda(host_columns(shape, recs))
    assert int(cols["tags"].sum()) == 0
    with_tags, _ = encode_entries_device(sd, cols, form)
    without, info = encode_entries_device(sd, dict(cols, tags=None), form)
    assert info.tombstones == 0 and torch.equal(with_tags, without)
    assert without.cpu().numpy().tobytes() == write_snapshot(shape, recs)[0][:info.entries_end]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", DECODE_SHAPES)
def test_round_trip_through_the_decoder(gpu, shape):
    import torch
    from rsos_hip.snapshot import decode_entries_device, encode_entries_device
    recs = gen_records(shape, 777, 0.25)
    sd, _, form = schemas(shape)
    cols = to_cuda(host_columns(shape, recs))
    data, info = encode_entries_device(sd, cols, form)
    back, info2 = decode_entries_device(sd, data.clone(), form, ragged=True)
    assert (info2.entries, info2.tombstones, info2.entries_end) == (777, info.tombstones, info.entries_end)
    for k in ("keys", "phys", "logical", "node", "tags"):
        assert torch.equal(back[k], cols[k]), k
    if isinstance(cols["values"], tuple):
        assert torch.equal(back["values"][0], cols["values"][0]) and torch.equal(back["values"][1], cols["values"][1])
        offs = back["values"][1].cpu().numpy()
        assert all(offs[i] == offs[i + 1] for i, r in enumerate(recs) if r[2])
    else:
        assert torch.equal(back["values"], cols["values"])
        assert not back["values"][cols["tags"] != 0].any()


def _state(st):
    agg = st.aggregate()
    return st.size(), agg.size, agg.fingerprint.to_int()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["b16_b64", "u64_u64", "str31_var"])
def test_round_trip_through_the_reload(gpu, shape):
    """load_snapshot of the encoded bytes leaves what rh_store_load_device of the columns leaves."""
    from rsos_hip import GpuFingerprintStore
    from rsos_hip.snapshot import encode_entries_device, load_snapshot
    recs = ordered(shape, gen_records(shape, 3000, 0.2, unique=True), "sorted")
    sd, sp, form = schemas(shape)
    cols = to_cuda(host_columns(shape, recs))
    data, info = encode_entries_device(sd, cols, form)
    load_cols = dict(cols)
    if isinstance(cols["values"], tuple):
        load_cols["values"], load_cols["value_offsets"] = cols["values"]
    want = []
    for schema in (sd, sp):
        st = GpuFingerprintStore(schema)
        st.load_bulk_device(load_cols)
        want.append(_state(st))
        st.close()
    assert want[0][0] == 3000
    for ragged in (True, False) if val_width(SHAPES[shape][1]) is not None else (True,):
        dated, proj = GpuFingerprintStore(sd), GpuFingerprintStore(sp)
        got = load_snapshot(data, dated, proj, form, ragged=ragged)
        assert (got.entries, got.keys, got.tombstones, got.entries_end) == (3000, 3000, info.tombstones,
                                                                            info.entries_end)
        assert [_state(dated), _state(proj)] == want, ragged
        dated.close(), proj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["str rows", "offsets", "tags"])
def test_malformed_columns_stay_in_bounds(gpu, what):
    """The clipping the contract promises: a wrong but well-formed file of exactly n entries, and
    no byte written past it.  Every access stays inside the given buffers by construction."""
    from rsos_hip import _abi as A
    shape = "str31_var"
    n = 600
    recs = gen_records(shape, n, 0.2, seed=8)
    host = host_columns(shape, recs)
    if what == "str rows":
        keys = host["keys"].copy()
        keys[::3, 31] = 200          # a length byte above W - 1: clipped to 31
        keys[1::3, 20:31] = 0x7F     # nonzero padding: written only where the length covers it
        host["keys"] = keys
    elif what == "offsets":
        heap, offs = host["values"]
        offs = offs.copy()
        offs[100] = offs[101] + 5                # a decreasing pair
        offs[300] = heap.size + 4096             # past bytes_len (the next pair decreases too)
        offs[n] = heap.size + 10                 # the last span ends past the heap
        host["values"] = (heap, offs)
    else:
        tags = host["tags"].copy()
        tags[::5] = 7
        host["tags"] = tags
    cols = to_cuda(host)
    rc, info = encode_raw(shape, cols, None, 0)
    assert rc == A.OK
    end = int(info.entries_end)
    out = guarded(end)
    rc, info = encode_raw(shape, cols, out, end)
    assert rc == A.OK and info.entries_end == end and info.entries == n
    got = out.cpu().numpy()
    assert (got[end:] == 0xA5).all()
    parsed, _, _, pend = parse_snapshot(shape, got[:end].tobytes() + bytes(16))
    assert len(parsed) == n and pend == end
    assert info.tombstones == sum(r[2] for r in parsed)
    if what == "str rows":
        assert all(len(parsed[i][0]) == 31 for i in range(0, n, 3))
        assert [parsed[i] for i in range(2, n, 3)] == [tuple(recs[i]) for i in range(2, n, 3)]
    elif what == "tags":
        assert [r[2] for r in parsed] == [1 if (i % 5 == 0 or recs[i][2]) else 0 for i in range(n)]
    else:
        assert parsed[100][3] == b"" or parsed[100][2] == 1
        assert [parsed[i] for i in range(99)] == [tuple(recs[i]) for i in range(99)]  # (99's span ends at offs[100])


@pytest.mark.gpu
def test_save_snapshot_writes_a_file_the_reload_reads(gpu, tmp_path):
    from rsos_hip import GpuFingerprintStore, pack_str_keys
    from rsos_hip.snapshot import decode_tail, load_snapshot, save_snapshot
    shape = "str31_var"
    recs = ordered(shape, gen_records(shape, 500, 0.2, unique=True), "sorted")
    sd, sp, form = schemas(shape)
    acks = {pack_str_keys([recs[3][0]], 32)[0].tobytes(): PEERS}
    path = tmp_path / "state.rcnl"
    info = save_snapshot(path, sd, to_cuda(host_columns(shape, recs)), MEMBERS, acks, form)
    data = path.read_bytes()
    assert data == write_snapshot(shape, recs, MEMBERS, {recs[3][0]: PEERS})[0]
    assert sorted(os.listdir(tmp_path)) == ["state.rcnl"]
    mem, back = decode_tail(data, info.entries_end, sd, form, ragged=True)
    assert mem == [ipaddress.ip_address(m) for m in MEMBERS] and back == acks
    dated = GpuFingerprintStore(sd)
    got = load_snapshot(data, dated, None, form, ragged=True)
    assert (got.entries, got.keys, got.entries_end) == (500, 500, info.entries_end) and dated.size() == 500
    dated.close()
    assert struct.unpack("<Q", data[8:16])[0] == 500
