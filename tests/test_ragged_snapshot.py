"""Snapshot reload of string-keyed and variable-length-value maps: RH_FORM_RAGGED, the
byte-granular locate (csrc/snap_ragged.hip) behind rh_store_load_snapshot and
rh_snapshot_decode_device.

oracle/snapshot.py writes fixed-width entries only, so tests/ragged_snapshot_common.py carries a
small writer (tied here to the oracle's bytes on the fixed shapes both can write) and an
independent sequential parser.  Expected fingerprints come from the oracle alone: canonical bytes
from oracle/pyref.py's typed model (records_common.canonical), hashed by oracle.lift_encoded.
"""
import ctypes as C
import ipaddress
import struct

import numpy as np
import pytest

import snapshot as OS  # oracle/snapshot.py
from ragged_snapshot_common import (DECODE_SHAPES, MEMBERS, SHAPES, VAL_EDGES, check_stores, decode_and_check, entry_bytes, gen_records,
                                    key_rows, ordered, parse_snapshot, reload_and_check, schemas, to_dev, write_snapshot)
from records_common import key_width, val_width

# ---- CPU --------------------------------------------------------------------------------------

SIZES = [(0, 0.0), (1, 0.0), (1, 1.0), (777, 0.25), (20000, 0.1), (5000, 1.0)]


@pytest.mark.parametrize("shape", DECODE_SHAPES + ["str31_u64", "b16_b64", "u32_u32"])
def test_writer_and_parser_round_trip(shape):
    """Every generator used below: what the writer wrote, the sequential parser reads back."""
    for n, tomb in ((0, 0.0), (1, 1.0), (777, 0.25)):
        for recs in (list(gen_records(shape, n, tomb)), ordered(shape, gen_records(shape, n, tomb, unique=True), "repeats")):
            acks = {recs[0][0]: {ipaddress.ip_address("10.0.0.1"): 7}} if recs else {}
            data, end, starts = write_snapshot(shape, recs, MEMBERS, acks)
            got, mem, ak, e2 = parse_snapshot(shape, data)
            assert got == [(k, s, t, v) for k, s, t, v in recs] and e2 == end
            assert mem == [ipaddress.ip_address(m) for m in MEMBERS] and ak == acks
            assert len(starts) == n and (not n or starts[0] == 16)
    key, value, _ = SHAPES[shape]
    recs = gen_records(shape, 777, 0.25)
    if key.startswith("str"):
        assert {len(r[0]) for r in recs} == set(range(key_width(key)))
    if value == "var":
        lens = {len(r[3]) for r in gen_records(shape, 777, 0.0)}
        assert set(VAL_EDGES) <= lens and max(lens) > 250


@pytest.mark.parametrize("shape", ["b16_b64", "b16v_b64", "u32_u32"])
def test_writer_equals_the_oracle_writer(shape):
    key, value, form = SHAPES[shape]
    recs = gen_records(shape, 300, 0.3)
    n = len(recs)
    vw = val_width(value)
    acks = {recs[5][0]: {ipaddress.ip_address("10.0.0.1"): 77},
            recs[9][0]: {ipaddress.ip_address("::1"): 2**40, ipaddress.ip_address("10.0.0.2"): 1}}
    want = OS.encode_snapshot(key_rows(shape, recs), np.array([r[1][0] for r in recs], np.uint64),
                              np.array([r[1][1] for r in recs], np.uint32), np.array([r[1][2] for r in recs], np.uint64),
                              np.array([r[2] for r in recs], np.uint8),
                              np.frombuffer(b"".join(r[3] or bytes(vw) for r in recs), np.uint8).reshape(n, vw),
                              {"u32": "u32", "u64": "u64"}.get(key, form), {"u32": "u32", "u64": "u64"}.get(value, "bytes"),
                              MEMBERS, acks)
    assert write_snapshot(shape, recs, MEMBERS, acks)[0] == want


def test_tail_decoder_reads_string_ack_keys(rsos_hip_lib):
    from rsos_hip import RecordSchema, pack_str_keys, _abi as A
    from rsos_hip.snapshot import decode_tail
    recs = list(gen_records("str31_var", 50, 0.5))
    peers = {ipaddress.ip_address("10.1.2.3"): 5, ipaddress.ip_address("fe80::1"): 2**40}
    ack_keys = [b"", b"k", bytes(range(1, 32)), b"node-7"]
    acks = {k: peers for k in ack_keys}
    data, end, _ = write_snapshot("str31_var", recs, MEMBERS, acks)
    schema = RecordSchema.dated("str31", "var")
    mem, got = decode_tail(data, end, schema, "vec", ragged=True)
    assert mem == [ipaddress.ip_address(m) for m in MEMBERS]
    assert got == {pack_str_keys([k], 32)[0].tobytes(): peers for k in ack_keys}
    assert [len(k) for k in ack_keys[:3]] == [0, 1, 31]
    bad, end, _ = write_snapshot("str31_var", recs, MEMBERS, {b"x" * 32: peers})
    with pytest.raises(A.RsosHipError) as e:
        decode_tail(bad, end, schema, "vec", ragged=True)
    assert e.value.code == A.ERR_DATA


# ---- GPU --------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,tomb", SIZES)
@pytest.mark.parametrize("shape", DECODE_SHAPES)
def test_decode_equals_source(gpu, shape, n, tomb):
    recs = gen_records(shape, n, tomb)
    acks = {recs[0][0]: {ipaddress.ip_address("10.0.0.1"): 7}} if recs else {}
    data, end, _ = write_snapshot(shape, recs, MEMBERS, acks)
    assert len(data) > end
    decode_and_check(shape, recs, data, end)


@pytest.mark.gpu
@pytest.mark.parametrize("stores", ["dated", "projection", "both"])
@pytest.mark.parametrize("order", ["sorted", "shuffled", "repeats"])
@pytest.mark.parametrize("shape", ["str15_var", "str31_u64", "str63_var", "u64_var"])
def test_reload_equals_the_oracle(gpu, oracle_lib, shape, order, stores):
    recs = ordered(shape, gen_records(shape, 3000, 0.2, unique=True), order)
    data, end, _ = write_snapshot(shape, recs)
    for device in (False, True):
        info = reload_and_check(oracle_lib, shape, recs, data, end, stores, device)
        assert (info.keys < 3000) == (order == "repeats")


def _state(st):
    return st.size(), st.aggregate().fingerprint.to_int(), [k for k, _ in st.enumerate()], st.fingerprints().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["b16_b64", "b16v_b64", "u64_u64", "u32_u32", "b16_b1024"])
def test_both_routes_agree(gpu, shape):
    """The flag-set reload of a file both routes can read leaves what the flag-clear reload leaves."""
    from rsos_hip import GpuFingerprintStore
    from rsos_hip.snapshot import load_snapshot, ragged_stats
    recs = ordered(shape, gen_records(shape, 20000, 0.1, unique=True), "shuffled")
    data, end, _ = write_snapshot(shape, recs)
    sd, sp, form = schemas(shape)
    states = []
    for ragged in (False, True):
        dated, proj = GpuFingerprintStore(sd), GpuFingerprintStore(sp)
        info = load_snapshot(to_dev(data), dated, proj, form, ragged=ragged)
        assert (info.entries, info.keys, info.entries_end) == (20000, 20000, end)
        assert info.tombstones == sum(r[2] for r in recs)
        states.append((_state(dated), _state(proj)))
        dated.close(), proj.close()
    assert states[0] == states[1] and states[0][0][0] == 20000
    assert ragged_stats()["segments"] == -(-len(data) // ragged_stats()["segment_bytes"])


def _filler(rng, i, vlen):
    return (b"fill-%d" % i, (1_700_000_000_000 + i, i, 7), 0, rng.bytes(vlen))


@pytest.mark.gpu
def test_segment_boundaries(gpu, oracle_lib):
    """Entries that start just before, at and just after a segment boundary (the staged overlap is
    103 bytes for str31 -> var), a value the chain passes three segments over, a value of exactly
    one segment, and a file whose last entry ends at a boundary with nothing behind it."""
    from rsos_hip.snapshot import ragged_stats
    S = ragged_stats()["segment_bytes"]
    shape = "str31_var"
    rng = np.random.default_rng(5)
    base = list(gen_records(shape, 400, 0.2, seed=9, unique=True))
    recs, pos, hit = [], 16, []

    def add(r):
        nonlocal pos
        recs.append(r)
        pos += len(entry_bytes(shape, r))
    it = iter(base)
    for j, delta in enumerate((-103, -40, -9, -8, -1, 0, 1)):
        for _ in range(5):
            add(next(it))
        # a filler whose value makes the entry after it start at a boundary + delta
        head = len(entry_bytes(shape, _filler(rng, j, 0)))
        target = (pos + head + 200 + S - 1) // S * S + S + delta
        add(_filler(rng, j, target - pos - head))
        assert pos == target
        hit.append(pos % S)
        add(next(it))
    assert hit == [S - 103, S - 40, S - 9, S - 8, S - 1, 0, 1]
    add(_filler(rng, 100, 3 * S))   # the chain passes over at least two whole segments
    for _ in range(5):
        add(next(it))
    add(_filler(rng, 101, S))
    for r in it:
        add(r)
    data, end, _ = write_snapshot(shape, recs)
    decode_and_check(shape, recs, data, end)
    reload_and_check(oracle_lib, shape, recs, data, end, "both", True)
    # the last entry ends exactly at a boundary, and the file with it
    head = len(entry_bytes(shape, _filler(rng, 102, 0)))
    last = _filler(rng, 102, (pos + head + S - 1) // S * S - pos - head)
    data, end, _ = write_snapshot(shape, recs + [last], tail=False)
    assert end == len(data) and end % S == 0
    decode_and_check(shape, recs + [last], data, end)
    reload_and_check(oracle_lib, shape, recs + [last], data, end, "both", True)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["zeros", "copy"])
def test_values_that_parse_as_entries(gpu, oracle_lib, what):
    """A value of zero bytes (every position in it is a valid empty-key, empty-value entry) and a
    value that is a verbatim copy of 200 real entries of the same file: the answer does not depend
    on what values hold; the zero run costs fix-up rounds, one per segment it spans."""
    from rsos_hip.snapshot import ragged_stats
    S = ragged_stats()["segment_bytes"]
    shape = "str31_var"
    recs = list(gen_records(shape, 2000, 0.2, seed=21, unique=True))
    if what == "zeros":
        trap = (b"zero-run", (1_700_000_000_001, 1, 2), 0, bytes(3 * S))
    else:
        trap = (b"copy", (1_700_000_000_001, 1, 2), 0, b"".join(entry_bytes(shape, r) for r in recs[600:800]))
    recs.insert(500, trap)
    data, end, starts = write_snapshot(shape, recs)
    decode_and_check(shape, recs, data, end)
    reload_and_check(oracle_lib, shape, recs, data, end, "both", True)
    st = ragged_stats()
    assert st["segment_bytes"] == S and st["segments"] == -(-len(data) // S) and st["rounds"] >= 1
    if what == "zeros":
        v0 = starts[501] - 3 * S
        spans = (starts[501] - 1) // S - v0 // S + 1
        assert st["rewalked"] > 0 and 2 <= st["rounds"] <= spans + 2, (st, spans)


def _other_contents(O):
    from rsos_hip import GpuFingerprintStore
    from rsos_hip.snapshot import load_snapshot
    shape = "str31_var"
    recs = ordered(shape, gen_records(shape, 1500, 0.1, seed=33, unique=True), "sorted")
    data, end, _ = write_snapshot(shape, recs)
    sd, sp, form = schemas(shape)
    dated, proj = GpuFingerprintStore(sd), GpuFingerprintStore(sp)
    load_snapshot(data, dated, proj, form, ragged=True)
    return dated, proj


def _damaged(shape, recs, k):
    """name -> (file bytes, the damaged entry's own bytes): entry k damaged in the ways a file can be."""
    data, end, starts = write_snapshot(shape, recs)
    n = len(recs)
    out = {}
    voff = starts[k] + 8 + len(recs[k][0]) + 20  # the State variant of entry k
    assert not recs[k][2] and len(recs[k][3]) > 0
    b = bytearray(data)
    b[voff:voff + 4] = struct.pack("<I", 2)
    out["variant 2"] = bytes(b)
    long_key = (b"k" * 32,) + recs[k][1:]
    out["key length 32"] = write_snapshot(shape, recs[:k] + [long_key] + recs[k + 1:])[0]
    b = bytearray(data)
    b[starts[k]:starts[k] + 8] = struct.pack("<Q", 1 << 40)
    out["key length 2^40"] = bytes(b)
    b = bytearray(data)
    b[voff + 4:voff + 12] = struct.pack("<Q", len(data))
    out["value past the end"] = bytes(b)
    out["count n + 1"] = write_snapshot(shape, recs, tail=False, count=n + 1)[0]
    cut = starts[n - 1] + 8 + len(recs[n - 1][0]) + 11
    out["cut in a stamp"] = data[:cut]
    entry = {name: out[name][starts[k]:starts[k + 1]] for name in ("variant 2", "key length 2^40", "value past the end")}
    entry["key length 32"] = entry_bytes(shape, long_key)
    entry["cut in a stamp"] = data[starts[n - 1]:cut]
    return out, entry


@pytest.mark.gpu
def test_corrupt_files_change_nothing(gpu, oracle_lib):
    from rsos_hip import _abi as A
    from rsos_hip.snapshot import load_snapshot
    shape = "str31_var"
    recs = [r for r in gen_records(shape, 1200, 0.0, seed=41, unique=True)]
    k = next(i for i in range(700, 1200) if len(recs[i][3]) > 0)
    files, entries = _damaged(shape, recs, k)
    dated, proj = _other_contents(oracle_lib)
    before = (_state(dated), _state(proj))
    assert before[0][0] == 1500
    for name, blob in files.items():
        with pytest.raises(ValueError):
            parse_snapshot(shape, blob)
        for src in (blob, to_dev(blob)):
            with pytest.raises(A.RsosHipError) as e:
                load_snapshot(src, dated, proj, "vec", ragged=True)
            assert e.value.code == A.ERR_DATA, (name, str(e.value))
            if name == "key length 32":
                assert f"entry {k}" in str(e.value) and "32" in str(e.value)
            if name in ("count n + 1", "cut in a stamp"):
                assert "unexpected end of file" in str(e.value)
            assert (_state(dated), _state(proj)) == before, name
    # the same bytes behind the n-th entry are not entries: no error, and entries_end is exact
    good, end, _ = write_snapshot(shape, recs, tail=False)
    for name, junk in entries.items():
        info = reload_and_check(oracle_lib, shape, recs, good + junk, end, "both", True)
        assert info.entries == len(recs), name
    dated.close(), proj.close()


@pytest.mark.gpu
def test_argument_errors(gpu):
    import torch
    from rsos_hip import GpuFingerprintStore, RecordSchema, _abi as A
    from rsos_hip.snapshot import load_snapshot
    recs = list(gen_records("str31_var", 100, 0.1, seed=2, unique=True))
    data, end, _ = write_snapshot("str31_var", recs)
    sd, sp, _ = schemas("str31_var")
    dated, proj = GpuFingerprintStore(sd), GpuFingerprintStore(sp)
    with pytest.raises(A.RsosHipError) as e:  # string keys are Vec keys in the file
        load_snapshot(data, dated, proj, "array", ragged=True)
    assert e.value.code == A.ERR_ARG
    other = GpuFingerprintStore(RecordSchema.projection("str15", "var"))
    with pytest.raises(A.RsosHipError) as e:
        load_snapshot(data, dated, other, "vec", ragged=True)
    assert e.value.code == A.ERR_ARG
    assert dated.size() == 0 == proj.size()
    # key_form takes 0..3
    fd = GpuFingerprintStore(RecordSchema.dated("bytes16", "bytes64"))
    frecs = list(gen_records("b16_b64", 10, 0.0))
    fdata = write_snapshot("b16_b64", frecs)[0]
    buf = np.frombuffer(fdata, np.uint8).copy()
    info = A.SnapshotInfo()
    for form, want in ((4, A.ERR_ARG), (-1, A.ERR_ARG), (A.FORM_ARRAY | A.FORM_RAGGED, A.OK)):
        rc = A.lib().rh_store_load_snapshot(fd._h, None, form, buf.ctypes.data, buf.size, 0, C.byref(info), None)
        assert rc == want, form
        if want != A.OK:
            assert b"bad key_form" in A.lib().rh_last_error()
    assert fd.size() == 10
    # a value heap one byte too small
    total = sum(len(r[3]) for r in recs)
    while total % 4 != 1:  # so that total - 1 is a heap size the contract allows
        recs.append((b"pad-%d" % total, (1, 2, 3), 0, b"v"))
        total += 1
    data, end, _ = write_snapshot("str31_var", recs)
    dev = to_dev(data)
    n = len(recs)
    cols = {"keys": torch.empty((n, 32), dtype=torch.uint8, device=gpu), "phys": torch.empty(n, dtype=torch.int64, device=gpu),
            "logical": torch.empty(n, dtype=torch.int32, device=gpu), "node": torch.empty(n, dtype=torch.int64, device=gpu),
            "tags": torch.empty(n, dtype=torch.uint8, device=gpu)}
    offs = torch.empty(n + 1, dtype=torch.int64, device=gpu)
    s = sd.c()
    for cap, want in ((total - 1, A.ERR_ARG), (total + 3, A.OK)):
        heap = torch.zeros(cap, dtype=torch.uint8, device=gpu)
        var = A.VarValues(heap.data_ptr(), offs.data_ptr(), cap)
        c = A.Columns(cols["keys"].data_ptr(), cols["phys"].data_ptr(), cols["logical"].data_ptr(),
                      cols["node"].data_ptr(), cols["tags"].data_ptr(), C.addressof(var))
        rc = A.lib().rh_snapshot_decode_device(C.byref(s), A.FORM_VEC | A.FORM_RAGGED, dev.data_ptr(), dev.numel(),
                                               C.byref(c), n, C.byref(info), None)
        torch.cuda.synchronize()
        assert rc == want, (cap, A.lib().rh_last_error())
    assert heap[:total].cpu().numpy().tobytes() == b"".join(r[3] for r in recs) and int(offs[n]) == total
    for st in (dated, proj, other, fd):
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("point", ["snapshot.load_begin", "snapshot.load_finish"])
def test_reload_failure_leaves_both_stores_empty(gpu, oracle_lib, point):
    from rsos_hip import _abi as A
    from rsos_hip.snapshot import load_snapshot
    dated, proj = _other_contents(oracle_lib)
    shape = "str31_var"
    recs = ordered(shape, gen_records(shape, 2500, 0.1, seed=51, unique=True), "shuffled")
    data, end, _ = write_snapshot(shape, recs)
    A.lib().rh_debug_fail_point(point.encode())
    with pytest.raises(A.RsosHipError) as e:
        load_snapshot(data, dated, proj, "vec", ragged=True)
    assert e.value.code == A.ERR_OOM and "injected" in str(e.value)
    for st in (dated, proj):
        agg = st.aggregate()
        assert st.size() == 0 and agg.size == 0 and agg.fingerprint.to_int() == 0
    info = load_snapshot(data, dated, proj, "vec", ragged=True)
    assert info.entries_end == end
    check_stores(oracle_lib, shape, recs, info, dated, proj, len(recs))
    dated.close(), proj.close()
