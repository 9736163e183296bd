"""Snapshot reload of string-keyed and variable-length-value maps: RH_FORM_RAGGED, the
byte-granular locate (csrc/snap_ragged.hip) behind rh_store_load_snapshot and
rh_snapshot_decode_device.

oracle/snapshot.py writes fixed-width entries only, so this file carries its own small writer
(struct packing of header, entries and tail; tied to the oracle's bytes on the fixed shapes both
can write) and an independent sequential parser.  Expected fingerprints come from the oracle
alone: canonical bytes from oracle/pyref.py's typed model, hashed by oracle.lift_encoded.
"""
import ctypes as C
import functools
import ipaddress
import struct

import numpy as np
import pytest

import pyref as P      # oracle/pyref.py
import snapshot as OS  # oracle/snapshot.py

MOD = 1 << 256
# name -> (key, value, key form in the file)
SHAPES = {
    "str15_u64": ("str15", "u64", "vec"), "str31_unit": ("str31", "unit", "vec"), "str31_u32": ("str31", "u32", "vec"),
    "str31_u64": ("str31", "u64", "vec"),
    "str15_var": ("str15", "var", "vec"), "str31_var": ("str31", "var", "vec"), "str63_var": ("str63", "var", "vec"),
    "u64_var": ("u64", "var", "array"), "b16_var": ("bytes16", "var", "array"), "b16v_var": ("bytes16", "var", "vec"),
    "u32_var": ("u32", "var", "array"),
    "b16_b64": ("bytes16", "bytes64", "array"), "b16v_b64": ("bytes16", "bytes64", "vec"),
    "u64_u64": ("u64", "u64", "array"), "u32_u32": ("u32", "u32", "array"), "b16_b1024": ("bytes16", "bytes1024", "array"),
}
VAL_EDGES = (0, 1, 3, 4, 5, 63, 64, 65)
MEMBERS = ["10.0.0.1", "::1", "192.168.1.20"]


def key_width(key):  # bytes of a key column row
    return {"u32": 4, "u64": 8}.get(key) or (int(key[3:]) + 1 if key.startswith("str") else int(key[5:]))


def val_width(value):  # bytes of a fixed value; None: per record
    return {"unit": 0, "u32": 4, "u64": 8, "var": None}.get(value, int(value[5:]) if value.startswith("bytes") else 0)


# ---- the writer -------------------------------------------------------------------------------
# a record: (key bytes as the file holds them behind any length, (phys, logical, node), tomb, value bytes)

def entry_bytes(shape, rec) -> bytes:
    key, value, form = SHAPES[shape]
    k, stamp, tomb, v = rec
    out = (struct.pack("<Q", len(k)) if key.startswith("str") or form == "vec" else b"") + k
    out += struct.pack("<QIQ", *stamp) + struct.pack("<I", 1 if tomb else 0)
    if not tomb:
        out += (struct.pack("<Q", len(v)) if value == "var" or value.startswith("bytes") else b"") + v
    return out


def tail_bytes(shape, members=(), acks=None) -> bytes:
    key, _, form = SHAPES[shape]

    def ip(a):
        a = ipaddress.ip_address(a)
        return struct.pack("<I", 0 if a.version == 4 else 1) + a.packed
    out = struct.pack("<Q", len(members)) + b"".join(ip(m) for m in members)
    acks = acks or {}
    out += struct.pack("<Q", len(acks))
    for k, peers in acks.items():
        out += (struct.pack("<Q", len(k)) if key.startswith("str") or form == "vec" else b"") + bytes(k)
        out += struct.pack("<Q", len(peers)) + b"".join(ip(a) + struct.pack("<Q", ver) for a, ver in peers.items())
    return out


def write_snapshot(shape, recs, members=MEMBERS, acks=None, tail=True, count=None):
    """(file bytes, entries_end, start offset of every entry)."""
    parts, starts, p = [b"RCNL" + struct.pack("<IQ", 1, len(recs) if count is None else count)], [], 16
    for r in recs:
        e = entry_bytes(shape, r)
        starts.append(p)
        parts.append(e)
        p += len(e)
    if tail:
        parts.append(tail_bytes(shape, members, acks))
    return b"".join(parts), p, starts


# ---- the sequential parser --------------------------------------------------------------------

def parse_snapshot(shape, data):
    """(records, members, acks, entries_end); ValueError as the reference's decode."""
    key, value, form = SHAPES[shape]
    W, vw = key_width(key), val_width(value)
    OS.check_header(data)
    r = OS._R(bytes(data), 8)

    def rd_key():
        if key.startswith("str"):
            L = r.u64()
            if L > W - 1:
                raise ValueError(f"key length {L} does not fit a row of {W}")
            return r.take(L)
        if form == "vec" and r.u64() != W:
            raise ValueError("key length differs from the schema's")
        return r.take(W)
    recs = []
    for _ in range(r.u64()):
        k = rd_key()
        stamp = (r.u64(), r.u32(), r.u64())
        var = r.u32()
        if var > 1:
            raise ValueError(f"invalid value: integer `{var}`, expected variant index 0 <= i < 2")
        v = b""
        if var == 0:
            if value == "var":
                v = r.take(r.u64())
            elif value.startswith("bytes"):
                if r.u64() != vw:
                    raise ValueError("value length differs from the schema's")
                v = r.take(vw)
            else:
                v = r.take(vw)
        recs.append((k, stamp, var, v))
    end = r.p
    members = [r.ip() for _ in range(r.u64())]
    acks = {}
    for _ in range(r.u64()):
        k = rd_key()
        acks[k] = {}
        for _ in range(r.u64()):
            a = r.ip()
            acks[k][a] = r.u64()
    return recs, members, acks, end


# ---- case generators --------------------------------------------------------------------------

def gen_key(rng, key, i, unique=None):
    """Record i's key bytes: a string of i % W bytes, or a fixed-width key; unique: a set to stay out of."""
    W = key_width(key)
    while True:
        if key.startswith("str"):
            L = i % W if unique is None else int(rng.integers(0, W))
            k = rng.bytes(L)
        else:
            k = rng.bytes(W)
        if unique is None or k not in unique:
            if unique is not None:
                unique.add(k)
            return k


def gen_value(rng, value, i):
    vw = val_width(value)
    if vw is not None:
        return rng.bytes(vw)
    return rng.bytes(VAL_EDGES[i] if i < len(VAL_EDGES) else int(rng.integers(0, 301)))


@functools.lru_cache(maxsize=None)
def gen_records(shape, n, tomb, seed=0, unique=False):
    """n records in generation order; tomb: the share of tombstones (1.0: all)."""
    key, value, _ = SHAPES[shape]
    rng = np.random.default_rng(1000 * n + 17 * seed + sum(shape.encode()))
    seen = set() if unique else None
    recs = []
    for i in range(n):
        t = 1 if tomb >= 1.0 or rng.random() < tomb else 0
        stamp = (1_700_000_000_000 + int(rng.integers(0, 1 << 30)), int(rng.integers(0, 1 << 32)),
                 int(rng.integers(0, 1 << 63)))
        v = gen_value(rng, value, i)
        recs.append((gen_key(rng, key, i, seen), stamp, t, b"" if t else v))
    return tuple(recs)


def key_order(shape, k):
    key = SHAPES[shape][0]
    return int.from_bytes(k, "little") if key in ("u32", "u64") else k


def ordered(shape, recs, order, seed=3):
    """sorted / shuffled / repeats (5 % of the rows take another row's key: the last wins)."""
    recs = sorted(recs, key=lambda r: key_order(shape, r[0]))
    if order == "sorted":
        return recs
    rng = np.random.default_rng(seed)
    if order == "repeats":
        n = len(recs)
        for s, d in zip(rng.integers(0, n, n // 20), rng.integers(0, n, n // 20)):
            recs[d] = (recs[s][0],) + recs[d][1:]
    return [recs[i] for i in rng.permutation(len(recs))]


# ---- expectations from the oracle -------------------------------------------------------------

def canonical(shape, kind, rec) -> bytes:
    key, value, _ = SHAPES[shape]
    k, stamp, tomb, v = rec
    ck = {"u32": lambda: P.U32(int.from_bytes(k, "little")), "u64": lambda: P.U64(int.from_bytes(k, "little"))}.get(
        key, lambda: P.Str(k))()
    cv = {"unit": lambda: P.Unit(), "u32": lambda: P.U32(int.from_bytes(v, "little")),
          "u64": lambda: P.U64(int.from_bytes(v, "little"))}.get(value, lambda: P.Str(v))()
    state = P.TOMBSTONE if tomb else P.present(cv)
    return P.encode(ck) + P.encode(P.entry(P.timestamp(*stamp), state) if kind == "dated" else state)


def replay(shape, recs):
    """What the sequential replay leaves: the last record of every key, in key order."""
    last = {}
    for r in recs:
        last[r[0]] = r
    return [last[k] for k in sorted(last, key=lambda k: key_order(shape, k))]


def fold(fps) -> int:
    return sum(int.from_bytes(bytes(f), "little") for f in fps) % MOD


def schemas(shape):
    from rsos_hip import RecordSchema
    key, value, form = SHAPES[shape]
    return RecordSchema.dated(key, value), RecordSchema.projection(key, value), form


def api_key(shape, k):
    return int.from_bytes(k, "little") if SHAPES[shape][0] in ("u32", "u64") else k


def check_stores(O, shape, recs, info, dated, proj, n_entries):
    """Both stores against the oracle's lift of the replayed records."""
    from rsos_hip.store import KeyRange
    kept = replay(shape, recs)
    assert info.entries == n_entries and info.keys == len(kept)
    assert info.tombstones == sum(r[2] for r in recs[:n_entries])
    ks = [api_key(shape, r[0]) for r in kept]
    for st, kind in ((dated, "dated"), (proj, "projection")):
        if st is None:
            continue
        want = O.lift_encoded([canonical(shape, kind, r) for r in kept], threads=4)
        assert st.size() == len(kept)
        assert [k for k, _ in st.enumerate()] == ks
        assert np.array_equal(st.fingerprints(), want), kind
        assert st.aggregate().fingerprint.to_int() == fold(want) and st.aggregate().size == len(kept)
        m = len(kept)
        for lo, hi in ((0, m // 3), (m // 3, m - 1), (m // 2, m // 2 + 1)) if m > 3 else ():
            got = st.aggregate(KeyRange(ks[lo], ks[hi], "included", "excluded"))
            assert (got.size, got.fingerprint.to_int()) == (hi - lo, fold(want[lo:hi])), (lo, hi)


def to_dev(data):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()


def reload_and_check(O, shape, recs, data, end, stores="both", device=False, n_entries=None):
    from rsos_hip import GpuFingerprintStore
    from rsos_hip.snapshot import load_snapshot
    sd, sp, form = schemas(shape)
    dated = GpuFingerprintStore(sd) if stores in ("both", "dated") else None
    proj = GpuFingerprintStore(sp) if stores in ("both", "projection") else None
    info = load_snapshot(to_dev(data) if device else data, dated, proj, form, ragged=True)
    assert info.entries_end == end
    check_stores(O, shape, recs, info, dated, proj, len(recs) if n_entries is None else n_entries)
    for st in (dated, proj):
        if st is not None:
            st.close()
    return info


def key_rows(shape, recs):
    from rsos_hip import pack_str_keys
    key = SHAPES[shape][0]
    W = key_width(key)
    if key.startswith("str"):
        return pack_str_keys([r[0] for r in recs], W)
    return np.frombuffer(b"".join(r[0] for r in recs), np.uint8).reshape(len(recs), W)


def decode_and_check(shape, recs, data, end):
    from rsos_hip.snapshot import decode_entries_device
    sd, _, form = schemas(shape)
    n = len(recs)
    got, info = decode_entries_device(sd, to_dev(data), form, ragged=True)
    assert (info.entries, info.tombstones, info.entries_end) == (n, sum(r[2] for r in recs), end)
    assert np.array_equal(got["keys"].cpu().numpy(), key_rows(shape, recs))
    assert np.array_equal(got["phys"].cpu().numpy().view(np.uint64), np.array([r[1][0] for r in recs], np.uint64))
    assert np.array_equal(got["logical"].cpu().numpy().view(np.uint32), np.array([r[1][1] for r in recs], np.uint32))
    assert np.array_equal(got["node"].cpu().numpy().view(np.uint64), np.array([r[1][2] for r in recs], np.uint64))
    assert np.array_equal(got["tags"].cpu().numpy(), np.array([r[2] for r in recs], np.uint8))
    vw = val_width(SHAPES[shape][1])
    if vw is None:
        heap, offs = got["values"]
        want = np.zeros(n + 1, np.int64)
        want[1:] = np.cumsum([len(r[3]) for r in recs])
        assert np.array_equal(offs.cpu().numpy(), want)
        assert heap.cpu().numpy().tobytes() == b"".join(r[3] for r in recs)
    else:
        want = np.frombuffer(b"".join(r[3] if not r[2] else bytes(vw) for r in recs), np.uint8).reshape(n, vw)
        assert np.array_equal(got["values"].cpu().numpy(), want)


# ---- CPU --------------------------------------------------------------------------------------

DECODE_SHAPES = ["str15_u64", "str31_unit", "str31_u32", "str15_var", "str31_var", "str63_var", "u64_var", "b16_var",
                 "b16v_var", "u32_var"]
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
