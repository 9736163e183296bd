"""RCNL v1 snapshots of string-keyed and variable-length-value maps, for tests/test_ragged_snapshot.py,
tests/test_snapshot_encode.py and the sharded reload tests: the shapes, a small writer, an independent
sequential parser, the record generators, and the check of reloaded stores against the oracle.

oracle/snapshot.py writes fixed-width entries only, so the writer here is struct packing of header,
entries and tail (tied to the oracle's bytes on the fixed shapes both can write).  Expected
fingerprints come from the oracle alone: records_common.canonical, hashed by oracle.lift_encoded.
"""
import functools
import ipaddress
import struct

import numpy as np

import snapshot as OS  # oracle/snapshot.py
from records_common import canonical, fold, key_width, val_width

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
# the shapes only the ragged route decodes
DECODE_SHAPES = ["str15_u64", "str31_unit", "str31_u32", "str15_var", "str31_var", "str63_var", "u64_var", "b16_var",
                 "b16v_var", "u32_var"]
VAL_EDGES = (0, 1, 3, 4, 5, 63, 64, 65)
MEMBERS = ["10.0.0.1", "::1", "192.168.1.20"]


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

def replay(shape, recs):
    """What the sequential replay leaves: the last record of every key, in key order."""
    last = {}
    for r in recs:
        last[r[0]] = r
    return [last[k] for k in sorted(last, key=lambda k: key_order(shape, k))]


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
        key, value, _ = SHAPES[shape]
        want = O.lift_encoded([canonical(key, value, kind, r[0], r[3], r[1], bool(r[2])) for r in kept], threads=4)
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
