"""Snapshot reload onto the GPU, and snapshot save from it.

The load side of FileSnapshot (src/snapshot.rs:30-98) and the replay that follows it in
ReplicatedMap::with_persistence (src/replicated_map/persistence.rs:108-143): every entry of
PersistedState.entries (lww-register/src/persistence.rs:32,62-70) is inserted into the dated
map and its value-only projection (just_insert_bulk, src/replica/write.rs:107-121).

On the GPU the entries are located and decoded by librsos_hip.so (rh_store_load_snapshot:
a parallel walk over the bincode entry Vec, then a column scatter), both stores are lifted and
summed from the decoded columns, and a key that appears twice keeps its last entry -- what the
sequential replay leaves.  PersistedState.members and .tombstone_acks, which follow the entries
in the file, are host state; `decode_tail` reads them on the host.

Entries whose lengths are in their own bytes -- String keys (RH_KEY_STR stores) and Vec<u8> /
String values (VARBYTES) -- take the byte-granular locate: `ragged=True` (RH_FORM_RAGGED).

The save side (FileSnapshot::save, src/snapshot.rs:164-189, driven by snapshot_inner,
src/replicated_map/persistence.rs:155-187): `encode_entries_device` turns device columns into the
file's header and entries on the GPU (rh_snapshot_encode_device), `encode_tail` is `decode_tail`'s
inverse on the host, and `save_snapshot` writes the file the way the reference does (a sibling
temporary file, fsync, rename, fsync of the directory).

Errors are the reference's: a short file, a wrong magic or format version, or entries that do
not parse raise RsosHipError with code ERR_DATA (io::ErrorKind::InvalidData) -- never a
silent fresh start (persistence.rs:111-114).
"""
from __future__ import annotations

import ctypes as C
import ipaddress
import os
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _abi as A
from .schema import RecordSchema

_FORMS = {"array": A.FORM_ARRAY, "vec": A.FORM_VEC}


@dataclass(frozen=True)
class SnapshotInfo:
    entries: int       # PersistedState.entries.len()
    tombstones: int    # entries holding State::Tombstone
    entries_end: int   # file offset of PersistedState.members
    keys: int          # distinct keys loaded

    @staticmethod
    def from_c(i: A.SnapshotInfo) -> "SnapshotInfo":
        return SnapshotInfo(int(i.entries), int(i.tombstones), int(i.entries_end), int(i.keys))


def _host_buffer(data) -> Tuple[int, int, object]:
    a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    return (a.ctypes.data if a.size else None), a.size, a


def read_header(data, length: Optional[int] = None) -> int:
    """Validate the RCNL header of the file's first bytes; returns the entry count.  `length`:
    the whole file's length when `data` holds only its start."""
    head = bytes(np.asarray(data[:16], np.uint8).tobytes() if not isinstance(data, (bytes, bytearray, memoryview))
                 else bytes(data[:16]))
    buf = C.create_string_buffer(head, max(len(head), 1))
    out = C.c_uint64()
    A.check(A.lib().rh_snapshot_header(buf, len(data) if length is None else length, C.byref(out)),
            "rh_snapshot_header")
    return int(out.value)


def _form(key_form: str, ragged: bool) -> int:
    return _FORMS[key_form] | (A.FORM_RAGGED if ragged else 0)


def ragged_stats() -> Dict[str, int]:
    """The calling thread's last ragged decode or reload (rh_debug_ragged_stats)."""
    w = [C.c_uint64() for _ in range(4)]
    A.check(A.lib().rh_debug_ragged_stats(*[C.byref(x) for x in w]), "rh_debug_ragged_stats")
    return dict(zip(("segment_bytes", "segments", "rounds", "rewalked"), (int(x.value) for x in w)))


def load_snapshot(data, dated=None, projection=None, key_form: str = "array", ragged: bool = False) -> SnapshotInfo:
    """Replace the contents of the dated and / or projection GpuFingerprintStore with the
    snapshot's entries.  `data`: the file's bytes on the host (bytes / bytearray / memoryview /
    numpy), or a contiguous uint8 torch tensor already in HBM.  `ragged`: the byte-granular
    locate, which string-keyed stores (key_form "vec") and VARBYTES stores need."""
    if dated is None and projection is None:
        raise ValueError("no store given")
    info = A.SnapshotInfo()
    is_dev = hasattr(data, "is_cuda") and data.is_cuda
    if is_dev:
        if not data.is_contiguous():
            raise ValueError("device snapshot must be contiguous")
        ptr, size, keep = data.data_ptr(), data.numel() * data.element_size(), data
    else:
        ptr, size, keep = _host_buffer(data)
    stream = None
    if is_dev:
        import torch
        stream = torch.cuda.current_stream(data.device).cuda_stream
    A.check(A.lib().rh_store_load_snapshot(dated._h if dated is not None else None,
                                           projection._h if projection is not None else None,
                                           _form(key_form, ragged), ptr, size, 1 if is_dev else 0, C.byref(info),
                                           stream),
            "rh_store_load_snapshot")
    del keep
    return SnapshotInfo.from_c(info)


def decode_entries_device(schema: RecordSchema, data, key_form: str = "array", ragged: bool = False):
    """Decode a device-resident snapshot's entries into device columns (keys, phys, logical,
    node, tags, values); returns (columns, SnapshotInfo).  With a VARBYTES schema (`ragged` only)
    `values` is (heap, offsets): the values packed in file order, a tombstone's span empty."""
    import torch
    if not (data.is_cuda and data.is_contiguous() and data.dtype == torch.uint8):
        raise ValueError("data must be a contiguous uint8 device tensor")
    n = read_header(data[:16].cpu().numpy(), data.numel())
    dev = data.device
    cols = {
        "keys": torch.empty((n, schema.key_row), dtype=torch.uint8, device=dev),
        "phys": torch.empty(n, dtype=torch.int64, device=dev),
        "logical": torch.empty(n, dtype=torch.int32, device=dev),
        "node": torch.empty(n, dtype=torch.int64, device=dev),
        "tags": torch.empty(n, dtype=torch.uint8, device=dev),
        "values": torch.empty((n, schema.value_row), dtype=torch.uint8, device=dev),
    }
    c = A.Columns(*[cols[k].data_ptr() if cols[k].numel() else None
                    for k in ("keys", "phys", "logical", "node", "tags", "values")])
    var = None
    if ragged and schema.value_kind == A.VAL_VARBYTES:
        # the values cannot take more bytes than the file has
        heap = torch.empty((data.numel() + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        var = A.VarValues(heap.data_ptr(), offsets.data_ptr(), heap.numel())
        c.values = C.addressof(var)
    s, info = schema.with_kind(A.REC_DATED).c(), A.SnapshotInfo()
    stream = torch.cuda.current_stream(dev).cuda_stream
    A.check(A.lib().rh_snapshot_decode_device(C.byref(s), _form(key_form, ragged), data.data_ptr(), data.numel(),
                                              C.byref(c), n, C.byref(info), stream), "rh_snapshot_decode_device")
    if var is not None:
        cols["values"] = (heap[:int(offsets[n])], offsets)
    return cols, SnapshotInfo.from_c(info)


# ---- the host part of the file: members and tombstone acks --------------------------------------
class _Rd:
    def __init__(self, d: bytes, p: int):
        self.d, self.p = d, p

    def take(self, k: int) -> bytes:
        if self.p + k > len(self.d):
            raise A.RsosHipError(A.ERR_DATA, "decode_tail", "io error: unexpected end of file")
        b = self.d[self.p:self.p + k]
        self.p += k
        return b

    def u64(self) -> int:
        return struct.unpack("<Q", self.take(8))[0]

    def ip(self):
        tag = struct.unpack("<I", self.take(4))[0]  # IpAddr: V4 = 0, V6 = 1, then the octets
        if tag > 1:
            raise A.RsosHipError(A.ERR_DATA, "decode_tail",
                                 f"invalid value: integer `{tag}`, expected variant index 0 <= i < 2")
        return ipaddress.ip_address(self.take(4 if tag == 0 else 16))


def decode_tail(data, entries_end: int, schema: RecordSchema, key_form: str = "array", ragged: bool = False
                ) -> Tuple[List, Dict[bytes, Dict[object, int]]]:
    """PersistedState.members (HashSet<IpAddr>) and .tombstone_acks (HashMap<K, HashMap<IpAddr,
    u64>>), bincode fixint, starting at entries_end.  Keys are returned as their column bytes:
    with `ragged` and a string-key schema, an ack key is read as u64 L + L bytes and returned as
    its padded row (strkeys.pack_str_keys); L past the row's width - 1 is ERR_DATA."""
    from .strkeys import pack_str_keys
    r = _Rd(bytes(data), entries_end)
    members = [r.ip() for _ in range(r.u64())]
    acks: Dict[bytes, Dict[object, int]] = {}
    str_keys = ragged and schema.key_kind == A.KEY_STR
    for _ in range(r.u64()):
        if str_keys:
            L = r.u64()
            if L >= schema.key_row:
                raise A.RsosHipError(A.ERR_DATA, "decode_tail",
                                     f"ack key length {L} does not fit a string key row of width {schema.key_row}")
            k = pack_str_keys([r.take(L)], schema.key_row)[0].tobytes()
        else:
            if key_form == "vec" and r.u64() != schema.key_row:
                raise A.RsosHipError(A.ERR_DATA, "decode_tail", "ack key length differs from the schema's")
            k = r.take(schema.key_row)
        peers = {}
        for _ in range(r.u64()):
            ip = r.ip()
            peers[ip] = r.u64()
        acks[k] = peers
    return members, acks


# ---- save: device columns -> the file ------------------------------------------------------------
def _ip_bytes(a) -> bytes:
    a = ipaddress.ip_address(a)
    return struct.pack("<I", 0 if a.version == 4 else 1) + a.packed


def _encode_columns(schema: RecordSchema, cols):
    """(rh_columns, n, heap bytes, what must stay alive) of decode_entries_device's dict."""
    import torch
    n = int(cols["phys"].numel())
    held = []

    def ptr(t, nbytes, name):
        if t is None or nbytes == 0:
            return None
        if not (t.is_cuda and t.is_contiguous()):
            raise ValueError(f"column {name!r} must be a contiguous device tensor")
        if t.numel() * t.element_size() != nbytes:
            raise ValueError(f"column {name!r} has {t.numel() * t.element_size()} bytes, expected {nbytes}")
        held.append(t)
        return t.data_ptr()
    c = A.Columns(ptr(cols.get("keys"), n * schema.key_row, "keys"), ptr(cols["phys"], n * 8, "phys"),
                  ptr(cols["logical"], n * 4, "logical"), ptr(cols["node"], n * 8, "node"),
                  ptr(cols.get("tags"), n, "tags"), None)
    heap_bytes = 0
    if schema.value_kind == A.VAL_VARBYTES:
        heap, offs = cols["values"]
        if not (heap.is_cuda and heap.is_contiguous() and heap.dtype == torch.uint8 and heap.dim() == 1):
            raise ValueError("the value heap must be a contiguous 1-D uint8 device tensor")
        if not (offs.is_cuda and offs.is_contiguous() and offs.element_size() == 8 and offs.numel() == n + 1):
            raise ValueError("the value offsets must be n + 1 contiguous int64 / uint64 device entries")
        heap_bytes = heap.numel()
        if heap.numel() % 4 or heap.data_ptr() % 4:  # the kernels read whole words: pad a copy
            heap = torch.cat([heap, torch.zeros(-heap.numel() % 4, dtype=torch.uint8, device=heap.device)])
        var = A.VarValues(heap.data_ptr() if heap.numel() else None, offs.data_ptr(), heap.numel())
        held += [heap, offs, var]
        c.values = C.addressof(var)
    else:
        c.values = ptr(cols.get("values"), n * schema.value_row, "values")
    return c, n, heap_bytes, held


def encode_entries_device(schema: RecordSchema, cols, key_form: str = "array"):
    """The inverse of decode_entries_device: `cols` (its dict -- keys, phys, logical, node, tags or
    None, values; a VARBYTES schema's values are (heap, offsets)) encoded on the GPU as the file's
    header and entries.  Returns (uint8 device tensor of entries_end bytes, SnapshotInfo); the
    caller appends `encode_tail` at entries_end.  Runs on the tensors' current stream."""
    import torch
    c, n, heap_bytes, held = _encode_columns(schema, cols)
    dev = cols["phys"].device
    kpre = 8 if schema.key_kind == A.KEY_STR or (key_form == "vec" and schema.key_kind == A.KEY_BYTES) else 0
    vpre = 8 if schema.value_kind in (A.VAL_BYTES, A.VAL_VARBYTES) else 0
    bound = 16 + n * (kpre + schema.key_row + 24 + vpre + schema.value_row) + heap_bytes
    out = torch.empty(bound, dtype=torch.uint8, device=dev)
    s, info = schema.with_kind(A.REC_DATED).c(), A.SnapshotInfo()
    stream = torch.cuda.current_stream(dev).cuda_stream
    A.check(A.lib().rh_snapshot_encode_device(C.byref(s), _FORMS[key_form], C.byref(c), n, out.data_ptr(), bound,
                                              C.byref(info), stream), "rh_snapshot_encode_device")
    del held
    return out[:int(info.entries_end)], SnapshotInfo.from_c(info)


def encode_tail(members, acks, schema: RecordSchema, key_form: str = "array", ragged: bool = False) -> bytes:
    """decode_tail's inverse: PersistedState.members and .tombstone_acks as the bytes that follow
    the entries.  Ack keys are column rows (what decode_tail returns); a string-key row is written
    as u64 L and its first L bytes, a byte key under key_form 'vec' as u64 width and the row."""
    if key_form not in _FORMS:
        raise ValueError(f"unknown key_form {key_form!r}")
    out = [struct.pack("<Q", len(members))] + [_ip_bytes(m) for m in members]
    acks = acks or {}
    out.append(struct.pack("<Q", len(acks)))
    W = schema.key_row
    for row, peers in acks.items():
        row = bytes(row)
        if len(row) != W:
            raise ValueError(f"ack key row of {len(row)} bytes, the schema's rows have {W}")
        if schema.key_kind == A.KEY_STR:
            L = row[W - 1]
            if L > W - 1:
                raise ValueError(f"ack key row has length byte {L} (at most {W - 1})")
            out.append(struct.pack("<Q", L) + row[:L])
        else:
            out.append((struct.pack("<Q", W) if key_form == "vec" else b"") + row)
        out.append(struct.pack("<Q", len(peers)))
        out += [_ip_bytes(a) + struct.pack("<Q", int(ver)) for a, ver in peers.items()]
    return b"".join(out)


def write_snapshot_file(path, *parts) -> None:
    """FileSnapshot::save's file sequence (src/snapshot.rs:164-189), host only: the parts written
    to the sibling `path + ".tmp"`, flushed and fsynced, renamed over `path`, and the directory
    fsynced (best effort: some file systems cannot sync a directory)."""
    path = os.fspath(path)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        for p in parts:
            f.write(p)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)
    parent = os.path.dirname(path)
    if parent:
        try:
            fd = os.open(parent, os.O_RDONLY)
        except OSError:
            return
        try:
            os.fsync(fd)
        except OSError:
            pass
        finally:
            os.close(fd)


def save_snapshot(path, schema: RecordSchema, cols, members=(), acks=None, key_form: str = "array") -> SnapshotInfo:
    """FileSnapshot::save for a map whose columns are in HBM: the entries encoded on the device
    (encode_entries_device), copied to the host, the tail appended (encode_tail), the file replaced
    atomically (write_snapshot_file)."""
    head, info = encode_entries_device(schema, cols, key_form)
    write_snapshot_file(path, head.cpu().numpy().tobytes(), encode_tail(list(members), acks, schema, key_form))
    return info
