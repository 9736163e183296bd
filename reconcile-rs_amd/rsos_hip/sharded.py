"""ShardedStore -- one replica's map over several GPUs inside one process (rh_sstore_*).

The benchmark scales with one process per GPU (torch.distributed); a replica is one process
(src/replica.rs:68-74), so inside it the same key-range partitioning is the
library's sharded store: one column store per device, each owning a contiguous key range
[split[s - 1], split[s]), cut at equal counts by a load (before the first load the key space is
cut evenly).  The library answers every question of the Rsos<K> surface (rsos/src/rsos_trait.rs:39-90)
and whole protocol rounds (rbsr/src/protocol.rs:212-317) by decomposing them over the shards, with
no device-to-device traffic and one host thread per shard (include/rsos_hip.h, csrc/sharded_store.hip):

  size / rank(z)        sums over shards: rank(z) = rows of the shards below z's + rank in z's shard
  aggregate(range)      the shards inside the range give their roots, <= 2 boundary shards are asked
                        (Aggregate's Add, rsos/src/aggregate.rs:79-89)
  select(r)             the shard whose rank interval holds r
  apply / stage         rows routed to their key's shard by the splitters
  load_bulk_device /    records already in HBM: a load cut at multiples of 16 rows and read in place,
  apply_device          a batch partitioned by the splitters on the GPU (csrc/shard_route.hip)
  protocol round        a run of segments inside one shard is that shard's own round; a segment
                        straddling a boundary is resolved from its two boundary shards, decided on
                        the host and cut by routed selects and rank-range aggregates
  enumerate_segments    a range inside one shard is that shard's; one that straddles splitters is its
                        pieces in shard order, first ranks made global (rh_sstore_enumerate_segments)

ShardedStore has GpuFingerprintStore's interface (the same methods, on rh_sstore_* entry points), so
rsos_hip.rbsr's native and two-call round paths run on it unchanged.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _abi as A
from .schema import RecordSchema
from .store import GpuFingerprintStore, Key, _np_ptr, DEFAULT_HOST_TIER


class _Shard(GpuFingerprintStore):
    """One shard's store, borrowed from the sharded store (destroyed with it)."""

    def __init__(self, schema: RecordSchema, handle: C.c_void_p):
        self.schema = schema
        self._s = schema.c()
        self._h = handle

    def close(self) -> None:
        self._h = None  # borrowed: the sharded store destroys it

    def _f(self, name):
        if self._h is None:
            raise ValueError("shard of a closed ShardedStore")
        return GpuFingerprintStore._f(self, name)


class ShardedStore(GpuFingerprintStore):
    _P = "rh_sstore_"

    def __init__(self, schema: RecordSchema, devices: Sequence[int], host_tier: Optional[bool] = None,
                 var_values: bool = False):
        """var_values=True opts in to a 'var' schema (String / Vec<u8> values: rh_sstore_create_flags with
        RH_SSTORE_VARBYTES); without it such a schema is refused, as ever."""
        if not devices:
            raise ValueError("at least one device")
        self.schema = schema
        self._s = schema.c()
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        if var_values:
            A.check(A.lib().rh_sstore_create_flags(devs, len(devices), C.byref(self._s), A.SSTORE_VARBYTES, C.byref(h)),
                    "rh_sstore_create_flags")
        else:
            A.check(A.lib().rh_sstore_create(devs, len(devices), C.byref(self._s), C.byref(h)), "rh_sstore_create")
        self._h = h
        self.shards = []
        for i in range(len(devices)):
            sh = C.c_void_p()
            A.check(A.lib().rh_sstore_shard(self._h, i, C.byref(sh)), "rh_sstore_shard")
            self.shards.append(_Shard(schema, sh))
        if DEFAULT_HOST_TIER if host_tier is None else host_tier:
            self.set_host_tier(True)

    def close(self) -> None:
        """Destroy the sharded store and every shard's store: the _Shard views (and any the caller
        kept) are detached first, so a later call on one raises instead of reaching freed memory."""
        for sh in getattr(self, "shards", []):
            sh.close()
        GpuFingerprintStore.close(self)

    # ---- the partition -------------------------------------------------------------------
    @property
    def splitters(self) -> List[Key]:
        kl = self.schema.key_row
        g = len(self.shards)
        buf = np.zeros(max((g - 1) * kl, 1), np.uint8)
        A.check(A.lib().rh_sstore_splitters(self._h, _np_ptr(buf)), "rh_sstore_splitters")
        return [self._key_out(buf[j * kl:(j + 1) * kl].tobytes()) for j in range(g - 1)]

    def set_splitters(self, keys: Sequence[Key]) -> None:
        """Cut an empty map's key space at `keys` (len(shards) - 1 of them, non-decreasing)."""
        if len(keys) != len(self.shards) - 1:
            raise ValueError("one splitter per shard boundary")
        buf = np.frombuffer(b"".join(self._key_bytes(k) for k in keys) or b"\0", np.uint8).copy()
        A.check(A.lib().rh_sstore_set_splitters(self._h, _np_ptr(buf)), "rh_sstore_set_splitters")

    def sizes(self) -> List[int]:
        return [s.size() for s in self.shards]

    # ---- per-shard bookkeeping (the shards' own counters) --------------------------------
    def stats(self) -> Dict[str, int]:
        out = {"base_rows": 0, "delta_rows": 0, "compactions": 0}
        for s in self.shards:
            for k, v in s.stats().items():
                out[k] += v
        return out

    def tier_stats(self) -> Dict[str, int]:
        out = {"base_rows": 0, "delta_entries": 0, "refreshes": 0, "folds": 0}
        for s in self.shards:
            for k, v in s.tier_stats().items():
                out[k] += v
        return out

    def batch_stats(self) -> Dict[str, int]:
        out = {"small": 0, "large": 0}
        for s in self.shards:
            for k, v in s.batch_stats().items():
                out[k] += v
        return out

    def enumerate_stats(self) -> Dict[str, int]:
        """The shards' device enumerate calls, summed (rh_store_enumerate_stats of each shard)."""
        out = {"one_launch": 0, "general": 0}
        for s in self.shards:
            for k, v in s.enumerate_stats().items():
                out[k] += v
        return out

    def tier_sync(self) -> None:
        for s in self.shards:
            s.tier_sync()

    def set_compaction(self, divisor: int, min_rows: int) -> None:
        for s in self.shards:
            s.set_compaction(divisor, min_rows)

    # ---- device columns (rh_sstore_load_device / rh_sstore_apply_device) ------------------
    @staticmethod
    def _device_of(cols) -> int:
        """The device the (torch) columns live on: all of them on one."""
        devs = {t.device for t in cols.values() if t is not None}
        if len(devs) != 1 or next(iter(devs)).type != "cuda":
            raise ValueError("device columns must live on one GPU")
        d = next(iter(devs))
        import torch
        return torch.cuda.current_device() if d.index is None else d.index

    @staticmethod
    def _stream_on(device: int) -> int:
        import torch
        return torch.cuda.current_stream(device).cuda_stream

    def load_bulk_device(self, cols) -> None:
        """load_bulk from device (torch) columns: keys sorted and strictly increasing.  The rows are
        cut at equal counts rounded down to multiples of 16; shards on the columns' device read them
        in place, shards elsewhere get a device-to-device copy."""
        from .device import _check_cols, _columns
        n = _check_cols(self.schema, cols)
        dev = self._device_of(cols)
        c = _columns(cols)
        A.check(A.lib().rh_sstore_load_device(self._h, dev, C.byref(c), n, self._stream_on(dev)),
                "rh_sstore_load_device")

    def apply_device(self, cols, ops=None):
        """apply() with device (torch) columns / ops: the rows are routed to their shards on the GPU
        (rsos_hip.device.route_columns' kernel), then each shard applies its segment.  Returns (new,
        overwritten, deleted).  A repeated key is refused by its shard after others may have
        committed: the map then refuses every call until a load."""
        from .device import _check_cols, _columns
        m = _check_cols(self.schema, cols)
        if ops is not None and (ops.numel() != m or not ops.is_cuda):
            raise ValueError("ops must be m device bytes")
        dev = self._device_of(cols)
        c = _columns(cols)
        a, b, d = C.c_uint64(), C.c_uint64(), C.c_uint64()
        A.check(A.lib().rh_sstore_apply_device(self._h, dev, C.byref(c), None if ops is None else ops.data_ptr(), m,
                                               C.byref(a), C.byref(b), C.byref(d), self._stream_on(dev)),
                "rh_sstore_apply_device")
        return int(a.value), int(b.value), int(d.value)

    def apply_device_many(self, batches, ops=None):
        """apply_device over several device batches in order; (new, overwritten, deleted) per batch."""
        if ops is not None and len(ops) != len(batches):
            raise ValueError("ops must have one entry per batch")
        return [self.apply_device(b, None if ops is None else ops[i]) for i, b in enumerate(batches)]

    @staticmethod
    def load_snapshot(data, dated: Optional["ShardedStore"], projection: Optional["ShardedStore"], key_form: str = "array",
                      ragged: bool = False, device: int = 0):
        """Reload a sharded replica's dated map and / or projection from an RCNL v1 snapshot
        (rh_sstore_load_snapshot): `data` is host bytes, or a uint8 tensor on `device`.  The entries
        must be in strictly increasing key order (what FileSnapshot::save writes).  Returns
        rsos_hip.snapshot.SnapshotInfo."""
        from .snapshot import SnapshotInfo
        form = {"array": A.FORM_ARRAY, "vec": A.FORM_VEC}[key_form] | (A.FORM_RAGGED if ragged else 0)
        info = A.SnapshotInfo()
        hd = None if dated is None else dated._h
        hp = None if projection is None else projection._h
        if isinstance(data, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(bytes(data), np.uint8)
            rc = A.lib().rh_sstore_load_snapshot(hd, hp, form, _np_ptr(buf), buf.size, 0, device, C.byref(info))
        else:
            import torch
            if not (data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()):
                raise ValueError("device snapshot bytes must be a contiguous uint8 device tensor")
            device = torch.cuda.current_device() if data.device.index is None else data.device.index
            torch.cuda.current_stream(device).synchronize()  # the call takes complete bytes
            rc = A.lib().rh_sstore_load_snapshot(hd, hp, form, data.data_ptr(), data.numel(), 1, device, C.byref(info))
        A.check(rc, "rh_sstore_load_snapshot")
        return SnapshotInfo(int(info.entries), int(info.tombstones), int(info.entries_end), int(info.keys))

    def _key_bytes(self, k: Key) -> bytes:
        return GpuFingerprintStore._key_bytes(self, k)
