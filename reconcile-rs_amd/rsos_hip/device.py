"""Device-resident batch API: torch CUDA(HIP) tensors in, kernels enqueued on torch's
current stream (no synchronisation, no host copies).

Every shape is checked on the host before a launch: the kernels index rows by `n`, so a
column shorter than n rows would read out of bounds.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import _abi as A
from .schema import RecordSchema

COLS = ("keys", "phys", "logical", "node", "tags", "values")
# a 'var' schema's values: `values` is the uint8 heap, `value_offsets` n + 1 int64 / uint64 offsets
VAR_OFFSETS = "value_offsets"


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def block_sums_for(n: int) -> int:
    return (n + A.BLOCK - 1) // A.BLOCK


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


_NEED: Dict[tuple, tuple] = {}  # per schema: (column, row width) of every required column


def _need(schema: RecordSchema) -> tuple:
    key = (schema.key_row, schema.value_row, bool(schema.dated_kind), schema.is_var)
    got = _NEED.get(key)
    if got is None:
        need = [("keys", schema.key_row), ("values", schema.value_row)]
        if schema.dated_kind:
            need += [("phys", 8), ("logical", 4), ("node", 8)]
        got = _NEED[key] = tuple((c, w) for c, w in need if w)
    return got


def _check_cols(schema: RecordSchema, cols: Dict[str, torch.Tensor]) -> int:
    """The row count, after checking every column the schema needs: present, a contiguous device
    tensor, and exactly n rows of its width (the kernels index rows by n)."""
    for k in cols:
        if k not in COLS and not (k == VAR_OFFSETS and schema.is_var):
            raise ValueError(f"unknown column {k!r}")
    if schema.is_var:
        heap, offs = cols.get("values"), cols.get(VAR_OFFSETS)
        if heap is None or offs is None:
            raise ValueError(f"columns 'values' (the heap) and {VAR_OFFSETS!r} are required by {schema}")
        if not (heap.is_cuda and heap.is_contiguous() and heap.dtype == torch.uint8 and heap.dim() == 1):
            raise ValueError("the value heap must be a contiguous 1-D uint8 device tensor")
        if not (offs.is_cuda and offs.is_contiguous() and offs.element_size() == 8 and offs.dim() == 1
                and offs.numel() >= 1):
            raise ValueError(f"{VAR_OFFSETS!r} must be a contiguous 1-D int64 / uint64 device tensor of n + 1 entries")
        n = offs.numel() - 1
        if schema.key_row and cols.get("keys") is not None and cols["keys"].nbytes != n * schema.key_row:
            raise ValueError(f"column 'keys' has {cols['keys'].nbytes} bytes, expected {n} x {schema.key_row}")
    elif schema.key_row:
        n = cols["keys"].nbytes // schema.key_row
    else:
        n = cols["values"].nbytes // max(schema.value_row, 1)
    for name, width in _need(schema):
        t = cols.get(name)
        if t is None:
            raise ValueError(f"column {name!r} is required by {schema}")
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"column {name!r} must be a contiguous device tensor")
        if t.nbytes != n * width:
            raise ValueError(f"column {name!r} has {t.nbytes} bytes, expected {n} x {width}")
    t = cols.get("tags")
    if t is not None and (t.nbytes != n or not t.is_cuda):
        raise ValueError("tags must be n device bytes")
    return n


def _columns(cols: Dict[str, torch.Tensor]) -> A.Columns:
    """rh_columns of device tensors.  For a 'var' schema the returned object owns what its `values`
    points to (the host descriptor and a padded heap copy): keep THIS object alive for the call --
    a copy of the struct (an assignment into a ctypes array) does not."""
    c = A.Columns(*[_ptr(cols.get(k)) for k in COLS])
    offs = cols.get(VAR_OFFSETS)
    if offs is not None:  # a 'var' schema: values -> the descriptor of heap + offsets (rh_var_values)
        heap = cols["values"]
        if heap.numel() % 4:  # the kernels read whole dwords: pad the heap, as lift_encoded does
            heap = torch.cat([heap, torch.zeros(4 - heap.numel() % 4, dtype=torch.uint8, device=heap.device)])
        var = A.VarValues(_ptr(heap), _ptr(offs), heap.numel())
        c.values = C.addressof(var)
        c._held = (var, heap)  # alive as long as the Columns
    return c


def route_columns(schema: RecordSchema, splitters, shards: int, cols: Dict[str, torch.Tensor],
                  ops: Optional[torch.Tensor] = None, out: Optional[Dict[str, torch.Tensor]] = None,
                  ops_out: Optional[torch.Tensor] = None, cap_rows: Optional[int] = None):
    """The sharded store's partition of a device batch, on its own (rh_route_columns_device): record
    i goes to shard s = the number of `splitters` (shards - 1 key rows, uint8, non-decreasing) <= its
    key; each shard's rows form one segment of the output columns, in input order, starting at a
    multiple of 16 rows.  Returns (out columns, out ops, counts, starts): shard s's rows are
    out[c][starts[s] : starts[s] + counts[s]].  `out` / `ops_out`: preallocated columns with room for
    `cap_rows` rows (default: new ones of n + 16 * shards rows).  Synchronous on the current stream."""
    import numpy as np
    n = _check_cols(schema, cols)
    if ops is not None and (ops.numel() != n or not ops.is_cuda):
        raise ValueError("ops must be n device bytes")
    dev = next(iter(cols.values())).device
    if cap_rows is None:
        cap_rows = n + 16 * max(shards, 0)
    if out is None:
        out = {k: torch.empty((cap_rows,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev)
               for k, v in cols.items() if v is not None}
    if ops is not None and ops_out is None:
        ops_out = torch.empty(cap_rows, dtype=torch.uint8, device=dev)
    sp = np.ascontiguousarray(splitters, dtype=np.uint8).reshape(-1)
    counts, starts = np.zeros(max(shards, 1), np.uint64), np.zeros(max(shards, 1), np.uint64)
    s, cin, cout = schema.c(), _columns(cols), _columns(out)
    A.check(A.lib().rh_route_columns_device(C.byref(s), sp.ctypes.data if sp.size else None, shards, C.byref(cin),
                                            _ptr(ops), n, C.byref(cout), _ptr(ops_out), cap_rows,
                                            counts.ctypes.data, starts.ctypes.data, _stream()),
            "rh_route_columns_device")
    return out, ops_out, counts[:shards], starts[:shards]


def route_columns_var(schema: RecordSchema, splitters, shards: int, cols: Dict[str, torch.Tensor],
                      ops: Optional[torch.Tensor] = None, out: Optional[Dict[str, torch.Tensor]] = None,
                      ops_out: Optional[torch.Tensor] = None, cap_rows: Optional[int] = None,
                      heap_cap: Optional[int] = None):
    """route_columns for a 'var' schema (rh_route_columns_var_device): the same row partition, and the
    values -- `values` the uint8 heap, `value_offsets` n + 1 offsets -- packed in output-row order into
    out['values'] (a heap of `heap_cap` bytes, a multiple of 4; default: the input heap's size rounded
    up to 4, which always suffices for well-formed offsets) with out['value_offsets'][0 .. R] written,
    R = starts[-1] + roundup16(counts[-1]).  Shard s's values are the heap with the offsets from
    starts[s] on.  Returns (out columns, out ops, counts, starts, heap_bytes).  A fixed-width schema
    goes to route_columns' entry point unchanged (heap_bytes = 0)."""
    import numpy as np
    n = _check_cols(schema, cols)
    if ops is not None and (ops.numel() != n or not ops.is_cuda):
        raise ValueError("ops must be n device bytes")
    dev = next(iter(cols.values())).device
    if cap_rows is None:
        cap_rows = n + 16 * max(shards, 0)
    if out is None:
        out = {k: torch.empty((cap_rows,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev)
               for k, v in cols.items() if v is not None and not (schema.is_var and k in ("values", VAR_OFFSETS))}
        if schema.is_var:
            if heap_cap is None:
                heap_cap = (cols["values"].numel() + 3) // 4 * 4
            out["values"] = torch.empty(max(heap_cap, 4), dtype=torch.uint8, device=dev)
            out[VAR_OFFSETS] = torch.empty(cap_rows + 1, dtype=cols[VAR_OFFSETS].dtype, device=dev)
    if ops is not None and ops_out is None:
        ops_out = torch.empty(cap_rows, dtype=torch.uint8, device=dev)
    sp = np.ascontiguousarray(splitters, dtype=np.uint8).reshape(-1)
    counts, starts = np.zeros(max(shards, 1), np.uint64), np.zeros(max(shards, 1), np.uint64)
    heap_bytes = C.c_uint64(0)
    s, cin = schema.c(), _columns(cols)
    if schema.is_var:  # the output heap is handed over as it is: its capacity, never a padded copy
        if heap_cap is None:
            heap_cap = out["values"].numel() // 4 * 4
        if out["values"].numel() < heap_cap or out[VAR_OFFSETS].numel() < cap_rows + 1:
            raise ValueError("out['values'] / out['value_offsets'] are smaller than heap_cap / cap_rows + 1")
        cout = A.Columns(*[_ptr(out.get(k)) for k in COLS])
        var = A.VarValues(_ptr(out["values"]), _ptr(out[VAR_OFFSETS]), heap_cap)
        cout.values = C.addressof(var)
    else:
        cout = _columns(out)
    A.check(A.lib().rh_route_columns_var_device(C.byref(s), sp.ctypes.data if sp.size else None, shards, C.byref(cin),
                                                _ptr(ops), n, C.byref(cout), _ptr(ops_out), cap_rows,
                                                counts.ctypes.data, starts.ctypes.data, C.byref(heap_bytes), _stream()),
            "rh_route_columns_var_device")
    return out, ops_out, counts[:shards], starts[:shards], int(heap_bytes.value)


def lift_records(schema: RecordSchema, cols: Dict[str, torch.Tensor], block_sums: bool = True,
                 fps: Optional[torch.Tensor] = None, bsums: Optional[torch.Tensor] = None
                 ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """fps[i] = lift(key_i, record_i) as 32 LE bytes; bsums[g] = Σ fps over rows 256g..256g+255."""
    n = _check_cols(schema, cols)
    dev = next(iter(cols.values())).device
    if fps is None:
        fps = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    if block_sums and bsums is None:
        bsums = torch.empty((block_sums_for(n), 32), dtype=torch.uint8, device=dev)
    if fps.shape != (n, 32) or (bsums is not None and bsums.shape != (block_sums_for(n), 32)):
        raise ValueError("output shape mismatch")
    s, c = schema.c(), _columns(cols)
    A.check(A.lib().rh_lift_records_async(C.byref(s), C.byref(c), n, _ptr(fps),
                                          _ptr(bsums) if block_sums else None, _stream()),
            "rh_lift_records_async")
    return fps, (bsums if block_sums else None)


def lift_dual(schema: RecordSchema, cols: Dict[str, torch.Tensor], out=None):
    """Both lifts of Replica::map_insert (src/replica/write.rs:44-45) from one read of the
    records: (dated fps, dated block sums, projection fps, projection block sums).  `out`: the
    same four tensors, preallocated (reused across calls)."""
    if schema.record_kind != A.REC_DATED:
        raise ValueError("dual lift needs a DATED schema")
    n = _check_cols(schema, cols)
    dev = next(iter(cols.values())).device
    if out is not None:
        fd, bd, fp, bp = out
        if fd.shape != (n, 32) or fp.shape != (n, 32) or bd.shape[0] < block_sums_for(n) or \
                bp.shape[0] < block_sums_for(n):
            raise ValueError("out tensors have the wrong shape")
    else:
        fd = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        fp = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        bd = torch.empty((block_sums_for(n), 32), dtype=torch.uint8, device=dev)
        bp = torch.empty((block_sums_for(n), 32), dtype=torch.uint8, device=dev)
    s, c = schema.c(), _columns(cols)
    A.check(A.lib().rh_lift_dual_async(C.byref(s), C.byref(c), n, _ptr(fd), _ptr(bd), _ptr(fp), _ptr(bp),
                                       _stream()), "rh_lift_dual_async")
    return fd, bd, fp, bp


def lift_encoded(data: torch.Tensor, offsets: torch.Tensor, block_sums: bool = True):
    """BLAKE3 of pre-encoded canonical records: record i = data[offsets[i]:offsets[i+1]]."""
    if offsets.dtype != torch.int64 or not offsets.is_cuda or offsets.dim() != 1:
        raise ValueError("offsets must be a 1-D int64 device tensor of n+1 entries")
    n = offsets.numel() - 1
    dev = offsets.device
    fps = torch.empty((max(n, 0), 32), dtype=torch.uint8, device=dev)
    bs = torch.empty((block_sums_for(n), 32), dtype=torch.uint8, device=dev) if block_sums else None
    # the kernel may read the last dword containing data[offsets[n]-1]: pad to 4
    if data.numel() % 4:
        data = torch.cat([data, torch.zeros(4 - data.numel() % 4, dtype=torch.uint8, device=dev)])
    A.check(A.lib().rh_lift_encoded_async(_ptr(data), data.numel(), _ptr(offsets), n, _ptr(fps), _ptr(bs),
                                          _stream()),
            "rh_lift_encoded_async")
    return fps, bs


def lift_fixed(data: torch.Tensor, record_len: int, n: Optional[int] = None, block_sums: bool = True):
    """BLAKE3 of fixed-length canonical records: record i = data[i*record_len:(i+1)*record_len]
    (n defaults to data.numel() // record_len; trailing bytes are padding)."""
    if data.dtype != torch.uint8 or not data.is_cuda or data.dim() != 1:
        raise ValueError("data must be a 1-D uint8 device tensor")
    if record_len < 0:
        raise ValueError("record_len must be >= 0")
    if n is None:
        if record_len == 0:
            raise ValueError("n is required when record_len is 0")
        n = data.numel() // record_len
    dev = data.device
    fps = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    bs = torch.empty((block_sums_for(n), 32), dtype=torch.uint8, device=dev) if block_sums else None
    if data.numel() % 4:
        data = torch.cat([data, torch.zeros(4 - data.numel() % 4, dtype=torch.uint8, device=dev)])
    A.check(A.lib().rh_lift_fixed_async(_ptr(data), data.numel(), record_len, n, _ptr(fps), _ptr(bs), _stream()),
            "rh_lift_fixed_async")
    return fps, bs


def reduce_blocks(x: torch.Tensor) -> torch.Tensor:
    """out[g] = Σ x[256g .. 256g+255] (mod 2^256)."""
    n = x.shape[0]
    out = torch.empty((block_sums_for(n), 32), dtype=torch.uint8, device=x.device)
    A.check(A.lib().rh_reduce_blocks_async(_ptr(x), n, _ptr(out), _stream()), "rh_reduce_blocks_async")
    return out


def range_aggregates(fps: torch.Tensor, bsums: Optional[torch.Tensor], ssums: Optional[torch.Tensor],
                     lo: torch.Tensor, hi: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(r, 5) int64 device tensor: per rank range [lo, hi), fingerprint limbs 0..3 then size."""
    n = fps.shape[0]
    r = lo.numel()
    if hi.numel() != r or lo.dtype != torch.int64 or hi.dtype != torch.int64:
        raise ValueError("lo / hi must be int64 of equal length")
    if bsums is not None and bsums.shape[0] != block_sums_for(n):
        raise ValueError("block sums do not match fps")
    if ssums is not None and (bsums is None or ssums.shape[0] != block_sums_for(bsums.shape[0])):
        raise ValueError("super-block sums do not match block sums")
    if out is None:
        out = torch.empty((r, 5), dtype=torch.int64, device=fps.device)
    A.check(A.lib().rh_range_aggregates_async(_ptr(fps), _ptr(bsums), _ptr(ssums), n, _ptr(lo), _ptr(hi), r,
                                              _ptr(out), _stream()), "rh_range_aggregates_async")
    return out


def combine_aggregates(parts: torch.Tensor) -> torch.Tensor:
    """parts: (P, r, 5) int64 gathered aggregates -> (r, 5) Σ over P (Aggregate's Add)."""
    p, r, five = parts.shape
    assert five == 5
    out = torch.empty((r, 5), dtype=torch.int64, device=parts.device)
    A.check(A.lib().rh_combine_aggregates_async(_ptr(parts.contiguous()), p, r, _ptr(out), _stream()),
            "rh_combine_aggregates_async")
    return out
