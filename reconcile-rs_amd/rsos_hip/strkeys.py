"""Short string keys in fixed-width rows (RH_KEY_STR, include/rsos_hip.h).

A row of width W holds the string's L <= W - 1 bytes, zero bytes up to offset W - 2, and L in its
last byte.  Sorting the rows by their raw bytes sorts the strings as Rust's Ord of String /
Vec<u8> does (bytes first, a proper prefix before its extensions), so every store operation
treats them as byte keys of width W; only the lift hashes the string and not the row.
"""
from __future__ import annotations

from typing import Iterable, List, Union

import numpy as np

StrKey = Union[str, bytes, bytearray, memoryview]


def _raw(k: StrKey) -> bytes:
    return k.encode() if isinstance(k, str) else bytes(k)


def pack_str_keys(keys: Iterable[StrKey], width: int) -> np.ndarray:
    """The (n, width) uint8 rows of `keys` (str: its UTF-8).  ValueError past width - 1 bytes."""
    if width not in (16, 32, 64):
        raise ValueError("a string key row is 16, 32 or 64 bytes wide")
    raws = [_raw(k) for k in keys]
    rows = np.zeros((len(raws), width), np.uint8)
    for i, b in enumerate(raws):
        if len(b) > width - 1:
            raise ValueError(f"string key of {len(b)} bytes: a {width}-byte row holds at most {width - 1}")
        rows[i, :len(b)] = np.frombuffer(b, np.uint8)
        rows[i, width - 1] = len(b)
    return rows


def unpack_str_keys(rows) -> List[bytes]:
    """pack_str_keys' inverse: the strings' bytes.  ValueError for a length byte past width - 1."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if rows.ndim != 2:
        raise ValueError("rows must be (n, width)")
    w = rows.shape[1]
    out = []
    for r in rows:
        n = int(r[w - 1])
        if n > w - 1:
            raise ValueError(f"length byte {n} in a {w}-byte row")
        out.append(r[:n].tobytes())
    return out
