"""What the batched-Enumerate tests share (test_enumerate_segments.py, test_enumerate_sharded.py,
test_enumerate_drive.py): a host model of a store's live key set, and the expected answer of
rh_store_enumerate_segments computed from it with no product code.

A key is a token: the integer for u32 / u64 keys, the row's bytes for byte keys, the string's bytes for
RH_KEY_STR keys -- Python's order of tokens is the key type's Ord (integers numerically, bytes and
strings bytewise with a proper prefix first), and a token is what the Python bindings take as a key.
Expected: first_rank = the lower bound of the start key in the sorted live keys (Unbounded: 0), the
rows = sorted[lo:hi] with hi the lower bound of the end key (Unbounded: the size)."""
import bisect

import numpy as np

SCHEMAS = {  # name -> (key, value): the column store's u32 / u64 / byte-array / 64-byte string rows
    "u32_u32": ("u32", "u32"),
    "u64_u64": ("u64", "u64"),
    "b16_u64": ("bytes16", "u64"),
    "b32_b64": ("bytes32", "bytes64"),
    "str63_u64": ("str63", "u64"),  # 64-byte rows: the general device path (no one-launch kernels)
}


def schema(name):
    from rsos_hip import RecordSchema
    return RecordSchema.plain(*SCHEMAS[name])


class Keys:
    """The live key set of a store, replayed on the host."""

    def __init__(self, sch):
        self.sch, self.kl = sch, sch.key_row
        self.ints = sch.key_kind in (1, 2)
        self.live = set()
        self._sorted = None

    # ---- tokens and rows ------------------------------------------------------------------------
    def row(self, tok) -> bytes:
        if self.ints:
            return int(tok).to_bytes(self.kl, "little")
        if self.sch.is_str:  # the string, zeros, its length in the last byte
            return tok + bytes(self.kl - 1 - len(tok)) + bytes([len(tok)])
        return tok

    def rows(self, toks) -> np.ndarray:
        return np.frombuffer(b"".join(self.row(t) for t in toks), np.uint8).reshape(len(toks), self.kl).copy()

    def fresh(self, rng, n, taken=()):
        """n distinct random tokens outside self.live and `taken`, all below self.above()"""
        out, seen = [], set(taken)
        while len(out) < n:
            if self.ints:
                t = int(rng.integers(0, (1 << (8 * self.kl - 1)) - 1, dtype=np.uint64))
            elif self.sch.is_str:
                t = bytes(rng.integers(97, 123, int(rng.integers(1, min(41, self.kl))), dtype=np.uint8))
            else:
                t = bytes(rng.integers(0, 0xF0, 1, dtype=np.uint8)) + rng.bytes(self.kl - 1)
            if t not in self.live and t not in seen:
                seen.add(t)
                out.append(t)
        return out

    def above(self, k=0):
        """a token above every key fresh() makes (k: a few distinct ones, increasing)"""
        if self.ints:
            return (1 << (8 * self.kl)) - 9 + k
        if self.sch.is_str:
            return b"~" * (3 + k)
        return b"\xff" * (self.kl - 1) + bytes([0xF0 + k])

    # ---- contents ----------------------------------------------------------------------------
    def apply(self, toks, ops):
        for t, op in zip(toks, ops):
            (self.live.discard if op else self.live.add)(t)
        self._sorted = None

    def sorted(self):
        if self._sorted is None:
            self._sorted = sorted(self.live)
        return self._sorted

    def columns(self, rng, toks):
        """host columns (plain record kind) for rows with these keys, random values"""
        return {"keys": self.rows(toks),
                "values": rng.integers(0, 256, size=(len(toks), self.sch.value_row), dtype=np.uint8)}

    # ---- the expected answer -------------------------------------------------------------------
    def expect(self, ranges):
        """(first_ranks, offsets, key rows) for (start, end) token pairs (None = Unbounded)"""
        s = self.sorted()
        first, offs, parts = np.zeros(len(ranges), np.uint64), np.zeros(len(ranges) + 1, np.uint64), []
        for j, (a, b) in enumerate(ranges):
            lo = 0 if a is None else bisect.bisect_left(s, a)
            hi = len(s) if b is None else bisect.bisect_left(s, b)
            first[j] = lo
            offs[j + 1] = offs[j] + max(hi - lo, 0)
            parts.extend(s[lo:hi])
        return first, offs, self.rows(parts) if parts else np.zeros((0, self.kl), np.uint8)


def special_ranges(rng, keys: Keys, base=None, touched=()):
    """The ranges every state is asked: both sides unbounded; bounds that are present keys; bounds that
    are absent keys; an empty range between two non-empty ones; an inverted range; two identical
    ranges; overlapping ranges; ranges whose rows straddle base rows 256 k and 65,536 (`base`: the
    base run's sorted tokens); ranges around `touched` keys (deleted base rows, run-only inserts,
    overwrites); starts above the last key; one side unbounded."""
    s = keys.sorted()
    n = len(s)
    out = [(None, None)]
    absent = sorted(keys.fresh(rng, 8))
    out += [(absent[0], absent[1]), (absent[5], absent[2])]  # absent bounds; inverted absent bounds
    out += [(keys.above(0), None), (keys.above(0), keys.above(1)), (None, keys.above(2))]
    if n >= 64:
        p = sorted(int(x) for x in rng.integers(0, n - 50, 6))
        out += [(s[p[0]], s[p[0] + 7]),                      # present bounds
                (s[p[1]], s[p[1]]),                          # empty, between two non-empty ones
                (s[p[2]], s[p[2] + 19]),
                (s[p[3] + 9], s[p[3]]),                      # inverted
                (s[p[4]], s[p[4] + 11]), (s[p[4]], s[p[4] + 11]),       # identical
                (s[p[5]], s[p[5] + 30]), (s[p[5] + 12], s[p[5] + 45]),  # overlapping
                (absent[3], s[p[2] + 3]), (s[p[1] + 2], absent[6]),     # one absent bound (maybe inverted)
                (None, s[5]), (s[n - 4], None)]
    if base is not None:
        for edge in (256, 1024, 65536):
            if edge + 9 < len(base):
                out.append((base[edge - 6], base[edge + 9]))
    for t in touched:
        i = bisect.bisect_left(s, t)
        out.append((s[max(i - 3, 0)], s[min(i + 3, n - 1)] if n else None))
    return out


def many_ranges(rng, keys: Keys, r, specials):
    """r ranges: the specials at random places among short random ranges (0 to 40 rows each, so that
    3,000 of them stay far below the 2^22-row cap)"""
    s = keys.sorted()
    n = len(s)
    out = []
    absent = keys.fresh(rng, max(r // 4, 4))
    for i in range(max(r - len(specials), 0)):
        a = absent[int(rng.integers(len(absent)))]
        if n < 64:  # (a small store: any two absent bounds)
            b = absent[int(rng.integers(len(absent)))]
        elif i % 4 == 3:  # an absent start, a present end a few rows on
            b = s[min(bisect.bisect_left(s, a) + int(rng.integers(0, 30)), n - 1)]
        else:
            p = int(rng.integers(0, n - 41))
            a, b = s[p], s[p + int(rng.integers(0, 41))]
        out.append((a, b))
    for sp in specials:
        out.insert(int(rng.integers(0, len(out) + 1)), sp)
    return out[:r] if len(out) > r else out


def check(store, keys: Keys, ranges, **kw):
    """enumerate_segments(ranges) equals the host's answer, array by array"""
    first, offs, rows = store.enumerate_segments(ranges, **kw)
    wf, wo, wr = keys.expect(ranges)
    assert first.dtype == np.uint64 and offs.dtype == np.uint64 and rows.dtype == np.uint8
    assert np.array_equal(offs, wo), "offsets"
    assert np.array_equal(first, wf), "first ranks"
    assert rows.shape == wr.shape and np.array_equal(rows, wr), "keys"
    return first, offs, rows
