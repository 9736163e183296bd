"""The record model shared by the lift, store, sharded and route tests.

One statement of each thing those tests used to carry a copy of: the 256-bit helpers, the shape
vocabulary (key / value row widths and oracle/pyref.py's typed model of a key and a value), the
reference's canonical encoding of a record (`canonical`, anchored to tests/golden/vectors.json by
tests/test_records_common.py), the lift-case builder with its device upload and check, the dict
model of a store over record tuples, and the column-style model of tests/test_small_batch.py.

Expected fingerprints come from the oracle alone: canonical bytes are built here with pyref's
typed model and hashed by the C oracle (oracle.lift_encoded, oracle.Records.lift) -- never by
the product's encoder or a second GPU kernel.

Keys are "unit" | "u32" | "u64" | "bytesN" | "strN"; values "unit" | "u32" | "u64" | "bytesN" |
"var"; record kinds "plain" | "dated" | "projection".  A record tuple is (key bytes, (phys,
logical, node), tomb, value) with the value as bytes, or as an int for u32 / u64.
"""
import bisect

import numpy as np

import pyref as P  # oracle/pyref.py

M256 = 1 << 256
U64_MAX = (1 << 64) - 1
KINDS = ("plain", "dated", "projection")
# message lengths (prefix + value) among the present rows of the string-key var lift cases: block
# edges, the chunk edge, and the multi-chunk kernel with parent nodes (two, three and five chunks)
STR_TOTALS = (63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1500, 3000, 5000)


# ---- 256-bit values --------------------------------------------------------------------------------

def fp_int(b) -> int:
    """32 little-endian bytes (a fingerprint row) -> int."""
    return int.from_bytes(bytes(b), "little")


def limbs_int(l) -> int:
    """Four 64-bit limbs, least significant first (signed int64 limbs taken as their bits) -> int."""
    return sum((int(x) & U64_MAX) << (64 * i) for i, x in enumerate(l))


def row_int(row) -> int:
    """Row of an (r, 5) aggregate array {fp[4]; size} -> the fingerprint as int."""
    return limbs_int(row[:4])


def agg_int(a) -> int:
    """rsos_hip Aggregate -> the fingerprint as int."""
    return a.fingerprint.to_int()


def fold(fps) -> int:
    """The sum of fingerprint rows mod 2^256."""
    return sum(fp_int(f) for f in fps) % M256


# ---- the shape vocabulary ---------------------------------------------------------------------------

def key_width(key) -> int:
    """Bytes of a key column row (a strN row: N bytes of string and padding, then the length byte)."""
    if key.startswith("str"):
        return int(key[3:]) + 1
    return int(key[5:]) if key.startswith("bytes") else {"unit": 0, "u32": 4, "u64": 8}[key]


def val_width(value):
    """Bytes of a fixed-width value row; None for "var" (per record)."""
    return int(value[5:]) if value.startswith("bytes") else {"unit": 0, "u32": 4, "u64": 8, "var": None}[value]


def _int(raw) -> int:
    return raw if isinstance(raw, (int, np.integer)) else int.from_bytes(raw, "little")


def key_model(key, raw):
    """pyref's typed key: a strN / bytesN key is the string or array (u64 length, then the bytes),
    whatever row it travels in."""
    return P.Unit() if key == "unit" else P.U32(_int(raw)) if key == "u32" else P.U64(_int(raw)) if key == "u64" else P.Str(raw)


def value_model(value, raw):
    return P.Unit() if value == "unit" else P.U32(_int(raw)) if value == "u32" else P.U64(_int(raw)) if value == "u64" \
        else P.Str(raw)


def canonical(key, value, kind, raw_key, raw_value, stamp=(0, 0, 0), tomb=False) -> bytes:
    """rsos::encoding::encode_to_vec(&k) ++ encode_to_vec(&v) by the oracle's typed model.  A
    tombstone's value is not looked at."""
    state = P.TOMBSTONE if tomb else P.present(value_model(value, raw_value))
    if kind == "plain":
        assert not tomb
        v = value_model(value, raw_value)
    elif kind == "dated":
        v = P.entry(P.timestamp(*stamp), state)
    else:
        v = state
    return P.encode(key_model(key, raw_key)) + P.encode(v)


def msg_len(key, value, kind, klen=None, vlen=None, tomb=False) -> int:
    """Length of canonical(): the key (a strN key of klen bytes), the stamp (dated), the State
    variant (dated / projection), and unless a tombstone the value (a var value of vlen bytes)."""
    k = 8 + klen if key.startswith("str") else key_width(key) + (8 if key.startswith("bytes") else 0)
    v = 8 + vlen if value == "var" else val_width(value) + (8 if value.startswith("bytes") else 0)
    return k + (20 if kind == "dated" else 0) + (0 if kind == "plain" else 4) + (0 if tomb else v)


def prefix_len(key, kind, klen=None) -> int:
    """Everything in front of a var value's bytes, its u64 length included."""
    return msg_len(key, "var", kind, klen, 0)


def tail_len(kind) -> int:
    """The fields between the key and a var value's bytes: stamp, State variant, u64 value length."""
    return prefix_len("unit", kind)


def value_column(value, vals):
    """n rows of a u32 / u64 value column (uint8, n x 4 / 8, little-endian); None for unit."""
    if value == "unit":
        return None
    return np.array(vals, np.uint64).astype({"u32": "<u4", "u64": "<u8"}[value]).view(np.uint8).reshape(len(vals), val_width(value))


# ---- lift cases -------------------------------------------------------------------------------------

def build_lift_case(key, value, kind, tags, n, seed, totals=(), per_total=1, small=(), slots_from=0, edge_klens=(),
                    edge_vals=()):
    """n records of one shape: key rows, stamps, tags, values and each record's canonical bytes.

    Row i's strN key has i % (N + 1) bytes, but for the special rows below.  With tags (and a kind
    that has a State) every 5th row is a tombstone.

    Var values are packed back to back, seeded-random lengths in [0, 300) but for: `per_total`
    present rows per message length in `totals` (value length = total - prefix; a strN row whose
    prefix is longer takes a key 4, 8, ... bytes shorter, a fixed prefix longer than the total
    cannot occur), one row per length in `small`, these drawn from the present rows `slots_from`..;
    for each key length in `edge_klens` three further rows with values of 0, 5 and 100 bytes; the
    last present record has 37 bytes (it ends the heap); tombstone 9 sits over a non-empty span
    (ignored).

    u32 / u64 values are seeded-random odd numbers masked to the width, but for the (row, value)
    pairs of `edge_vals`; a tombstone's value row is nonzero and ignored.

    The order of the draws from `rng` is part of the contract: the callers' cases stay what they
    were."""
    from rsos_hip import pack_str_keys
    rng = np.random.default_rng(seed)
    w, is_str, var = key_width(key), key.startswith("str"), value == "var"
    tagged = tags and kind != "plain"
    tomb = np.array([tagged and i % 5 == 4 for i in range(n)])
    case = {"n": n}
    if is_str:
        klen = np.arange(n) % w
    plen = lambda r: prefix_len(key, kind, int(klen[r]) if is_str else None)  # noqa: E731
    if var:
        lens = rng.integers(0, 300, n)
        present_rows = [i for i in range(n) if not tomb[i]]
        last = present_rows[-1]
        cand = [i for i in present_rows[:-1] if i >= slots_from]
        special = [t for t in totals if is_str or t >= plen(0) for _ in range(per_total)]
        slots = rng.choice(cand, len(special) + len(small), replace=False)
        for r, t in zip(slots, special):
            while plen(r) > t:
                klen[r] -= 4  # same byte alignment
            lens[r] = t - plen(r)
        for r, ln in zip(slots[len(special):], small):
            lens[r] = ln
        taken = set(int(s) for s in slots)
        for length in edge_klens:
            rows = [i for i in cand if klen[i] == length and i not in taken][:3]
            assert len(rows) == 3
            for r, ln in zip(rows, (0, 5, 100)):
                lens[r] = ln
        lens[last] = 37
        if tagged:
            lens[tomb] = 0
            lens[9] = 11
            assert tomb[9]
    else:
        mask = (1 << (8 * val_width(value))) - 1
        vals = [int(x) & mask for x in rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + 1]  # odd: nonzero
        for row, v in edge_vals:
            assert not tomb[row]
            vals[row] = v & mask
    if is_str:
        strs = raw_keys = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in klen]
        case.update(w=w, keys=pack_str_keys(strs, w), strs=strs)
        if var:
            case["klen"] = klen
    else:
        keys = rng.integers(0, 256, (n, max(w, 1)), dtype=np.uint8)[:, :w]
        raw_keys = [k.tobytes() for k in keys]
        case.update(p=plen(0), keys=keys)
    phys = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    logical = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    node = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    case.update(phys=phys, logical=logical, node=node, tags=tomb.astype(np.uint8) if tagged else None, tomb=tomb)
    if var:
        vals = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in lens]
        offsets = np.zeros(n + 1, np.uint64)
        offsets[1:] = np.cumsum(lens)
        case.update(lens=lens, heap=b"".join(vals), offsets=offsets)
    else:
        case.update(vals=vals, values=value_column(value, vals))
    case["blobs"] = [canonical(key, value, kind, raw_keys[i], vals[i], (int(phys[i]), int(logical[i]), int(node[i])),
                               bool(tomb[i])) for i in range(n)]
    return case


def case_value(case, i) -> bytes:
    """Row i's span of a var case's heap."""
    return case["heap"][int(case["offsets"][i]):int(case["offsets"][i + 1])]


def to_device(cols, dev, pad_heap=True):
    """Host columns as device tensors: stamps and value offsets as the signed types torch holds;
    a var heap padded with zeros to a multiple of 4 bytes unless pad_heap is off."""
    import torch
    view = {"phys": np.int64, "logical": np.int32, "node": np.int64, "value_offsets": np.int64}
    cols = {c: v for c, v in cols.items() if v is not None}
    if pad_heap and "value_offsets" in cols:
        heap = np.zeros((cols["values"].size + 3) & ~3, np.uint8)
        heap[:cols["values"].size] = cols["values"]
        cols = dict(cols, values=heap)
    return {c: torch.from_numpy(np.ascontiguousarray(v).view(view.get(c, v.dtype)).copy()).to(dev) for c, v in cols.items()}


def upload_var_heap(heap: bytes, offsets, dev, lead=0, slack=0):
    """A var heap on the device: `lead` bytes of filler, the values, `slack` bytes of filler, then
    filler up to a multiple of 4 (0xA5: a byte read past a value would show)."""
    import torch
    used = lead + len(heap) + slack
    buf = np.full((used + 3) & ~3, 0xA5, np.uint8)
    buf[lead:lead + len(heap)] = np.frombuffer(heap, np.uint8)
    return {"values": torch.from_numpy(buf).to(dev),
            "value_offsets": torch.from_numpy((offsets + np.uint64(lead)).astype(np.int64)).to(dev)}


def host_cols(case, schema, n=None, keys=None):
    """The first n rows of a case's fixed-width columns (copies: the case is shared)."""
    n = case["n"] if n is None else n
    cols = {"keys": (case["keys"] if keys is None else keys)[:n].copy()} if schema.key_row else {}
    if case.get("values") is not None:
        cols["values"] = case["values"][:n].copy()
    if schema.dated_kind:
        cols.update(phys=case["phys"][:n].copy(), logical=case["logical"][:n].copy(), node=case["node"][:n].copy())
    if case["tags"] is not None:
        cols["tags"] = case["tags"][:n].copy()
    return cols


def device_cols(case, schema, dev, lead=0, slack=0, keys=None):
    """A var case as device columns, its heap by upload_var_heap."""
    cols = to_device(host_cols(case, schema, keys=keys), dev)
    cols.update(upload_var_heap(case["heap"], case["offsets"], dev, lead, slack))
    return cols


TELL = {"key lengths": lambda c, i: len(c["strs"][i]), "message lengths": lambda c, i: len(c["blobs"][i]),
        "tombstones": lambda c, i: bool(c["tomb"][i])}


def check_lift(schema, cols, case, want, n=None, tell=("message lengths",)):
    """Every row's fingerprint and every 256-row block sum of the first n rows equal `want`; a
    failure names the first rows that differ and what `tell` lists about them."""
    from rsos_hip import lift_records
    n = case["n"] if n is None else n
    fps, bs = lift_records(schema, cols)
    got, got_bs = fps.cpu().numpy(), bs.cpu().numpy()
    bad = np.nonzero((got != want[:n]).any(axis=1))[0]
    assert bad.size == 0, f"n = {n}: {bad.size} rows differ, first {bad[:8]} (" + ", ".join(
        f"{what} {[TELL[what](case, i) for i in bad[:8]]}" for what in tell) + ")"
    assert got_bs.shape[0] == (n + 255) // 256
    for g in range(got_bs.shape[0]):
        assert fp_int(got_bs[g]) == fold(want[256 * g:min(256 * g + 256, n)]), (n, f"block {g}")


def check_var_lift(dev, schema, case, want, lead, slack, keys=None, tell=("message lengths",)):
    """check_lift of a var case uploaded with `lead` and `slack`; with no slack the first value
    sits at heap offset 0 and the last record ends at the buffer's end."""
    cols = device_cols(case, schema, dev, lead, slack, keys=keys)
    if not slack:
        assert cols["values"].numel() == (int(case["offsets"][-1]) + 3) & ~3 and lead == 0
    check_lift(schema, cols, case, want, tell=tell)


# ---- record tuples and the dict model of a store ----------------------------------------------------

def ragged_records(rng, keys, long_every=0):
    """One dated var record per key: a tenth tombstones, values of 0..199 bytes, with long_every a
    multi-chunk value every so many rows."""
    out = []
    for i, k in enumerate(keys):
        tomb = int(rng.integers(0, 10) == 0)
        ln = int(rng.integers(0, 200))
        if long_every and i % long_every == 7:
            ln = (1500, 3000, 5000, 1024, 960)[(i // long_every) % 5]
        val = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        stamp = (int(rng.integers(1, 1 << 40)), int(rng.integers(0, 1 << 20)), int(rng.integers(1, 1 << 40)))
        out.append((k, stamp, tomb, val))
    return out


class DictModel:
    """key bytes -> (record, oracle fingerprint) for a store of one shape."""

    def __init__(self, key, value, kind="dated"):
        self.key, self.value, self.kind, self.rows = key, value, kind, {}
        self.w = key_width(key)

    def cols(self, recs):
        """Host columns of record tuples; var values ragged."""
        from rsos_hip import pack_str_keys
        if self.key.startswith("str"):
            c = {"keys": pack_str_keys([r[0] for r in recs], self.w)}
        else:
            keys = np.frombuffer(b"".join(r[0] for r in recs), np.uint8).reshape(len(recs), self.w)
            c = {"keys": keys.view(np.uint64).reshape(-1) if self.key == "u64" else keys}
        if self.kind == "dated":
            c.update(phys=np.array([r[1][0] for r in recs], np.uint64), logical=np.array([r[1][1] for r in recs], np.uint32),
                     node=np.array([r[1][2] for r in recs], np.uint64))
        if self.kind != "plain":
            c["tags"] = np.array([r[2] for r in recs], np.uint8)
        if self.value == "var":
            offs = np.zeros(len(recs) + 1, np.uint64)
            offs[1:] = np.cumsum([len(r[3]) for r in recs])
            c.update(values=np.frombuffer(b"".join(r[3] for r in recs), np.uint8), value_offsets=offs)
        elif self.value != "unit":
            c["values"] = value_column(self.value, [r[3] for r in recs])
        return c

    def apply(self, recs, ops):
        """The batch in order (a key met twice keeps its last row), fingerprints from the oracle."""
        import oracle as O
        ins = [r for r, op in zip(recs, ops) if op == 0]
        fps = iter(O.lift_encoded([canonical(self.key, self.value, self.kind, r[0], r[3], r[1], bool(r[2])) for r in ins]))
        for r, op in zip(recs, ops):
            if op == 0:
                self.rows[r[0]] = (r, next(fps).tobytes())
            else:
                self.rows.pop(r[0], None)

    def key_order(self, k):
        """The sort key of the key type's Ord: numeric for u32 / u64, bytes order otherwise."""
        return int.from_bytes(k, "little") if self.key in ("u32", "u64") else k

    def api_key(self, k):
        """The key as the store's Python surface gives it."""
        return self.key_order(k)

    def order(self):
        return sorted(self.rows, key=self.key_order)

    def check(self, st, absent=None):
        """size, root, 16 rank ranges around the block edges, the keys in order, every fingerprint;
        given `absent` keys (a store keyed in bytes order), also rank / select and key-range
        aggregates over every pair of bound kinds, with present and absent keys as bounds"""
        ks = self.order()
        n = len(ks)
        fps = [self.rows[k][1] for k in ks]
        assert st.size() == n
        assert agg_int(st.aggregate()) == fold(fps)
        cuts = sorted({0, n, 1, n // 3, n // 2, n - 1, 255, 256, 257, 511, 512, 513, 700, 768, 1000, 1024, 1025} & set(range(n + 1)))
        lo = [cuts[i % len(cuts)] for i in range(16)]
        hi = [cuts[(i * 5 + 3) % len(cuts)] for i in range(16)]
        for a, l, h in zip(st.aggregates_ranks(lo, hi), lo, hi):
            assert (a.size, agg_int(a)) == ((h - l, fold(fps[l:h])) if h > l else (0, 0)), (l, h)
        assert [k for k, _ in st.enumerate()] == [self.api_key(k) for k in ks]
        assert st.fingerprints(0, n).tobytes() == b"".join(fps)
        if absent is None:
            return
        probes = [ks[i] for i in range(0, n, max(n // 24, 1))] + list(absent)
        for z in probes:
            assert st.rank(z) == bisect.bisect_left(ks, z), z
        for r in (0, 1, n // 2, n - 1):
            assert st.select(r) == ks[r]
        check_key_ranges(st, ks, fps, ((BOUND_KINDS[i % 3], BOUND_KINDS[(i // 3) % 3],
                                        *sorted((probes[(i * 7) % len(probes)], probes[(i * 11 + 3) % len(probes)])))
                                       for i in range(18)))


def check_key_ranges(st, ks, fps, bounds):
    """st.aggregate over key ranges: `bounds` yields (start kind, end kind, a, b), a <= b; the
    expected keys are filtered from ks by the bound kinds ("unbounded" | "included" | "excluded")."""
    from rsos_hip.store import KeyRange
    for lk, hk, a, b in bounds:
        rg = KeyRange(None if lk == "unbounded" else a, None if hk == "unbounded" else b, lk, hk)
        inside = [j for j, k in enumerate(ks)
                  if (lk == "unbounded" or k > a or (lk == "included" and k == a))
                  and (hk == "unbounded" or k < b or (hk == "included" and k == b))]
        got = st.aggregate(rg)
        assert (got.size, agg_int(got)) == (len(inside), fold(fps[j] for j in inside)), (lk, hk, a, b)


BOUND_KINDS = ("unbounded", "included", "excluded")


# ---- columns and the column-style model (tests/test_small_batch.py and the sharded tests) -----------

def oracle_records(O, schema, h):
    """Host columns as the oracle's Records of the same schema."""
    sch = O.Schema(schema.key_kind, schema.key_len, schema.value_kind, schema.value_len, schema.record_kind, 0)
    return O.Records(sch, h.get("keys"), h.get("values"), h.get("phys"), h.get("logical"), h.get("node"), h.get("tags"))


def _gen(rng, sch, n, tombstones):
    """n random host rows of schema sch (keys distinct)."""
    kl, vl = sch.key_row, sch.value_row
    keys = rng.integers(0, 256, size=(n, kl), dtype=np.uint8)
    cols = {"keys": keys, "values": rng.integers(0, 256, size=(n, vl), dtype=np.uint8)}
    if sch.dated_kind:
        cols["phys"] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
        cols["logical"] = rng.integers(0, 1 << 31, size=n, dtype=np.uint32)
        cols["node"] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    if tombstones:
        cols["tags"] = (rng.random(n) < 0.1).astype(np.uint8)
    return cols


def _order(sch, k: bytes):
    return int.from_bytes(k, "little") if sch.key_kind in (1, 2) else k


class ColumnModel:
    """FingerprintTreeMap's contents: key -> fingerprint (last write wins, deletes remove)."""

    def __init__(self, O, sch):
        self.O, self.sch, self.d = O, sch, {}

    def lifts(self, cols):
        return oracle_records(self.O, self.sch, cols).lift()

    def apply(self, cols, ops):
        """rows in order; returns (new, overwritten, deleted) as the store counts them for a batch
        of distinct keys"""
        fps = self.lifts(cols)
        new = over = dele = 0
        for i in range(len(ops)):
            k = cols["keys"][i].tobytes()
            live = k in self.d
            if ops[i]:
                dele += live
                self.d.pop(k, None)
            else:
                new += not live
                over += live
                self.d[k] = fps[i].tobytes()
        return new, over, dele

    def root(self):
        return fold(self.d.values()), len(self.d)

    def sorted_keys(self):
        return sorted(self.d, key=lambda k: _order(self.sch, k))


def _batch(rng, sch, model, m, tombstones, repeats=False):
    """m rows: fresh keys, overwrites of live keys, deletes of live and of absent keys; with
    repeats, some keys appear two or three times (staged rows only)."""
    cols = _gen(rng, sch, m, tombstones)
    ops = np.zeros(m, np.uint8)
    live = model.sorted_keys()
    if live:
        for i in range(m):
            u = rng.random()
            if u < 0.2:  # overwrite a live key
                cols["keys"][i] = np.frombuffer(live[rng.integers(len(live))], np.uint8)
            elif u < 0.27:  # delete a live key
                cols["keys"][i] = np.frombuffer(live[rng.integers(len(live))], np.uint8)
                ops[i] = 1
            elif u < 0.3:  # delete an absent key
                ops[i] = 1
    if repeats and m > 2:
        for i in range(1, m, 3):
            cols["keys"][i] = cols["keys"][i - 1]
            ops[i] = rng.integers(0, 2)
    if not repeats:  # distinct keys: keep the first of any accidental repeat
        _, first = np.unique(cols["keys"], axis=0, return_index=True)
        keep = np.sort(first)
        cols = {c: v[keep] for c, v in cols.items()}
        ops = ops[keep]
    return cols, ops


# ---- what the sharded and route tests share ---------------------------------------------------------

def _sorted_unique(sch, cols):
    k = cols["keys"]
    if sch.key_kind in (1, 2):
        order = np.argsort(k.copy().view("<u4" if sch.key_row == 4 else "<u8").ravel(), kind="stable")
    else:
        order = np.lexsort(k.T[::-1])
    cols = {c: v[order] for c, v in cols.items()}
    _, first = np.unique(cols["keys"], axis=0, return_index=True)
    keep = np.sort(first)
    return {c: v[keep] for c, v in cols.items()}


def _drive(a, b, policy):
    """a whole reconciliation between two maps, native rounds: every round's output"""
    from rsos_hip import rbsr as R
    out, active, sides, k = [], R.initial_ranges(a), [b, a], 0
    while active and k < 64:
        ch, en = [], []
        o = R.protocol_round_with_policy(sides[k % 2], policy, active, ch, en)
        out.append(([(c.start, c.end, c.aggregate) for c in ch], en,
                    (o.skipped, o.enumerated, o.split, o.children, o.dropped_malformed)))
        active, k = ch, k + 1
    return out


def _devices(shards):
    import torch
    return [s % torch.cuda.device_count() for s in range(shards)]


def _key_rows(st):
    from rsos_hip import _abi as A
    n, kl = st.size(), st.schema.key_row
    out = np.zeros((max(n, 1), kl), np.uint8)
    A.check(st._f("keys")(st._h, 0, n, out.ctypes.data if n else None), "keys")
    return out[:n]


def _state(st, probes, ranges, selects):
    """len, root, key-range aggregates, ranks, selects, the key and fingerprint dumps, in a form that compares with =="""
    from rsos_hip.store import KeyRange
    n = st.size()
    return {
        "len": n,
        "root": st.aggregate(),
        "ranges": [st.aggregate(KeyRange(st._key_out(a.tobytes()), st._key_out(b.tobytes()))) for a, b in ranges],
        "ranks": st.ranks(probes).tolist(),
        "selects": [st.select(r) for r in selects if r < n],
        "keys": _key_rows(st).tobytes(),
        "fps": st.fingerprints().tobytes(),
    }


def _same(maps, rng, peer=None):
    """all of `maps` (the device-fed map first) hold the same state"""
    from rsos_hip import rbsr as R
    rows = _key_rows(maps[0])
    n, kl = rows.shape[0], maps[0].schema.key_row
    pick = rows[rng.integers(0, n, 150)] if n else np.zeros((0, kl), np.uint8)
    near = pick[:50].copy()
    if len(near):
        near[:, kl // 2] ^= 1  # keys that are mostly absent, next to present ones
    probes = np.ascontiguousarray(np.concatenate([pick, near]))
    order = np.lexsort(probes.T[::-1]) if maps[0].schema.key_kind not in (1, 2) else \
        np.argsort(probes.copy().view("<u4" if kl == 4 else "<u8").ravel())
    srt = probes[order]
    ranges = [(srt[i], srt[-1 - i]) for i in range(min(16, len(srt) // 2))]
    selects = sorted(set(int(x) for x in rng.integers(0, max(n, 1), 40)) | {0, max(n - 1, 0)})
    want = _state(maps[0], probes, ranges, selects)
    assert want["len"] == n
    for other in maps[1:]:
        got = _state(other, probes, ranges, selects)
        for k in want:
            assert got[k] == want[k], k
    if peer is not None:
        rounds = _drive(maps[0], peer, R.FixedFanOut(16))
        for other in maps[1:]:
            assert _drive(other, peer, R.FixedFanOut(16)) == rounds


def _dump(st):
    return st.size(), st.aggregate(), _key_rows(st).tobytes(), st.fingerprints().tobytes()


def _key_ints(sch, rows):
    """each key row as a Python int whose order is the key order"""
    rows = np.ascontiguousarray(rows).reshape(-1, sch.key_row)
    if sch.key_kind in (1, 2):
        return rows.view("<u4" if sch.key_row == 4 else "<u8").ravel().astype(object)
    out = np.empty(len(rows), object)
    for i, r in enumerate(rows):
        out[i] = int.from_bytes(r.tobytes(), "big")
    return out


def _splitters(rng, sch, shards, cols):
    """shards - 1 non-decreasing key rows: some drawn from the batch's own keys (a key equal to a
    splitter belongs to the shard above it), the rest random"""
    kl = sch.key_row
    sp = rng.integers(0, 256, size=(shards - 1, kl), dtype=np.uint8)
    n = len(cols["keys"])
    for j in range(0, shards - 1, 2):
        if n:
            sp[j] = cols["keys"][rng.integers(0, n)]
    order = np.argsort(_key_ints(sch, sp), kind="stable") if shards > 1 else np.zeros(0, np.int64)
    return np.ascontiguousarray(sp[order])
