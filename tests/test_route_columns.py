"""rh_route_columns_device (csrc/shard_route.hip): device columns partitioned by the sharded store's
splitters, bit-exact against a numpy stable partition -- np.searchsorted(splitters, keys, "right")
(rh_sstore's owner(): bisect_right in the key type's Ord), then a stable argsort.

Every row count at which the kernels take another path (0, one row, around the 16-row alignment,
around a 256-thread step, more than one 2,048-row tile, and 70,001 rows: 35 tiles, so that the scan
over (shard, tile) leaves one scan block for 64 shards), every shard count class (1, a power of two,
an odd one, the limit 64), every key order (u32 / u64 numeric; 8-, 16-, 32-, 64-byte rows by
memcmp) and every column mover (1-, 4-, 8- and 16-byte units; a 1 KiB value row copied by a whole
wave).  Invariants: segment starts are multiples of 16, gap rows are zero, nothing past cap_rows or
past the last segment is written, counts sum to n.  The argument checks run without a GPU."""
import ctypes as C

import numpy as np
import pytest

from records_common import _key_ints, _splitters

NS = [0, 1, 15, 16, 17, 255, 256, 257, 4097, 70001]
GS = [1, 2, 4, 7, 64]
GUARD = 0xA5
GUARD_ROWS = 8

# (name, record kind, key, value, tags, ops, row counts)
SCHEMAS = [
    ("u64-u64-plain", "plain", "u64", "u64", False, False, NS),
    ("u32-unit", "plain", "u32", "unit", False, False, NS),
    ("b16-b64-dated-tags-ops", "dated", "bytes16", "bytes64", True, True, NS),
    ("b32-u32-projection", "projection", "bytes32", "u32", True, False, NS),
    ("str31-u64-dated", "dated", "str31", "u64", False, False, NS),
    ("b64-rows", "plain", "bytes64", "u32", False, True, NS),
    ("b8-rows", "plain", "bytes8", "u64", False, False, [257, 4097]),
    ("b16-1KiB", "plain", "bytes16", "bytes1024", False, False, [300]),
]


def _schema(kind, key, value):
    from rsos_hip import RecordSchema
    return getattr(RecordSchema, kind)(key, value)


def _gen(rng, sch, n, tags, ops, few_keys=0):
    kl, vl = sch.key_row, sch.value_row
    keys = rng.integers(0, 256, size=(n, kl), dtype=np.uint8)
    if few_keys and n:  # long runs of equal leading bytes: the order is decided late in the row
        keys[:, : kl - 2] = keys[rng.integers(0, min(few_keys, n), n), : kl - 2]
    cols = {"keys": keys}
    if vl:
        cols["values"] = rng.integers(0, 256, size=(n, vl), dtype=np.uint8)
    if sch.dated_kind:
        cols["phys"] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
        cols["logical"] = rng.integers(0, 1 << 31, size=n, dtype=np.uint32)
        cols["node"] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    if tags:
        cols["tags"] = (rng.random(n) < 0.3).astype(np.uint8)
    return cols, ((rng.random(n) < 0.4).astype(np.uint8) if ops else None)


def _route_and_check(gpu, sch, sp, shards, cols, ops):
    """route on the device into guarded columns; everything checked against the numpy partition"""
    import torch
    from rsos_hip.device import route_columns
    n = len(cols["keys"])
    cap = n + 16 * shards
    dcols = {c: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for c, v in cols.items()}
    dops = None if ops is None else torch.from_numpy(ops).to(gpu)
    row_bytes = {c: int(np.prod(v.shape[1:], dtype=np.int64)) * v.dtype.itemsize for c, v in cols.items()}
    out = {c: torch.full(((cap + GUARD_ROWS) * row_bytes[c],), GUARD, dtype=torch.uint8, device=gpu) for c in dcols}
    oops = None if ops is None else torch.full((cap + GUARD_ROWS,), GUARD, dtype=torch.uint8, device=gpu)
    _, _, counts, starts = route_columns(sch, sp, shards, dcols, dops, out=out, ops_out=oops, cap_rows=cap)
    counts, starts = counts.astype(np.int64), starts.astype(np.int64)
    # the numpy stable partition
    owner = np.searchsorted(_key_ints(sch, sp), _key_ints(sch, cols["keys"]), side="right").astype(np.int64) \
        if shards > 1 else np.zeros(n, np.int64)
    perm = np.argsort(owner, kind="stable")
    want_counts = np.bincount(owner, minlength=shards)
    assert counts.tolist() == want_counts.tolist() and counts.sum() == n
    assert (starts % 16 == 0).all()
    pad = (counts + 15) // 16 * 16
    assert starts.tolist() == (np.cumsum(pad) - pad).tolist()
    used = int(starts[-1] + pad[-1])
    assert used <= cap
    host = dict(cols, ops=ops) if ops is not None else dict(cols)
    got = {c: (oops if c == "ops" else out[c]).cpu().numpy() for c in host}
    for c, src in host.items():
        rb = row_bytes.get(c, 1)
        g = got[c].reshape(cap + GUARD_ROWS, rb)
        s = np.ascontiguousarray(src).view(np.uint8).reshape(n, rb)
        at = 0
        for t in range(shards):
            a, k = int(starts[t]), int(counts[t])
            assert (g[a:a + k] == s[perm[at:at + k]]).all(), (c, t)
            assert not g[a + k:a + int(pad[t])].any(), (c, t, "gap rows are zero")
            at += k
        assert (g[used:] == GUARD).all(), (c, "rows past the last segment, and the guard past cap_rows")


@pytest.mark.gpu
@pytest.mark.parametrize("shards", GS)
@pytest.mark.parametrize("spec", SCHEMAS, ids=lambda s: s[0])
def test_route_is_the_numpy_stable_partition(gpu, spec, shards):
    name, kind, key, value, tags, ops, ns = spec
    sch = _schema(kind, key, value)
    rng = np.random.default_rng(1000 + shards)
    for n in ns:
        cols, o = _gen(rng, sch, n, tags, ops, few_keys=5 if sch.key_row >= 16 else 0)
        _route_and_check(gpu, sch, _splitters(rng, sch, shards, cols), shards, cols, o)


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["one_shard_low", "one_shard_high", "every_other_empty", "keys_are_splitters",
                                   "all_splitters_equal", "all_keys_equal"])
@pytest.mark.parametrize("shards", [7, 64])
def test_route_adversarial_placements(gpu, place, shards):
    sch = _schema("dated", "bytes16", "bytes64")
    rng = np.random.default_rng(77)
    n = 4097
    cols, ops = _gen(rng, sch, n, True, True)
    kl = sch.key_row
    if place == "one_shard_low":  # every key below every splitter
        cols["keys"][:, 0] &= 0x7F
        sp = np.full((shards - 1, kl), 0xFF, np.uint8)
        sp[:, -1] = np.arange(shards - 1)
    elif place == "one_shard_high":  # every key at or above every splitter: the last shard
        sp = np.zeros((shards - 1, kl), np.uint8)
    elif place == "every_other_empty":  # splitters in equal pairs: the shard between a pair holds nothing
        sp = _splitters(rng, sch, shards, cols)
        sp[1::2] = sp[0:-1:2][: len(sp[1::2])]
        sp = sp[np.argsort(_key_ints(sch, sp), kind="stable")]
    elif place == "keys_are_splitters":  # every key equals some splitter: bisect_right puts it above
        sp = _splitters(rng, sch, shards, cols)
        cols["keys"][:] = sp[rng.integers(0, shards - 1, n)]
    elif place == "all_splitters_equal":
        sp = np.repeat(cols["keys"][:1], shards - 1, axis=0)
    else:  # all_keys_equal
        cols["keys"][:] = cols["keys"][0]
        sp = _splitters(rng, sch, shards, cols)
    _route_and_check(gpu, sch, np.ascontiguousarray(sp), shards, cols, ops)


def test_route_argument_checks_come_before_any_device_call(rsos_hip_lib):
    """NULLs, shards outside 1..64, cap_rows too small, VARBYTES and decreasing splitters are refused
    on the arguments alone (this test runs without a GPU), and n = 0 answers without a device call."""
    from rsos_hip import RecordSchema, _abi as A
    L = A.lib()
    s = RecordSchema.plain("u64", "u64").c()
    cols, out = A.Columns(), A.Columns()
    cnt, st = (C.c_uint64 * 64)(), (C.c_uint64 * 64)()
    sp = np.arange(1, 64, dtype=np.uint64)
    spp = sp.ctypes.data
    fake = 0x1000  # never dereferenced: every call below fails (or answers) before a device call

    def call(schema=s, splitters=spp, shards=4, cin=cols, n=100, cout=out, cap=100 + 64, counts=cnt, starts=st):
        return L.rh_route_columns_device(C.byref(schema) if schema is not None else None, splitters, shards,
                                         C.byref(cin) if cin is not None else None, None, n,
                                         C.byref(cout) if cout is not None else None, None, cap, counts, starts, None)

    assert call(schema=None) == A.ERR_ARG
    for shards in (0, -1, 65):
        assert call(shards=shards) == A.ERR_ARG and "1..64" in L.rh_last_error().decode()
    assert call(counts=None) == A.ERR_ARG and call(starts=None) == A.ERR_ARG
    assert call(splitters=None) == A.ERR_ARG
    assert call(cap=100 + 63) == A.ERR_ARG and "cap_rows" in L.rh_last_error().decode()
    assert call(cin=None) == A.ERR_ARG and call(cout=None) == A.ERR_ARG
    assert call() == A.ERR_ARG and "keys" in L.rh_last_error().decode()  # NULL key column
    cols.keys, cols.values, out.keys = fake, fake, fake
    assert call() == A.ERR_ARG and "values" in L.rh_last_error().decode()  # given, but no room for it in the output
    out.values = fake + 8
    assert call() == A.ERR_ARG and "16-byte aligned" in L.rh_last_error().decode()
    var = RecordSchema.plain("u64", "var").c()
    assert call(schema=var) == A.ERR_UNSUPPORTED and "VARBYTES" in L.rh_last_error().decode()
    odd = RecordSchema.plain("bytes12", "u64").c()
    assert call(schema=odd) == A.ERR_UNSUPPORTED
    bad = sp.copy()
    bad[1] = 0  # 1, 0, 3: decreases
    assert call(splitters=bad.ctypes.data) == A.ERR_ARG and "must not decrease" in L.rh_last_error().decode()
    assert call(n=1 << 32, cap=(1 << 32) + 64) == A.ERR_ARG
    # n = 0: zero counts and starts, no column is looked at
    cnt[0] = st[1] = 7
    assert call(cin=None, cout=None, n=0, cap=64) == A.OK
    assert list(cnt[:4]) == [0, 0, 0, 0] and list(st[:4]) == [0, 0, 0, 0]
