"""rh_route_columns_var_device (csrc/shard_route.hip): the ragged form of the route.  The row partition
is rh_route_columns_device's (counts, starts, 16-row segment starts, zeroed gap rows); a VARBYTES value
column travels with it: every row's span, clipped as the snapshot encode clips it, packed in output-row
order into a heap, offsets[0 .. R] written, the bytes up to the next multiple of 4 zeroed.

The model is a numpy stable partition (np.searchsorted(splitters, keys, "right"), a stable argsort)
and the clip rule: a span that decreases or starts past bytes_len is empty, one that ends past it is
cut there.  Row counts: one tile of 2,048 rows, its edges, three tiles.  Value lengths: 0, 1..7,
63..65, 1023..1025 and one value of 5,000 bytes, the input heap with a lead of 0..3 bytes so that
source and destination starts take every residue mod 4; the output heap at every 4-byte alignment
inside a 16-byte granule.  Sentinels past the heap's capacity and past offsets[R] must survive."""
import ctypes as C

import numpy as np
import pytest

from records_common import _key_ints, _splitters

NS = [1, 15, 17, 2047, 2049, 5000]
GS = [1, 2, 7, 64]
LENS = [0, 1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 1023, 1024, 1025]
GUARD = 0xA5
OFF_GUARD = 0xA5A5A5A5A5A5A5A5
SPECS = [("str31-var-dated-tags-ops", "dated", "str31", True, True), ("u64-var-plain", "plain", "u64", False, False)]


def _schema(kind, key):
    from rsos_hip import RecordSchema
    return getattr(RecordSchema, kind)(key, "var")


def _gen(rng, sch, n, tags, ops, lead):
    """n host rows: fixed columns, and values packed behind `lead` bytes; one value of 5,000 bytes"""
    kl = sch.key_row
    if sch.key_kind in (1, 2):
        keys = rng.integers(0, 256, size=(n, kl), dtype=np.uint8)
    else:  # string rows: L bytes, zero padding, the length in the last byte
        keys = np.zeros((n, kl), np.uint8)
        for i in range(n):
            L = int(rng.integers(0, kl))
            keys[i, :L] = rng.integers(1, 256, L, dtype=np.uint8)
            keys[i, kl - 1] = L
    cols = {"keys": keys}
    if sch.dated_kind:
        cols["phys"] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
        cols["logical"] = rng.integers(0, 1 << 31, size=n, dtype=np.uint32)
        cols["node"] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    if tags:
        cols["tags"] = (rng.random(n) < 0.3).astype(np.uint8)
    if n > 64:  # mostly short values, a few long ones: the heap stays small
        lens = np.array(LENS)[rng.integers(0, len(LENS), n)]
        short = rng.random(n) < 0.9
        lens[short] = rng.integers(0, 8, int(short.sum()))
        lens[:len(LENS)] = LENS  # every length is present
        lens[n // 2] = 5000
    else:
        lens = np.array(LENS)[rng.integers(0, 11, n)]
        lens[0] = 5000
    offs = np.zeros(n + 1, np.uint64)
    offs[0] = lead
    offs[1:] = lead + np.cumsum(lens)
    total = int(offs[n])
    heap = rng.integers(0, 256, (total + 3) // 4 * 4, dtype=np.uint8)
    cols["values"], cols["value_offsets"] = heap, offs
    return cols, ((rng.random(n) < 0.4).astype(np.uint8) if ops else None)


def _clip(offs, limit):
    """(source start, length) per row under the clip rule"""
    o0, o1 = offs[:-1].astype(object), offs[1:].astype(object)
    src = np.zeros(len(o0), np.int64)
    ln = np.zeros(len(o0), np.int64)
    for i in range(len(o0)):
        if o0[i] > limit or o1[i] < o0[i]:
            continue
        src[i], ln[i] = int(o0[i]), int(min(o1[i], limit) - o0[i])
    return src, ln


def _model(sch, sp, shards, cols):
    """the partition and the routed value column: counts, starts, pad, perm, per-output-row (src, len)"""
    n = len(cols["keys"])
    owner = np.searchsorted(_key_ints(sch, sp), _key_ints(sch, cols["keys"]), side="right").astype(np.int64) \
        if shards > 1 else np.zeros(n, np.int64)
    perm = np.argsort(owner, kind="stable")
    counts = np.bincount(owner, minlength=shards)
    pad = (counts + 15) // 16 * 16
    starts = np.cumsum(pad) - pad
    R = int(starts[-1] + pad[-1])
    src, ln = _clip(cols["value_offsets"], len(cols["values"]))
    osrc, olen = np.zeros(R, np.int64), np.zeros(R, np.int64)
    at = 0
    for t in range(shards):
        a, k = int(starts[t]), int(counts[t])
        osrc[a:a + k], olen[a:a + k] = src[perm[at:at + k]], ln[perm[at:at + k]]
        at += k
    woffs = np.concatenate([[0], np.cumsum(olen)]).astype(np.uint64)
    heap = cols["values"]
    wheap = np.concatenate([heap[s:s + l] for s, l in zip(osrc, olen) if l] or [np.zeros(0, np.uint8)])
    return counts, starts, pad, perm, R, woffs, wheap


def _route_and_check(gpu, sch, sp, shards, cols, ops, mis=0, cap=None, expect_fail=False):
    """route into guarded buffers (the output heap `mis` bytes past a 16-byte boundary); everything
    against the model.  cap: the output heap's capacity (default: roundup4 of the model's total)"""
    import torch
    from rsos_hip import _abi as A
    from rsos_hip.device import route_columns_var
    n = len(cols["keys"])
    cap_rows = n + 16 * shards
    counts_w, starts_w, pad, perm, R, woffs, wheap = _model(sch, sp, shards, cols)
    total = int(woffs[R])
    if cap is None:
        cap = (total + 3) // 4 * 4
    fixed = {c: v for c, v in cols.items() if c not in ("values", "value_offsets")}
    dcols = {c: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for c, v in cols.items()}
    dcols["value_offsets"] = torch.from_numpy(cols["value_offsets"].view(np.int64)).to(gpu)
    dops = None if ops is None else torch.from_numpy(ops).to(gpu)
    row_bytes = {c: int(np.prod(v.shape[1:], dtype=np.int64)) * v.dtype.itemsize for c, v in fixed.items()}
    out = {c: torch.full(((cap_rows + 8) * row_bytes[c],), GUARD, dtype=torch.uint8, device=gpu) for c in fixed}
    raw = torch.full((16 + cap + 64,), GUARD, dtype=torch.uint8, device=gpu)
    out["values"] = raw[mis:mis + cap + 64]  # the call is told `cap`: the 64 bytes behind it are sentinels
    out["value_offsets"] = torch.from_numpy(np.full(cap_rows + 1 + 8, OFF_GUARD, np.uint64).view(np.int64)).to(gpu)
    oops = None if ops is None else torch.full((cap_rows + 8,), GUARD, dtype=torch.uint8, device=gpu)

    def sentinels():
        r = raw.cpu().numpy()
        assert (r[:mis] == GUARD).all() and (r[mis + cap:] == GUARD).all(), "bytes outside the heap's capacity"
        o = out["value_offsets"].cpu().numpy().view(np.uint64)
        assert (o[R + 1:] == OFF_GUARD).all(), "offsets past index R"

    if expect_fail:
        with pytest.raises(A.RsosHipError) as e:
            route_columns_var(sch, sp, shards, dcols, dops, out=out, ops_out=oops, cap_rows=cap_rows, heap_cap=cap)
        assert e.value.code == A.ERR_ARG
        sentinels()
        return
    _, _, counts, starts, heap_bytes = route_columns_var(sch, sp, shards, dcols, dops, out=out, ops_out=oops,
                                                         cap_rows=cap_rows, heap_cap=cap)
    counts, starts = counts.astype(np.int64), starts.astype(np.int64)
    assert counts.tolist() == counts_w.tolist() and counts.sum() == n
    assert starts.tolist() == starts_w.tolist() and (starts % 16 == 0).all()
    # every fixed column, as test_route_columns.py checks it
    host = dict(fixed, ops=ops) if ops is not None else dict(fixed)
    for c, src in host.items():
        rb = row_bytes.get(c, 1)
        g = (oops if c == "ops" else out[c]).cpu().numpy().reshape(cap_rows + 8, rb)
        s = np.ascontiguousarray(src).view(np.uint8).reshape(n, rb)
        at = 0
        for t in range(shards):
            a, k = int(starts[t]), int(counts[t])
            assert (g[a:a + k] == s[perm[at:at + k]]).all(), (c, t)
            assert not g[a + k:a + int(pad[t])].any(), (c, t, "gap rows are zero")
            at += k
        assert (g[R:] == GUARD).all(), (c, "rows past the last segment")
    # the value column
    assert heap_bytes == total
    goffs = out["value_offsets"].cpu().numpy().view(np.uint64)
    assert (goffs[:R + 1] == woffs).all()
    gheap = raw.cpu().numpy()[mis:mis + (total + 3) // 4 * 4]
    assert (gheap[:total] == wheap).all()
    assert not gheap[total:].any(), "the bytes up to the next multiple of 4 are zeroed"
    sentinels()


def test_generated_values_cover_the_cases():
    """source and destination value starts take every residue mod 4, a value is longer than 1 KiB"""
    sch = _schema("plain", "u64")
    src_res, dst_res, longest = set(), set(), 0
    for lead in range(4):
        rng = np.random.default_rng(lead)
        cols, _ = _gen(rng, sch, 2049, False, False, lead)
        assert int(cols["value_offsets"][0]) == lead
        sp = _splitters(rng, sch, 7, cols)
        _, _, _, _, R, woffs, _ = _model(sch, sp, 7, cols)
        lens = np.diff(cols["value_offsets"].astype(np.int64))
        src_res |= set((cols["value_offsets"][:-1][lens > 0] % 4).tolist())
        dst_res |= set((woffs[:-1][np.diff(woffs.astype(np.int64)) > 0] % 4).tolist())
        longest = max(longest, int(lens.max()))
        assert set(LENS) <= set(lens.tolist())
    assert src_res == {0, 1, 2, 3} and dst_res == {0, 1, 2, 3} and longest == 5000 > 1024


@pytest.mark.gpu
@pytest.mark.parametrize("shards", GS)
@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s[0])
def test_ragged_route_is_the_numpy_stable_partition(gpu, spec, shards):
    name, kind, key, tags, ops = spec
    sch = _schema(kind, key)
    rng = np.random.default_rng(2000 + shards)
    for j, n in enumerate(NS):
        cols, o = _gen(rng, sch, n, tags, ops, lead=j % 4)
        _route_and_check(gpu, sch, _splitters(rng, sch, shards, cols), shards, cols, o, mis=4 * (j % 4))


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["all_first", "all_last", "empty_middle", "alternating_far", "sorted", "keys_are_splitters"])
@pytest.mark.parametrize("shards", [7, 64])
def test_ragged_route_placements(gpu, place, shards):
    sch = _schema("plain", "u64")
    rng = np.random.default_rng(91)
    n = 2049
    cols, _ = _gen(rng, sch, n, False, False, lead=3)
    k = cols["keys"].view("<u8").ravel()
    k[:] = rng.integers(1 << 20, 1 << 62, n, dtype=np.uint64)
    sp = np.sort(rng.integers(1 << 20, 1 << 62, shards - 1, dtype=np.uint64))
    if place == "all_first":
        k[:] = rng.integers(0, 1 << 20, n, dtype=np.uint64)
    elif place == "all_last":
        k[:] = (1 << 63) + rng.integers(0, 1 << 20, n, dtype=np.uint64)
    elif place == "empty_middle":
        sp[shards // 2] = sp[shards // 2 - 1]  # equal splitters: the shard between them holds nothing
    elif place == "alternating_far":
        k[0::2] = rng.integers(0, 1 << 20, len(k[0::2]), dtype=np.uint64)
        k[1::2] = (1 << 63) + rng.integers(0, 1 << 20, len(k[1::2]), dtype=np.uint64)
    elif place == "sorted":
        k.sort()
    else:  # every key equals a splitter: bisect_right puts it in the shard above
        k[:] = sp[rng.integers(0, shards - 1, n)]
    _route_and_check(gpu, sch, np.ascontiguousarray(sp).view(np.uint8).reshape(shards - 1, 8), shards, cols, None, mis=8)


@pytest.mark.gpu
def test_heap_capacity_is_exact(gpu):
    """roundup4(total) bytes suffice; 4 bytes less is RH_ERR_ARG with nothing written outside the buffers"""
    sch = _schema("dated", "str31")
    rng = np.random.default_rng(5)
    cols, ops = _gen(rng, sch, 2049, True, True, lead=1)
    sp = _splitters(rng, sch, 7, cols)
    total = int(_model(sch, sp, 7, cols)[5][-1])
    cap = (total + 3) // 4 * 4
    _route_and_check(gpu, sch, sp, 7, cols, ops, mis=4, cap=cap)
    _route_and_check(gpu, sch, sp, 7, cols, ops, mis=4, cap=cap - 4, expect_fail=True)
    # the input heap's own size always suffices
    _route_and_check(gpu, sch, sp, 7, cols, ops, mis=12, cap=len(cols["values"]))


@pytest.mark.gpu
def test_malformed_offsets_follow_the_clip_model(gpu):
    """decreasing offsets and offsets past bytes_len: the output is the clip model's, nothing outside"""
    sch = _schema("plain", "u64")
    rng = np.random.default_rng(6)
    cols, _ = _gen(rng, sch, 2049, False, False, lead=2)
    offs, limit = cols["value_offsets"], len(cols["values"])
    offs[100] = offs[90]              # decreases at 100, a long span behind it
    offs[500:520] = limit + 1000      # starts past the heap
    offs[900] = limit + 7             # row 899 ends past the heap: cut there; row 900 starts past it
    offs[1500] = np.uint64(1 << 63)   # far past
    sp = _splitters(rng, sch, 7, cols)
    total = int(_model(sch, sp, 7, cols)[5][-1])
    _route_and_check(gpu, sch, sp, 7, cols, None, mis=4, cap=(max(total, limit) + 3) // 4 * 4)


def test_argument_checks_come_before_any_device_call(rsos_hip_lib):
    """Both symbols exist; NULLs, a misaligned heap, bytes_len not a multiple of 4, cap_rows too small
    and an unknown create flag are refused on the arguments alone (no GPU here); the old entry points
    still refuse VARBYTES."""
    from rsos_hip import RecordSchema, _abi as A
    L = A.lib()
    assert L.rh_route_columns_var_device and L.rh_sstore_create_flags
    var = RecordSchema.plain("u64", "var").c()
    fix = RecordSchema.plain("u64", "u64").c()
    cols, out = A.Columns(), A.Columns()
    cnt, st, hb = (C.c_uint64 * 64)(), (C.c_uint64 * 64)(), C.c_uint64(7)
    sp = np.arange(1, 64, dtype=np.uint64)
    fake = 0x1000  # never dereferenced
    vin, vout = A.VarValues(fake, fake, 64), A.VarValues(fake, fake, 64)

    def call(schema=var, cin=cols, n=100, cout=out, cap=100 + 64, counts=cnt, heap=hb):
        return L.rh_route_columns_var_device(C.byref(schema), sp.ctypes.data, 4, C.byref(cin) if cin is not None else None,
                                             None, n, C.byref(cout) if cout is not None else None, None, cap, counts, st,
                                             C.byref(heap) if heap is not None else None, None)

    assert call(heap=None) == A.ERR_ARG and "heap_bytes" in L.rh_last_error().decode()
    assert call(counts=None) == A.ERR_ARG
    assert call(cap=100 + 63) == A.ERR_ARG and "cap_rows" in L.rh_last_error().decode()
    assert call(cin=None) == A.ERR_ARG and call(cout=None) == A.ERR_ARG
    assert call() == A.ERR_ARG and "keys" in L.rh_last_error().decode()
    cols.keys, out.keys = fake, fake
    assert call() == A.ERR_ARG and "values" in L.rh_last_error().decode()  # no rh_var_values given
    cols.values, out.values = C.addressof(vin), C.addressof(vout)
    vout.bytes = fake + 2
    assert call() == A.ERR_ARG and "4-byte aligned" in L.rh_last_error().decode()
    vout.bytes, vout.bytes_len = fake, 62
    assert call() == A.ERR_ARG and "multiple of 4" in L.rh_last_error().decode()
    vout.bytes_len, vin.bytes_len = 64, 63
    assert call() == A.ERR_ARG and "multiple of 4" in L.rh_last_error().decode()
    vin.bytes_len, vout.offsets = 64, fake + 4
    assert call() == A.ERR_ARG and "8-byte aligned" in L.rh_last_error().decode()
    vout.offsets = None
    assert call() == A.ERR_ARG
    # n = 0 answers without a device call; a fixed-width schema reports heap_bytes = 0
    assert call(cin=None, cout=None, n=0, cap=64) == A.OK and hb.value == 0
    hb.value = 7
    assert call(schema=fix, cin=None, cout=None, n=0, cap=64) == A.OK and hb.value == 0
    # the create flags
    devs, h = (C.c_int * 1)(0), C.c_void_p()
    assert L.rh_sstore_create_flags(devs, 1, C.byref(var), 2, C.byref(h)) == A.ERR_ARG
    assert "flag" in L.rh_last_error().decode()
    assert L.rh_sstore_create_flags(devs, 1, C.byref(var), 0, C.byref(h)) == A.ERR_UNSUPPORTED
    flagless = L.rh_last_error().decode()
    assert L.rh_sstore_create(devs, 1, C.byref(var), C.byref(h)) == A.ERR_UNSUPPORTED
    assert L.rh_last_error().decode() == flagless and "VARBYTES" in flagless
    assert L.rh_sstore_create_flags(None, 1, C.byref(var), A.SSTORE_VARBYTES, C.byref(h)) == A.ERR_ARG
    odd = RecordSchema.plain("bytes12", "var").c()
    assert L.rh_sstore_create_flags(devs, 1, C.byref(odd), A.SSTORE_VARBYTES, C.byref(h)) < 0
    # the fixed-width route still refuses VARBYTES
    assert L.rh_route_columns_device(C.byref(var), sp.ctypes.data, 4, C.byref(cols), None, 100, C.byref(out), None, 164,
                                     cnt, st, None) == A.ERR_UNSUPPORTED
    assert "VARBYTES" in L.rh_last_error().decode()
