"""The sharded store with variable-length values (rh_sstore_create_flags, RH_SSTORE_VARBYTES): a
String -> String map and a u64 -> Vec<u8> map over 4, 1 and 7 shards.

Shard s sits on device s % device_count: on a box with one GPU that is device 0 throughout, and the
copy of a segment's offsets and heap span to a shard on another device is then not exercised.

Every state is compared three ways, as tests/test_sharded_device.py does for fixed-width values: the
flagged map fed device columns (load_bulk_device / apply_device: the ragged route on the GPU), one
rh_store fed the same device columns, and a second flagged map fed the same rows through the host
route (each shard's values packed into a heap of its own) -- len, root, 16 key-range aggregates,
ranks, selects, the key dump, the fingerprint dump, and one FixedFanOut(16) reconciliation round by
round against a peer."""
import numpy as np
import pytest

from ragged_snapshot_common import gen_records, ordered, schemas, to_dev, write_snapshot
from records_common import _devices, _dump, _same

SPECS = [("dated", "str31", True), ("plain", "u64", False)]


def _gen(rng, sch, n, tomb):
    """n host rows with distinct keys: one value of 1,500 bytes, some empty, the rest short"""
    kl = sch.key_row
    if sch.key_kind in (1, 2):
        keys = rng.integers(0, 256, size=(n, kl), dtype=np.uint8)
    else:
        keys = np.zeros((n, kl), np.uint8)
        for i in range(n):
            L = int(rng.integers(6, kl))
            keys[i, :L] = rng.integers(1, 256, L, dtype=np.uint8)
            keys[i, kl - 1] = L
    cols = {"keys": keys}
    if sch.dated_kind:
        cols["phys"] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
        cols["logical"] = rng.integers(0, 1 << 31, size=n, dtype=np.uint32)
        cols["node"] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    if tomb:
        cols["tags"] = (rng.random(n) < 0.1).astype(np.uint8)
    lens = rng.integers(1, 40, n)
    lens[rng.random(n) < 0.15] = 0
    lens[int(rng.integers(0, n))] = 1500
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    cols["values"] = rng.integers(0, 256, int(offs[-1]), dtype=np.uint8)
    cols["value_offsets"] = offs
    return cols


def _take(cols, idx):
    """rows idx of a var batch, their values packed anew"""
    offs, heap = cols["value_offsets"].astype(np.int64), cols["values"]
    out = {c: v[idx] for c, v in cols.items() if c not in ("values", "value_offsets")}
    lens = (offs[1:] - offs[:-1])[idx]
    out["value_offsets"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    out["values"] = np.concatenate([heap[offs[i]:offs[i + 1]] for i in idx] or [np.zeros(0, np.uint8)]).astype(np.uint8)
    return out


def _order(sch, keys):
    if sch.key_kind in (1, 2):
        return np.argsort(keys.copy().view("<u4" if sch.key_row == 4 else "<u8").ravel(), kind="stable")
    return np.lexsort(keys.T[::-1])


def _sorted_unique(sch, cols):
    order = _order(sch, cols["keys"])
    k = cols["keys"][order]
    keep = np.ones(len(k), bool)
    keep[1:] = (k[1:] != k[:-1]).any(axis=1)
    return _take(cols, order[keep])


def _batch(rng, sch, live, m, tomb):
    """m rows with distinct keys: fresh keys, overwrites and deletes of live keys, deletes of absent ones"""
    cols = _gen(rng, sch, m, tomb)
    ops = np.zeros(m, np.uint8)
    pool = sorted(live)
    if pool:
        for i in range(m):
            u = rng.random()
            if u < 0.27:
                cols["keys"][i] = np.frombuffer(pool[rng.integers(len(pool))], np.uint8)
                ops[i] = u >= 0.2
            elif u < 0.3:
                ops[i] = 1
    _, first = np.unique(cols["keys"], axis=0, return_index=True)
    keep = np.sort(first)
    cols, ops = _take(cols, keep), ops[keep]
    for k, o in zip(cols["keys"], ops):
        (live.discard if o else live.add)(k.tobytes())
    return cols, ops


def _dev(cols, gpu):
    import torch
    out = {c: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for c, v in cols.items() if c != "value_offsets"}
    out["value_offsets"] = torch.from_numpy(cols["value_offsets"].view(np.int64)).to(gpu)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [4, 1, 7])
@pytest.mark.parametrize("spec", SPECS, ids=lambda s: f"{s[0]}-{s[1]}-var")
def test_var_device_route_equals_host_route_and_one_store(gpu, spec, shards):
    import torch
    from rsos_hip import GpuFingerprintStore, RecordSchema
    from rsos_hip.sharded import ShardedStore
    kind, kk, tomb = spec
    sch = getattr(RecordSchema, kind)(kk, "var")
    rng = np.random.default_rng(60 + shards)
    dmap = ShardedStore(sch, _devices(shards), var_values=True)
    hmap = ShardedStore(sch, _devices(shards), var_values=True)
    one, peer = GpuFingerprintStore(sch), GpuFingerprintStore(sch)
    maps = [dmap, one, hmap]
    for st in maps:
        st.set_compaction(6, 1024)
    live = set()

    def batch(m, stage_first=0):
        if stage_first:  # staged rows pending before a device batch are applied first
            b, ops = _batch(rng, sch, live, stage_first, tomb)
            for st in maps + [peer]:
                st.stage(b, ops)
        b, ops = _batch(rng, sch, live, m, tomb)
        db, dops = _dev(b, gpu), torch.from_numpy(ops).to(gpu)
        want = one.apply_device(db, dops)
        assert dmap.apply_device(db, dops) == want
        assert hmap.apply(b, ops) == want
        skip = rng.random(len(ops)) < 0.01  # the peer follows, a few rows short: the reconciliations stay small
        if not skip.all():
            idx = np.flatnonzero(~skip)
            peer.apply(_take(b, idx), ops[idx])
        assert dmap.sizes() == hmap.sizes() and dmap.splitters == hmap.splitters
        assert dmap.size() == len(live)
        _same(maps, rng, peer)

    batch(257)  # a never-loaded map: even splitters
    if shards > 1:
        assert sum(1 for s in dmap.sizes() if s) > 1
    n = 16 * shards * 150
    cols = _sorted_unique(sch, _gen(rng, sch, n + 40, tomb))
    cols = _take(cols, np.arange(n))
    live = set(k.tobytes() for k in cols["keys"])
    dmap.load_bulk_device(_dev(cols, gpu))
    one.load_bulk_device(_dev(cols, gpu))
    hmap.load_bulk(cols)
    peer.load_bulk(_take(cols, np.flatnonzero(rng.random(n) > 0.003)))
    assert dmap.sizes() == hmap.sizes() == [n // shards] * shards and dmap.splitters == hmap.splitters
    _same(maps, rng, peer)
    batch(1)
    batch(257, stage_first=33)
    batch(5001)
    assert dmap.stats()["compactions"] > 0
    # a load whose cuts are rounded down to multiples of 16 rows: the offsets start inside the heap
    m = n - 5
    part = _take(cols, np.arange(m))
    dmap.load_bulk_device(_dev(part, gpu))
    one.load_bulk_device(_dev(part, gpu))
    cut = [(m * s // shards) & ~15 for s in range(shards)] + [m]
    assert dmap.sizes() == [cut[s + 1] - cut[s] for s in range(shards)]
    _same([dmap, one], rng)
    for st in maps + [peer]:
        st.close()


@pytest.mark.gpu
def test_var_sharded_snapshot_reload_equals_one_store(gpu):
    from rsos_hip import GpuFingerprintStore, _abi as A
    from rsos_hip.sharded import ShardedStore
    from rsos_hip.snapshot import load_snapshot
    shape = "str31_var"
    recs = ordered(shape, gen_records(shape, 3001, 0.2, unique=True), "sorted")
    data, end, starts = write_snapshot(shape, recs)
    schd, schp, form = schemas(shape)
    sd, sp = ShardedStore(schd, _devices(4), var_values=True), ShardedStore(schp, _devices(4), var_values=True)
    od, op = GpuFingerprintStore(schd), GpuFingerprintStore(schp)
    want = load_snapshot(data, od, op, form, ragged=True)
    for src in (data, to_dev(data)):
        info = ShardedStore.load_snapshot(src, sd, sp, key_form=form, ragged=True)
        assert (info.entries, info.tombstones, info.entries_end, info.keys) == \
            (want.entries, want.tombstones, want.entries_end, want.keys) == (3001, want.tombstones, end, 3001)
        assert _dump(sd) == _dump(od) and _dump(sp) == _dump(op)
        cut = [(3001 * s // 4) & ~15 for s in range(4)] + [3001]
        assert sd.sizes() == sp.sizes() == [cut[s + 1] - cut[s] for s in range(4)]
    # entries out of key order: RH_ERR_UNSUPPORTED, both maps unchanged
    before = (_dump(sd), _dump(sp), sd.sizes(), sd.splitters)
    swapped = list(recs)
    swapped[1700], swapped[1701] = swapped[1701], swapped[1700]
    with pytest.raises(A.RsosHipError) as e:
        ShardedStore.load_snapshot(write_snapshot(shape, swapped)[0], sd, sp, key_form=form, ragged=True)
    assert e.value.code == A.ERR_UNSUPPORTED and "entry 1701" in str(e.value)
    assert (_dump(sd), _dump(sp), sd.sizes(), sd.splitters) == before
    for st in (sd, sp, od, op):
        st.close()


@pytest.mark.gpu
def test_var_errors(gpu):
    """A host batch whose offsets decrease is RH_ERR_ARG before any shard changes: the map is unchanged
    and still usable.  Without var_values the schema is refused as ever."""
    from rsos_hip import RecordSchema, _abi as A
    from rsos_hip.sharded import ShardedStore
    sch = RecordSchema.dated("str31", "var")
    with pytest.raises(A.RsosHipError) as e:
        ShardedStore(sch, _devices(4))
    assert e.value.code == A.ERR_UNSUPPORTED and "VARBYTES" in str(e.value)
    rng = np.random.default_rng(9)
    sh = ShardedStore(sch, _devices(4), var_values=True)
    cols = _sorted_unique(sch, _gen(rng, sch, 2000, True))
    sh.load_bulk(cols)
    before = (_dump(sh), sh.sizes())
    live = set()
    b, ops = _batch(rng, sch, live, 300, True)
    for what in ("decreasing", "past_the_heap"):
        bad = dict(b, value_offsets=b["value_offsets"].copy())
        if what == "decreasing":
            bad["value_offsets"][150] = bad["value_offsets"][151] + 5  # row 150 ends before it starts
        else:
            bad["value_offsets"][-1] = len(b["values"]) + 1
        for call in (lambda: sh.apply(bad, ops), lambda: sh.stage(bad, ops)):
            with pytest.raises(A.RsosHipError) as e:
                call()
            assert e.value.code == A.ERR_ARG, what
            assert (_dump(sh), sh.sizes()) == before
    got = sh.apply(b, ops)  # still usable
    assert sum(got) > 0 and sh.size() == before[0][0] + got[0] - got[2]
    # a staged delete-only batch may leave the values out, as for one store
    from rsos_hip import GpuFingerprintStore
    one = GpuFingerprintStore(sch)
    one.load_bulk(cols)
    one.apply(b, ops)
    dels = {c: np.ascontiguousarray(v[:80:2]) for c, v in cols.items() if c not in ("values", "value_offsets")}
    for st in (sh, one):
        st.stage(dels, np.ones(40, np.uint8))
    assert sh.size() == one.size() == before[0][0] + got[0] - got[2] - 40 and sh.aggregate() == one.aggregate()
    one.close()
    sh.close()
