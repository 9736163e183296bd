"""The sharded store's device-column write side (rh_sstore_load_device / _apply_device /
_load_snapshot, csrc/sharded_store.hip over csrc/shard_route.hip), with 4 shards and also 1 and 7.

Shard s sits on device s % device_count: on a box with one GPU that is device 0 throughout, and the
device-to-device copy a shard on another device gets is then not exercised.

Every state is compared three ways: the map fed device columns, one rh_store fed the same device
columns, and a second rh_sstore fed the same rows through the host route -- len, root, 16 key-range
aggregates, ranks of 200 keys, selects, the whole key dump, the whole fingerprint dump, and one
FixedFanOut reconciliation round by round."""
import ctypes as C
import os

import numpy as np
import pytest

from ragged_snapshot_common import gen_records, ordered, schemas, to_dev, write_snapshot
from records_common import ColumnModel, _batch, _devices, _dump, _gen, _key_rows, _same, _sorted_unique

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(cols, gpu):
    import torch
    return {c: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for c, v in cols.items()}


SPECS = [("dated", "bytes16", "bytes64", True), ("plain", "u64", "u64", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [4, 1, 7])
@pytest.mark.parametrize("spec", SPECS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_device_route_equals_host_route_and_one_store(gpu, oracle_lib, spec, shards):
    import torch
    from rsos_hip import GpuFingerprintStore, RecordSchema
    from rsos_hip.sharded import ShardedStore
    kind, kk, vk, tomb = spec
    sch = getattr(RecordSchema, kind)(kk, vk)
    rng = np.random.default_rng(40 + shards)
    dmap, hmap = ShardedStore(sch, _devices(shards)), ShardedStore(sch, _devices(shards))
    one, peer = GpuFingerprintStore(sch), GpuFingerprintStore(sch)
    maps = [dmap, one, hmap]
    for st in maps:
        st.set_compaction(6, 1024)
    model = ColumnModel(oracle_lib, sch)
    even = dmap.splitters

    def batch(m, stage_first=0):
        if stage_first:  # staged rows pending before a device batch are applied first
            b, ops = _batch(rng, sch, model, stage_first, tomb)
            for st in maps + [peer]:
                st.stage(b, ops)
            model.apply(b, ops)
        b, ops = _batch(rng, sch, model, m, tomb)
        db, dops = _dev(b, gpu), torch.from_numpy(ops).to(gpu)
        want = model.apply(b, ops)
        assert dmap.apply_device(db, dops) == want
        assert one.apply_device(db, dops) == want
        assert hmap.apply(b, ops) == want
        peer.apply(b, ops)  # the peer follows, a few rows short: the reconciliations stay small

    # a never-loaded map: even splitters, every row routed by them
    batch(257)
    assert dmap.splitters == hmap.splitters and dmap.sizes() == hmap.sizes()
    if shards > 1:
        assert sum(1 for s in dmap.sizes() if s) > 1
    _same(maps, rng)
    # a load whose equal-count cuts are multiples of 16 rows: both routes cut alike ...
    n = 16 * shards * 150
    cols = _sorted_unique(sch, _gen(rng, sch, n + 40, tomb))
    cols = {c: v[:n] for c, v in cols.items()}
    assert len(cols["keys"]) == n
    model = ColumnModel(oracle_lib, sch)
    model.apply(cols, np.zeros(n, np.uint8))
    dmap.load_bulk_device(_dev(cols, gpu))
    one.load_bulk_device(_dev(cols, gpu))
    hmap.load_bulk(cols)
    peer.load_bulk({c: v[rng.random(n) > 0.003] for c, v in cols.items()})
    assert dmap.sizes() == hmap.sizes() == [n // shards] * shards and dmap.splitters == hmap.splitters
    _same(maps, rng)
    # ... then batches of 1, 257 and 70,001 rows with inserts, overwrites and deletes, through a compaction
    batch(1)
    batch(257, stage_first=33)
    batch(70001)
    assert dmap.stats()["compactions"] > 0
    batch(257)
    assert dmap.sizes() == hmap.sizes() and dmap.splitters == hmap.splitters
    assert (_int_root(dmap), dmap.size()) == model.root()
    # apply_device_many: a plain loop over batches
    b1, o1 = _batch(rng, sch, model, 300, tomb)
    model.apply(b1, o1)
    b2, o2 = _batch(rng, sch, model, 40, tomb)
    model.apply(b2, o2)
    dbs, dos = [_dev(b1, gpu), _dev(b2, gpu)], [torch.from_numpy(o1).to(gpu), torch.from_numpy(o2).to(gpu)]
    assert dmap.apply_device_many(dbs, dos) == one.apply_device_many(dbs, dos)
    hmap.apply(b1, o1), hmap.apply(b2, o2)
    _same(maps, rng, peer)
    # a load whose cuts are not: each rounded down to a multiple of 16 rows
    m = n - 5
    dmap.load_bulk_device(_dev({c: v[:m] for c, v in cols.items()}, gpu))
    one.load_bulk_device(_dev({c: v[:m] for c, v in cols.items()}, gpu))
    cut = [(m * s // shards) & ~15 for s in range(shards)] + [m]
    assert dmap.sizes() == [cut[s + 1] - cut[s] for s in range(shards)]
    assert dmap.splitters == [one.select(c) for c in cut[1:-1]]
    _same([dmap, one], rng)
    # fewer rows than 16 per shard, and none
    for few in (9, 0):
        dmap.load_bulk_device(_dev({c: v[:few] for c, v in cols.items()}, gpu))
        one.load_bulk_device(_dev({c: v[:few] for c, v in cols.items()}, gpu))
        assert dmap.sizes() == [0] * (shards - 1) + [few]
        assert (dmap.size(), dmap.aggregate(), _key_rows(dmap).tobytes()) == (few, one.aggregate(), _key_rows(one).tobytes())
    assert dmap.splitters == even  # even again after an empty load
    for st in maps + [peer]:
        st.close()


def _int_root(st):
    return sum(int(x) << (64 * i) for i, x in enumerate(st.aggregate().fingerprint.limbs))


def _u64_cols(keys, mul):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    return {"keys": keys.view(np.uint8).reshape(-1, 8), "values": (keys * np.uint64(mul)).view(np.uint8).reshape(-1, 8)}


@pytest.mark.gpu
def test_device_batch_with_a_repeated_key(gpu):
    """The device route sees a repeated key only in its shard's sort: RH_ERR_ARG, and -- other shards
    having taken their rows -- the map refuses every call until a load.  With all rows in one shard
    nothing was committed and the map stays whole."""
    from rsos_hip import RecordSchema, _abi as A
    from rsos_hip.sharded import ShardedStore
    sch = RecordSchema.plain("u64", "u64")
    sh = ShardedStore(sch, _devices(4))
    keys = np.arange(4000, dtype=np.uint64)
    sh.load_bulk_device(_dev(_u64_cols(keys, 3), gpu))
    root = sh.aggregate()
    bad = keys[::9].copy()
    bad[7] = bad[300]  # equal keys land in one shard
    with pytest.raises(A.RsosHipError) as e:
        sh.apply_device(_dev(_u64_cols(bad, 5), gpu))
    assert e.value.code == A.ERR_ARG
    for call in (sh.size, sh.aggregate, lambda: sh.rank(5), lambda: sh.apply_device(_dev(_u64_cols(keys[:4], 7), gpu))):
        with pytest.raises(A.RsosHipError) as e:
            call()
        assert e.value.code == A.ERR_STATE and "load to recover" in str(e.value)
    sh.load_bulk_device(_dev(_u64_cols(keys, 3), gpu))
    assert sh.size() == 4000 and sh.aggregate() == root
    only = keys[10:200:3].copy()  # shard 0 alone
    only[3] = only[40]
    with pytest.raises(A.RsosHipError) as e:
        sh.apply_device(_dev(_u64_cols(only, 5), gpu))
    assert e.value.code == A.ERR_ARG
    assert sh.size() == 4000 and sh.aggregate() == root
    sh.close()


@pytest.mark.gpu
def test_device_apply_failure_is_sticky_until_a_load(gpu):
    """"sstore.apply_last_shard" under rh_sstore_apply_device, as
    test_sharded.py::test_sharded_failed_apply_is_sticky_until_a_load has it for the host route."""
    from rsos_hip import RecordSchema, _abi as A
    from rsos_hip.sharded import ShardedStore
    sch = RecordSchema.plain("u64", "u64")
    sh = ShardedStore(sch, _devices(4))
    keys = np.arange(4000, dtype=np.uint64)
    cols = _dev(_u64_cols(keys, 3), gpu)
    sh.load_bulk_device(cols)
    root = sh.aggregate()
    A.lib().rh_debug_fail_point(b"sstore.apply_last_shard")
    with pytest.raises(A.RsosHipError) as e:
        sh.apply_device(_dev(_u64_cols(keys[::7], 5), gpu))
    A.lib().rh_debug_fail_point(b"")
    assert e.value.code == A.ERR_OOM
    for call in (sh.size, sh.aggregate, lambda: sh.rank(5), lambda: sh.select(0)):
        with pytest.raises(A.RsosHipError) as e:
            call()
        assert e.value.code == A.ERR_STATE and "load to recover" in str(e.value)
    sh.load_bulk_device(cols)
    assert sh.size() == 4000 and sh.aggregate() == root and sh.shards[0].size() == 992  # (1000 & ~15)
    sh.close()


@pytest.mark.gpu
def test_bad_device_loads_leave_the_map_empty(gpu):
    """Keys out of order inside one shard, and only across a cut (every shard's own rows in order):
    RH_ERR_ARG, the map empty with even splitters."""
    from rsos_hip import RecordSchema, _abi as A
    from rsos_hip.sharded import ShardedStore
    sch = RecordSchema.plain("u64", "u64")
    sh = ShardedStore(sch, _devices(4))
    even = sh.splitters
    good = np.arange(1, 4001, dtype=np.uint64) * np.uint64(3)
    for what in ("inside", "across", "equal_across"):
        sh.load_bulk_device(_dev(_u64_cols(good, 3), gpu))
        assert sh.size() == 4000 and sh.splitters != even
        keys = good.copy()
        if what == "inside":
            keys[[1500, 1501]] = keys[[1501, 1500]]
        elif what == "across":  # rows 1999 | 2000 are the two sides of the middle cut
            keys[[1999, 2000]] = keys[[2000, 1999]]
        else:
            keys[1999] = keys[2000]
        with pytest.raises(A.RsosHipError) as e:
            sh.load_bulk_device(_dev(_u64_cols(keys, 3), gpu))
        assert e.value.code == A.ERR_ARG, what
        assert sh.size() == 0 and sh.sizes() == [0] * 4 and sh.splitters == even, what
    sh.close()


def test_device_row_cap_is_refused_on_the_arguments(rsos_hip_lib):
    """A device load or batch that must overflow a shard (2^31 rows each, at most 64 shards) is refused
    with RH_ERR_ARG before anything else is looked at, as test_abi.py::
    test_store_row_cap_is_refused_at_the_boundary has it for one store; under it, the NULL map.
    The header states the two places where the device route's contract differs from the host route's."""
    from rsos_hip import _abi as A
    L = A.lib()
    cols = A.Columns()
    assert L.rh_sstore_load_device(None, 0, C.byref(cols), (1 << 31) * 64, None) == A.ERR_ARG
    assert "2^31 rows" in L.rh_last_error().decode()
    assert L.rh_sstore_apply_device(None, 0, C.byref(cols), None, 1 << 32, None, None, None, None) == A.ERR_ARG
    assert "2^31 rows" in L.rh_last_error().decode()
    assert L.rh_sstore_load_device(None, 0, C.byref(cols), 10, None) == A.ERR_ARG
    assert "NULL" in L.rh_last_error().decode()
    assert L.rh_sstore_apply_device(None, 0, C.byref(cols), None, 10, None, None, None, None) == A.ERR_ARG
    assert "NULL" in L.rh_last_error().decode()
    assert L.rh_sstore_load_snapshot(None, None, 0, None, 0, 0, 0, None) == A.ERR_ARG
    header = " ".join(open(os.path.join(ROOT, "include", "rsos_hip.h")).read().split())
    assert "rounds every cut down to a * multiple of 16 rows" in header
    assert "A DEVICE batch (rh_sstore_apply_device) differs" in header and "the map is then broken" in header


# ---- snapshot reload ---------------------------------------------------------------------------

SNAP = [("b16_b64", False), ("str31_u64", True)]


def _snap_maps(shape, shards=4):
    from rsos_hip import GpuFingerprintStore
    from rsos_hip.sharded import ShardedStore
    sd, sp, form = schemas(shape)
    return (ShardedStore(sd, _devices(shards)), ShardedStore(sp, _devices(shards)), GpuFingerprintStore(sd),
            GpuFingerprintStore(sp), form)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ragged", SNAP, ids=[s for s, _ in SNAP])
def test_sharded_snapshot_reload_equals_one_store(gpu, shape, ragged):
    from rsos_hip import _abi as A
    from rsos_hip.sharded import ShardedStore
    from rsos_hip.snapshot import load_snapshot
    recs = ordered(shape, gen_records(shape, 3001, 0.2, unique=True), "sorted")
    data, end, starts = write_snapshot(shape, recs)
    sd, sp, od, op, form = _snap_maps(shape)
    want = load_snapshot(data, od, op, form, ragged=ragged)
    for src in (data, to_dev(data)):
        info = ShardedStore.load_snapshot(src, sd, sp, form, ragged=ragged)
        assert (info.entries, info.tombstones, info.entries_end) == (3001, want.tombstones, end)
        assert info.keys == info.entries == want.keys
        assert _dump(sd) == _dump(od) and _dump(sp) == _dump(op)
        cut = [(3001 * s // 4) & ~15 for s in range(4)] + [3001]
        assert sd.sizes() == sp.sizes() == [cut[s + 1] - cut[s] for s in range(4)]
        assert sd.splitters == sp.splitters == [od.select(c) for c in cut[1:-1]]
    # one map alone
    solo = _snap_maps(shape)[1]
    ShardedStore.load_snapshot(data, None, solo, form, ragged=ragged)
    assert _dump(solo) == _dump(op)
    solo.close()
    # entries out of key order: RH_ERR_UNSUPPORTED naming the first of them, both maps unchanged
    before = (_dump(sd), _dump(sp), sd.sizes(), sd.splitters)
    swapped = list(recs)
    swapped[1700], swapped[1701] = swapped[1701], swapped[1700]
    with pytest.raises(A.RsosHipError) as e:
        ShardedStore.load_snapshot(write_snapshot(shape, swapped)[0], sd, sp, form, ragged=ragged)
    assert e.value.code == A.ERR_UNSUPPORTED and "entry 1701" in str(e.value)
    assert (_dump(sd), _dump(sp), sd.sizes(), sd.splitters) == before
    # a truncated file: RH_ERR_DATA, both maps unchanged
    with pytest.raises(A.RsosHipError) as e:
        ShardedStore.load_snapshot(data[:starts[2000] + 5], sd, sp, form, ragged=ragged)
    assert e.value.code == A.ERR_DATA
    assert (_dump(sd), _dump(sp), sd.sizes(), sd.splitters) == before
    for st in (sd, sp, od, op):
        st.close()
