"""Batched Enumerate on the sharded map (rh_sstore_enumerate_segments): 4 and 8 key-range shards on
device 0, u64 keys and strings in 32-byte rows, 20,000 rows.  Ranges inside one shard, ranges that
straddle one splitter, ranges that cover three shards and bounds equal to a splitter key, after a load
and after a host batch that leaves delta rows, with the shards' host tiers off and on: every output
array equals, byte for byte, what one rh_store holding the same map answers (and the host's replay,
enumerate_common.Keys).  A map broken by a failed apply refuses the call with RH_ERR_STATE."""
import bisect

import numpy as np
import pytest

import enumerate_common as E

pytestmark = pytest.mark.gpu

N = 20_000


def _schema(name):
    from rsos_hip import RecordSchema
    return RecordSchema.plain(*{"u64": ("u64", "u64"), "str31": ("str31", "u64")}[name])


def _ranges(rng, keys, spl):
    """ranges placed by the splitters `spl` (tokens): inside a shard, across one splitter, across two
    (three shards), with bounds on the splitters themselves; then short random ones and the specials"""
    s = keys.sorted()
    n = len(s)
    at = [bisect.bisect_left(s, x) for x in spl]  # each splitter's rank: the first row of the next shard
    near = lambda i, d: s[min(max(i + d, 0), n - 1)]  # noqa: E731
    out = []
    for g, i in enumerate(at):
        out += [(near(i, -9), near(i, 7)),        # straddles splitter g
                (near(i, -40), near(i, -3)),      # inside the shard below it
                (spl[g], near(i, 12)),            # starts on the splitter
                (near(i, -12), spl[g]),           # ends on it: nothing of the next shard
                (spl[g], spl[g]),                 # empty, on it
                (near(i, 5), near(i, -5))]        # inverted across it
        if g + 1 < len(at):
            out += [(near(i, -6), near(at[g + 1], 6)),  # three shards: a whole shard in the middle
                    (spl[g], spl[g + 1]),               # exactly one shard
                    (spl[g + 1], spl[g])]               # inverted, splitter to splitter
    out += [(None, spl[0]), (spl[-1], None), (None, None), (near(at[0], -3), None), (None, near(at[-1], 3))]
    return E.many_ranges(rng, keys, len(out) + 120, out + E.special_ranges(rng, keys))


def _same(sh, one, keys, ranges):
    got, want = sh.enumerate_segments(ranges), E.check(one, keys, ranges)
    for x, y, what in zip(got, want, ("first ranks", "offsets", "keys")):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what


@pytest.mark.parametrize("shards", [4, 8])
@pytest.mark.parametrize("name", ["u64", "str31"])
def test_sharded_equals_one_store(gpu, name, shards):
    from rsos_hip import GpuFingerprintStore
    from rsos_hip.sharded import ShardedStore
    sch = _schema(name)
    rng = np.random.default_rng(31)
    keys = E.Keys(sch)
    sh, one = ShardedStore(sch, [0] * shards, host_tier=False), GpuFingerprintStore(sch, host_tier=False)
    try:
        _same(sh, one, keys, [(None, None), (keys.above(0), None)])  # an empty map: all zeros
        base = sorted(keys.fresh(rng, N))
        cols = keys.columns(rng, base)
        sh.load_bulk(cols), one.load_bulk(cols)
        keys.apply(base, [0] * N)
        spl = list(sh.splitters)  # (an int, or a string's bytes: tokens)
        assert len(spl) == shards - 1 and all(sh.sizes())
        _same(sh, one, keys, _ranges(rng, keys, spl))
        # a host batch: inserts, overwrites and deletes near every splitter and elsewhere
        pick = [base[int(i)] for i in rng.choice(N, 600, replace=False)]
        edge = [base[bisect.bisect_left(base, x) + d] for x in spl for d in (-2, -1, 0, 1)]
        new = keys.fresh(rng, 900)
        gone = sorted(set(pick[300:] + edge[::2]))
        over = sorted(set(pick[:300] + edge[1::2]) - set(gone))
        toks, ops = new + over + gone, [0] * (len(new) + len(over)) + [1] * len(gone)
        batch = keys.columns(rng, toks)
        assert sh.apply(batch, np.array(ops, np.uint8)) == one.apply(batch, np.array(ops, np.uint8))
        keys.apply(toks, ops)
        assert sh.stats()["delta_rows"] > 0 and one.stats()["delta_rows"] > 0
        ranges = _ranges(rng, keys, spl)
        _same(sh, one, keys, ranges)
        assert sh.stats()["delta_rows"] > 0  # read in place
        sh.set_host_tier(True), one.set_host_tier(True)
        sh.tier_sync(), one.tier_sync()
        _same(sh, one, keys, ranges)
        _same(sh, one, keys, ranges[:40])  # few enough for every shard's host tier
        _same(sh, one, keys, [])
    finally:
        sh.close(), one.close()


def test_sharded_row_cap_and_output_buffer(gpu):
    """the cap weighs the shards' totals together; the answer is the sharded store's own buffer, which
    a later call on a shard does not touch"""
    import ctypes as C
    from rsos_hip import _abi as A
    from rsos_hip.rbsr import Segments
    from rsos_hip.sharded import ShardedStore
    sch = _schema("u64")
    rng = np.random.default_rng(3)
    keys = E.Keys(sch)
    sh = ShardedStore(sch, [0] * 4, host_tier=False)
    try:
        base = sorted(keys.fresh(rng, N))
        sh.load_bulk(keys.columns(rng, base))
        keys.apply(base, [0] * N)
        ranges = [(None, None), (base[4000], base[12000]), (base[100], base[100])]
        wf, wo, wr = keys.expect(ranges)
        total = int(wo[-1])  # every shard's part is below the cap of total - 1; their sum is not
        with pytest.raises(A.RsosHipError) as e:
            sh.enumerate_segments(ranges, max_rows=total - 1)
        assert e.value.code == A.ERR_ARG and str(total) in str(e.value) and e.value.rows == total
        assert np.array_equal(e.value.first_ranks, wf) and np.array_equal(e.value.offsets, wo)
        E.check(sh, keys, ranges, max_rows=total)
        seg = Segments.from_items(sch, ranges)
        cs, out = seg.c(), A.Enumerated()
        assert A.lib().rh_sstore_enumerate_segments(sh._h, C.byref(cs), 0, C.byref(out)) == A.OK
        view = np.ctypeslib.as_array(C.cast(out.keys, C.POINTER(C.c_uint8)), (total * 8,))
        held = view.copy()
        for shard in sh.shards:  # the shards answer other ranges meanwhile
            shard.enumerate_segments([(None, None)])
        assert np.array_equal(view, held) and np.array_equal(held.reshape(-1, 8), wr)
        assert A.lib().rh_sstore_enumerate_segments(sh._h, C.byref(cs), (1 << 22) + 1, C.byref(out)) == A.ERR_ARG
    finally:
        sh.close()


def test_broken_map_refuses_enumerate(gpu):
    from rsos_hip import _abi as A
    from rsos_hip.sharded import ShardedStore
    sch = _schema("u64")
    sh = ShardedStore(sch, [0] * 4)
    try:
        k = np.arange(4000, dtype=np.uint64)
        cols = {"keys": k.view(np.uint8).reshape(-1, 8), "values": (k * 3).view(np.uint8).reshape(-1, 8)}
        sh.load_bulk(cols)
        batch = {"keys": k[::7].copy().view(np.uint8).reshape(-1, 8), "values": (k[::7] * 5).view(np.uint8).reshape(-1, 8)}
        A.lib().rh_debug_fail_point(b"sstore.apply_last_shard")
        with pytest.raises(A.RsosHipError):
            sh.apply(batch, np.zeros(len(k[::7]), np.uint8))
        A.lib().rh_debug_fail_point(b"")
        for ranges in ([(None, None)], [(5, 900), (2000, None)], []):
            with pytest.raises(A.RsosHipError) as e:
                sh.enumerate_segments(ranges)
            assert e.value.code == A.ERR_STATE and "load to recover" in str(e.value)
        sh.load_bulk(cols)
        first, offs, rows = sh.enumerate_segments([(5, 900), (2000, None)])
        assert list(first) == [5, 2000] and list(offs) == [0, 895, 2895]
        assert np.array_equal(rows.view("<u8").ravel(), np.concatenate([k[5:900], k[2000:]]))
    finally:
        sh.close()
