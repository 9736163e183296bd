"""The one-launch enumerate (csrc/enum_tiny.hpp k_enum_tiny) behind rh_store_enumerate_segments: at most
16 ranges over rows of at most 32 bytes, at most 512 rows in all.  Two stores hold the same contents,
one created with RSOS_HIP_ENUM_FUSED=1 and one with 0 (the general path always); every answer must be
the same bytes from both, and equal the live key set replayed on the host (enumerate_common.Keys).
rh_store_enumerate_stats tells which path answered."""
import bisect
import ctypes as C

import numpy as np
import pytest

import enumerate_common as E

pytestmark = pytest.mark.gpu

NAMES = ("u32_u32", "u64_u64", "b16_u64", "b32_b64", "str31_u64")
N_BASE, N_BATCH = 5_000, 300


def _schema(name):
    from rsos_hip import RecordSchema
    return RecordSchema.plain("str31", "u64") if name == "str31_u64" else E.schema(name)


def _pair(monkeypatch, name, state, seed=3, n_base=N_BASE):
    """(fused store, general store, Keys, base tokens, touched tokens): the same loads and batches into
    both; state "base" or "delta" (a 300-row batch of inserts, overwrites and deletes left in the run)"""
    from rsos_hip import GpuFingerprintStore
    sch = _schema(name)
    stores = []
    for flag in ("1", "0"):
        monkeypatch.setenv("RSOS_HIP_ENUM_FUSED", flag)
        stores.append(GpuFingerprintStore(sch, host_tier=False))
    monkeypatch.delenv("RSOS_HIP_ENUM_FUSED")
    rng = np.random.default_rng(seed)
    keys = E.Keys(sch)
    base = sorted(keys.fresh(rng, n_base))
    cols = keys.columns(rng, base)
    for st in stores:
        st.load_bulk(cols)
    keys.apply(base, [0] * n_base)
    touched = []
    if state == "delta":
        pick = [base[int(i)] for i in rng.choice(n_base, 100, replace=False)]
        new, gone = keys.fresh(rng, 200), pick[60:]
        toks = new[:180] + pick[:60] + gone + new[180:]  # 180 inserts, 60 overwrites, 40 deletes, 20 of absent keys
        ops = [0] * 240 + [1] * 60
        order = rng.permutation(N_BATCH)
        toks, ops = [toks[i] for i in order], [ops[i] for i in order]
        cols = keys.columns(rng, toks)
        for st in stores:
            assert st.apply(cols, np.array(ops, np.uint8)) == (180, 60, 40)
            assert st.stats()["delta_rows"] > 0
        keys.apply(toks, ops)
        touched = new[:6] + pick[:4] + gone[:6]
    return stores[0], stores[1], keys, base, touched


def _both(fused, general, keys, ranges, one_launch, **kw):
    """the same bytes from both stores and from the host's replay; `one_launch`: the fused store must
    have answered with k_enum_tiny (True) or on the general path (False)"""
    before = fused.enumerate_stats()
    got = E.check(fused, keys, ranges, **kw)
    after = fused.enumerate_stats()
    want = general.enumerate_segments(ranges, **kw)
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes() and x.shape == y.shape
    assert (after["one_launch"] - before["one_launch"], after["general"] - before["general"]) == \
        ((1, 0) if one_launch else (0, 1)), (len(ranges), int(got[1][-1]))
    assert general.enumerate_stats()["one_launch"] == 0
    return got


def _consecutive(s, p, r, total):
    """r ranges over consecutive rows of s from rank p, total rows in all (the first ones one longer)"""
    out, q = [], p
    for i in range(r):
        c = total // r + (i < total % r)
        out.append((s[q], s[q + c]))
        q += c
    return out


@pytest.mark.parametrize("state", ["base", "delta"])
@pytest.mark.parametrize("name", NAMES)
def test_range_counts_and_totals(gpu, monkeypatch, name, state):
    """r = 1, 2, 16 (one launch) and 17 (the general path); totals of 0, 1, 511, 512 (one launch) and 513
    rows (a fall-back that still answers), over rows near the batch's keys."""
    fused, general, keys, base, touched = _pair(monkeypatch, name, state)
    try:
        s = keys.sorted()
        p = max(min(bisect.bisect_left(s, touched[0]) - 5, len(s) - 600), 0) if touched else 1000
        for r in (1, 2, 16, 17):
            for total in (0, 1, 511, 512, 513):
                _both(fused, general, keys, _consecutive(s, p, r, total), r <= 16 and total <= 512)
        if state == "delta":
            assert fused.stats()["delta_rows"] > 0 and general.stats()["delta_rows"] > 0  # no compaction on the way
    finally:
        fused.close(), general.close()


@pytest.mark.parametrize("state", ["base", "delta"])
@pytest.mark.parametrize("name", ["u64_u64", "b16_u64", "str31_u64"])
def test_range_kinds(gpu, monkeypatch, name, state):
    """Empty, inverted, repeated and overlapping ranges, absent bounds, one side unbounded, starts above
    the last key, and -- over the run -- ranges with run entries inside them, at their edges (a bound
    that is an inserted, an overwritten or a deleted key) and deleting their rows: alone, in pairs and 16
    at a time."""
    fused, general, keys, base, touched = _pair(monkeypatch, name, state)
    rng = np.random.default_rng(7)
    try:
        s = keys.sorted()
        specials = [sp for sp in E.special_ranges(rng, keys, base, touched) if sp != (None, None)]
        for t in touched:  # a touched key as the start, as the end, and just inside
            i = bisect.bisect_left(s, t)
            specials += [(t, s[min(i + 9, len(s) - 1)]), (s[max(i - 9, 0)], t), (s[max(i - 1, 0)], s[min(i + 2, len(s) - 1)])]
        small = lambda rs: int(keys.expect(rs)[1][-1]) <= 512  # noqa: E731
        for sp in specials:
            _both(fused, general, keys, [sp], small([sp]))
        for a, b in zip(specials[::2], specials[1::2]):
            _both(fused, general, keys, [a, b], small([a, b]))
        seen = set()
        for k in range(0, len(specials), 16):
            rs = specials[k:k + 16]
            seen.add(small(rs))
            _both(fused, general, keys, rs, small(rs))
        assert True in seen
        _both(fused, general, keys, [(None, None)], False)  # both sides unbounded over 5,000 rows: the general path
    finally:
        fused.close(), general.close()


@pytest.mark.parametrize("name", ["u32_u32", "b32_b64"])
def test_small_store_both_sides_unbounded(gpu, monkeypatch, name):
    """A store of 300 rows: (.., ..) is one launch; twice in one call is 600 rows, the general path."""
    fused, general, keys, _, _ = _pair(monkeypatch, name, "base", n_base=300)
    try:
        s = keys.sorted()
        _both(fused, general, keys, [(None, None)], True)
        _both(fused, general, keys, [(None, s[40]), (s[250], None), (None, None)], True)
        _both(fused, general, keys, [(None, None), (None, None)], False)
    finally:
        fused.close(), general.close()


def test_empty_store_and_wide_rows(gpu, monkeypatch):
    """An empty store answers all zeros with no launch; a store of 64-byte rows takes the general path."""
    from rsos_hip import GpuFingerprintStore
    monkeypatch.setenv("RSOS_HIP_ENUM_FUSED", "1")
    sch = E.schema("u64_u64")
    st, keys = GpuFingerprintStore(sch, host_tier=False), E.Keys(sch)
    wide, wkeys = GpuFingerprintStore(E.schema("str63_u64"), host_tier=False), E.Keys(E.schema("str63_u64"))
    try:
        first, offs, rows = E.check(st, keys, [(None, None), (5, 9), (9, 5)])
        assert not first.any() and not offs.any() and rows.shape == (0, 8)
        assert st.enumerate_stats() == {"one_launch": 0, "general": 0}
        rng = np.random.default_rng(1)
        toks = sorted(wkeys.fresh(rng, 400))
        wide.load_bulk(wkeys.columns(rng, toks))
        wkeys.apply(toks, [0] * 400)
        E.check(wide, wkeys, [(toks[3], toks[30]), (None, toks[2])])
        assert wide.enumerate_stats() == {"one_launch": 0, "general": 1}
    finally:
        st.close(), wide.close()


def _raw_call(st, ranges, max_rows):
    from rsos_hip import _abi as A
    from rsos_hip.rbsr import Segments
    seg = Segments.from_items(st.schema, ranges)
    cs, out = seg.c(), A.Enumerated()
    rc = A.lib().rh_store_enumerate_segments(st._h, C.byref(cs), max_rows, C.byref(out))
    return rc, out, seg


@pytest.mark.parametrize("state", ["base", "delta"])
def test_row_cap(gpu, monkeypatch, state):
    """max_rows below the total: RH_ERR_ARG naming both, offsets and first ranks filled, keys NULL --
    from the one launch (whatever the total: it always writes the offsets) as from the general path; the
    exact total answers, by one launch within 512 rows and by the general path above."""
    from rsos_hip import _abi as A
    fused, general, keys, base, touched = _pair(monkeypatch, "b16_u64", state)
    try:
        s = keys.sorted()
        for total, one_launch in ((100, True), (600, False)):
            ranges = _consecutive(s, 700, 7, total)
            wf, wo, _ = keys.expect(ranges)
            for st in (fused, general):
                before = st.enumerate_stats()
                rc, out, _ = _raw_call(st, ranges, total - 1)
                assert rc == A.ERR_ARG
                msg = A.lib().rh_last_error().decode()
                assert str(total) in msg and str(total - 1) in msg
                assert not out.keys and out.n == len(ranges) and out.rows == total
                assert np.array_equal(np.ctypeslib.as_array(C.cast(out.first_ranks, C.POINTER(C.c_uint64)), (len(ranges),)), wf)
                assert np.array_equal(np.ctypeslib.as_array(C.cast(out.offsets, C.POINTER(C.c_uint64)), (len(ranges) + 1,)), wo)
                after = st.enumerate_stats()
                # (the one launch always writes the offsets and the total: it alone refuses, whatever the total)
                assert (after["one_launch"] - before["one_launch"], after["general"] - before["general"]) == \
                    ((1, 0) if st is fused else (0, 1))
            _both(fused, general, keys, ranges, one_launch, max_rows=total)
    finally:
        fused.close(), general.close()


def test_a_threshold_rounds_enumerations_struct_is_the_input(gpu, monkeypatch):
    """`ranges` = the `enumerations` of the preceding EnumerateBelowThreshold round, in place: one launch,
    the same answer as a copy of it gives, and the round's children untouched by the call."""
    from rsos_hip import GpuFingerprintStore
    from rsos_hip import rbsr as R
    monkeypatch.setenv("RSOS_HIP_ENUM_FUSED", "1")
    sch = E.schema("u64_u64")
    rng = np.random.default_rng(21)
    ka, kb = E.Keys(sch), E.Keys(sch)
    common = sorted(ka.fresh(rng, 6000))
    only_a, only_b = ka.fresh(rng, 5, common), ka.fresh(rng, 4, common)  # at most 9 IDLIST ranges a round
    a, b = GpuFingerprintStore(sch, host_tier=False), GpuFingerprintStore(sch, host_tier=False)

    def cols(k, toks):  # a record's value is a function of its key: the two stores differ in the 9 keys alone
        vals = np.array(toks, np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
        return {"keys": k.rows(toks), "values": vals.view(np.uint8).reshape(len(toks), 8)}
    try:
        for st, k, toks in ((a, ka, sorted(common + only_a)), (b, kb, sorted(common + only_b))):
            st.load_bulk(cols(k, toks))
            k.apply(toks, [0] * len(toks))
        active, sides, asked = R.initial_segments(a), [(b, kb), (a, ka)], 0
        for k in range(40):
            st, keys = sides[k % 2]
            ch, en, _ = R.protocol_round_segments(st, R.EnumerateBelowThreshold(32, 16), active, raw=True)
            if len(en):
                kl = sch.key_row
                before = R._wrap(ch.cs, kl, True, True)
                copy = R._wrap(en.cs, kl, True, False)
                ranges = [copy.bounds(sch, i) for i in range(copy.n)]
                assert len(ranges) <= 16 and int(keys.expect(ranges)[1][-1]) <= 512
                n0 = st.enumerate_stats()
                got = st.enumerate_segments(en)  # the round's own struct
                again = st.enumerate_segments(copy)
                assert st.enumerate_stats() == {"one_launch": n0["one_launch"] + 2, "general": n0["general"]}
                for x, y, w in zip(got, again, keys.expect(ranges)):
                    assert np.array_equal(x, y) and np.array_equal(x, w)
                after = R._wrap(ch.cs, kl, False, True)
                for f in ("start_kinds", "start_keys", "end_kinds", "end_keys", "aggregates"):
                    assert getattr(before, f).tobytes() == getattr(after, f).tobytes(), f
                asked += len(en)
            if not len(ch):
                break
            active = R._wrap(ch.cs, sch.key_row, True, True)
        assert asked >= 5  # a's 5 keys alone end in IDLISTs (a range may hold two of them: 3 at the least, on both sides)
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("state", ["base", "delta"])
def test_stale_sequence_word(gpu, monkeypatch, state):
    """With "enum.stale_seq" armed the sequence word already holds the number the next launch will
    store, as a reused buffer may: the answer is still the right one (the host disarms the word)."""
    from rsos_hip import _abi as A
    fused, general, keys, base, touched = _pair(monkeypatch, "u64_u64", state)
    try:
        s = keys.sorted()
        _both(fused, general, keys, _consecutive(s, 100, 3, 40), True)
        for p in (900, 2000):  # different answers of the same shape: a stale one would show
            assert A.lib().rh_debug_fail_point(b"enum.stale_seq") == A.OK
            _both(fused, general, keys, _consecutive(s, p, 3, 40), True)
        A.lib().rh_debug_fail_point(None)
    finally:
        fused.close(), general.close()


def test_sharded_map_takes_the_path_per_shard(gpu, monkeypatch):
    """A map of 4 shards on device 0 gets the one launch through its shards' own enumerate calls (a range
    inside a shard, and 370 rows in ranges that straddle splitters): one store's bytes, and the shards' counters
    summed by ShardedStore.enumerate_stats."""
    from rsos_hip import GpuFingerprintStore
    from rsos_hip.sharded import ShardedStore
    monkeypatch.setenv("RSOS_HIP_ENUM_FUSED", "1")
    sch = E.schema("u64_u64")
    rng = np.random.default_rng(4)
    keys = E.Keys(sch)
    toks = sorted(keys.fresh(rng, 400))
    cols = keys.columns(rng, toks)
    one, four = GpuFingerprintStore(sch, host_tier=False), ShardedStore(sch, [0] * 4, host_tier=False)
    try:
        one.load_bulk(cols), four.load_bulk(cols)
        keys.apply(toks, [0] * 400)
        assert all(four.sizes())
        for ranges in ([(toks[3], toks[20])], [(None, toks[150]), (toks[90], toks[310]), (toks[5], toks[5])]):
            got = E.check(four, keys, ranges)
            for x, y in zip(got, one.enumerate_segments(ranges)):
                assert x.tobytes() == y.tobytes()
        stats = four.enumerate_stats()
        assert stats["one_launch"] >= 2 and stats["general"] == 0
        assert one.enumerate_stats() == {"one_launch": 2, "general": 0}
    finally:
        one.close(), four.close()
