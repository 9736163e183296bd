"""Batched Enumerate (rh_store_enumerate_segments; Rsos::enumerate, rsos/src/rsos_trait.rs:73-83) on
one store, against the live key set replayed on the host (enumerate_common.Keys: no product code in the
expected answer).

Every schema (u32, u64, 16- and 32-byte keys, strings in 64-byte rows) in every state of the store
-- empty; a 70,000-row base (past one 65,536-row super-block); base + a delta run left by a 3,000-row
batch of inserts, overwrites and deletes; the same with 5 staged rows; the same compacted -- is asked
r = 1, 2, 300 and 3,000 ranges in one call (the offsets' scan crosses its 256- and 1,024-entry
tiles): unbounded, present and absent bounds, empty, inverted, identical and overlapping ranges,
ranges across base rows 256 k and 65,536, ranges over deleted base rows and run-only inserts, starts
above the last key.  Then the row cap, the round's own `enumerations` struct as input, the host tier
on and off, and the per-range route (GpuFingerprintStore.enumerate)."""
import ctypes as C

import numpy as np
import pytest

import enumerate_common as E

pytestmark = pytest.mark.gpu

STATES = ("empty", "base", "delta", "staged", "compacted")
N_BASE, N_BATCH = 70_000, 3_000


def _build(name, state, seed=11):
    """(store, Keys, base tokens, touched tokens) with the store taken to `state`"""
    from rsos_hip import GpuFingerprintStore
    sch = E.schema(name)
    rng = np.random.default_rng(seed)
    st, keys = GpuFingerprintStore(sch, host_tier=False), E.Keys(sch)
    base, touched = None, []
    if state == "empty":
        return st, keys, base, touched
    base = sorted(keys.fresh(rng, N_BASE))
    st.load_bulk(keys.columns(rng, base))
    keys.apply(base, [0] * N_BASE)
    if state == "base":
        return st, keys, base, touched
    # one batch: 1,800 new keys, 600 overwrites of base rows, 400 deletes of base rows, 200 of absent keys
    pick = [base[int(i)] for i in rng.choice(N_BASE, 1000, replace=False)]
    new, gone = keys.fresh(rng, 2000), pick[600:]
    toks = new[:1800] + pick[:600] + gone + new[1800:]
    ops = [0] * 2400 + [1] * 600
    order = rng.permutation(N_BATCH)
    toks, ops = [toks[i] for i in order], [ops[i] for i in order]
    assert st.apply(keys.columns(rng, toks), np.array(ops, np.uint8)) == (1800, 600, 400)
    keys.apply(toks, ops)
    assert st.stats()["delta_rows"] > 0  # the batch sits in the delta run: reads go over base + run
    touched = new[:4] + pick[:3] + gone[:4]
    if state in ("staged", "compacted"):
        s5 = keys.fresh(rng, 3) + [gone[5], base[17]]
        o5 = [0, 0, 0, 0, 1]  # three inserts, a deleted base row put back, a base row deleted
        st.stage(keys.columns(rng, s5), np.array(o5, np.uint8))
        keys.apply(s5, o5)
        touched += s5
    if state == "compacted":
        st.compact()
        assert st.stats()["delta_rows"] == 0
        base = keys.sorted()
    return st, keys, base, touched


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", list(E.SCHEMAS))
def test_every_state_and_range_kind(gpu, name, state):
    st, keys, base, touched = _build(name, state)
    rng = np.random.default_rng(5)
    try:
        specials = E.special_ranges(rng, keys, base, touched)
        # the staged rows are applied by the first call; the special ranges, then, one by one and in pairs
        E.check(st, keys, E.many_ranges(rng, keys, 300, specials))
        if state == "delta":
            assert st.stats()["delta_rows"] > 0  # no compaction on the way
        for sp in specials:
            E.check(st, keys, [sp])
        for a, b in zip(specials[::2], specials[1::2]):
            E.check(st, keys, [a, b])
        E.check(st, keys, E.many_ranges(rng, keys, 3000, specials))
        first, offs, rows = E.check(st, keys, [])
        assert len(first) == 0 and list(offs) == [0] and rows.shape == (0, keys.kl)
        assert st.size() == len(keys.live)
    finally:
        st.close()


def _raw_call(st, ranges, max_rows):
    """the C call itself on (start, end) token pairs: (rc, rh_enumerated, what keeps its input alive)"""
    from rsos_hip import _abi as A
    from rsos_hip.rbsr import Segments
    seg = Segments.from_items(st.schema, ranges)
    cs, out = seg.c(), A.Enumerated()
    rc = A.lib().rh_store_enumerate_segments(st._h, C.byref(cs), max_rows, C.byref(out))
    return rc, out, seg


@pytest.mark.parametrize("state", ["base", "delta"])
def test_row_cap(gpu, state):
    from rsos_hip import _abi as A
    st, keys, base, touched = _build("u64_u64", state)
    try:
        rng = np.random.default_rng(2)
        ranges = E.many_ranges(rng, keys, 40, E.special_ranges(rng, keys, base, touched))
        wf, wo, wr = keys.expect(ranges)
        total = int(wo[-1])
        assert total > 4096
        rc, out, _ = _raw_call(st, ranges, total - 1)  # one row short: refused, but sized
        assert rc == A.ERR_ARG
        msg = A.lib().rh_last_error().decode()
        assert str(total) in msg and str(total - 1) in msg
        assert not out.keys and out.n == len(ranges) and out.rows == total
        assert np.array_equal(np.ctypeslib.as_array(C.cast(out.first_ranks, C.POINTER(C.c_uint64)), (len(ranges),)), wf)
        assert np.array_equal(np.ctypeslib.as_array(C.cast(out.offsets, C.POINTER(C.c_uint64)), (len(ranges) + 1,)), wo)
        with pytest.raises(A.RsosHipError) as e:
            st.enumerate_segments(ranges, max_rows=total - 1)
        assert e.value.code == A.ERR_ARG and e.value.rows == total and np.array_equal(e.value.offsets, wo)
        E.check(st, keys, ranges, max_rows=total)  # the exact total
        rc, out, _ = _raw_call(st, ranges, (1 << 22) + 1)
        assert rc == A.ERR_ARG and "2^22" in A.lib().rh_last_error().decode()
        assert not out.first_ranks and not out.offsets and not out.keys and out.n == 0 and out.rows == 0
        rc, out, _ = _raw_call(st, ranges, 1 << 22)
        assert rc == A.OK and out.rows == total
    finally:
        st.close()


def test_bad_bounds_are_refused(gpu):
    from rsos_hip import _abi as A
    st, keys, _, _ = _build("u64_u64", "base")
    try:
        kinds, two, key = np.ones(1, np.uint8), np.full(1, 2, np.uint8), np.zeros(8, np.uint8)
        out = A.Enumerated()
        for seg in (A.Segments(two.ctypes.data, key.ctypes.data, kinds.ctypes.data, key.ctypes.data, None, 1, 1),
                    A.Segments(kinds.ctypes.data, key.ctypes.data, two.ctypes.data, key.ctypes.data, None, 1, 1),
                    A.Segments(kinds.ctypes.data, None, kinds.ctypes.data, key.ctypes.data, None, 1, 1),
                    A.Segments(kinds.ctypes.data, key.ctypes.data, kinds.ctypes.data, None, None, 1, 1)):
            assert A.lib().rh_store_enumerate_segments(st._h, C.byref(seg), 0, C.byref(out)) == A.ERR_ARG
    finally:
        st.close()


@pytest.mark.parametrize("name", ["u64_u64", "str63_u64"])
@pytest.mark.parametrize("tier", [False, True])
def test_a_rounds_enumerations_struct_is_the_input(gpu, name, tier):
    """`ranges` = the `enumerations` rh_store_protocol_round returned, in place: the same answer as a
    copy of it gives, and the round's children untouched by the call"""
    from rsos_hip import GpuFingerprintStore
    from rsos_hip import rbsr as R
    sch = E.schema(name)
    rng = np.random.default_rng(21)
    ka, kb = E.Keys(sch), E.Keys(sch)
    common = sorted(ka.fresh(rng, 6000))
    only_a, only_b = ka.fresh(rng, 12, common), ka.fresh(rng, 9, common)
    a, b = GpuFingerprintStore(sch, host_tier=tier), GpuFingerprintStore(sch, host_tier=tier)
    try:
        for st, k, toks in ((a, ka, sorted(common + only_a)), (b, kb, sorted(common + only_b))):
            st.load_bulk(k.columns(rng, toks))
            k.apply(toks, [0] * len(toks))
        active, sides, asked = R.initial_segments(a), [(b, kb), (a, ka)], 0
        for k in range(40):
            st, keys = sides[k % 2]
            ch, en, _ = R.protocol_round_segments(st, R.FixedFanOut(16), active, raw=True)
            if len(en):
                kl = sch.key_row
                before = R._wrap(ch.cs, kl, True, True)
                copy = R._wrap(en.cs, kl, True, False)
                ranges = [copy.bounds(sch, i) for i in range(copy.n)]
                got = st.enumerate_segments(en)  # the round's own struct
                again = st.enumerate_segments(copy)
                for x, y, w in zip(got, again, keys.expect(ranges)):
                    assert np.array_equal(x, y) and np.array_equal(x, w)
                after = R._wrap(ch.cs, kl, False, True)
                for f in ("start_kinds", "start_keys", "end_kinds", "end_keys", "aggregates"):
                    assert getattr(before, f).tobytes() == getattr(after, f).tobytes(), f
                asked += len(en)
            if not len(ch):
                break
            active = R._wrap(ch.cs, sch.key_row, True, True)
        assert asked >= 15  # most differences ended in an IDLIST
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("name", list(E.SCHEMAS))
def test_host_tier_on_and_off(gpu, name):
    """the same answers from a fresh host tier (r <= round_max: no device round trip), from the device
    beside it (r above round_max) and with the tier off again"""
    st, keys, base, touched = _build(name, "delta")
    rng = np.random.default_rng(9)
    try:
        specials = E.special_ranges(rng, keys, base, touched)
        small, large = E.many_ranges(rng, keys, 100, specials), E.many_ranges(rng, keys, 300, specials)
        off = [st.enumerate_segments(r) for r in (small, large)]
        st.set_host_tier(True)
        st.tier_sync()
        on = [E.check(st, keys, r) for r in (small, large)]
        for sp in specials:
            E.check(st, keys, [sp])
        st.set_host_tier(False)
        again = [E.check(st, keys, r) for r in (small, large)]
        for x, y, z in zip(off, on, again):
            for i in range(3):
                assert np.array_equal(x[i], y[i]) and np.array_equal(x[i], z[i])
    finally:
        st.close()


@pytest.mark.parametrize("name", ["u32_u32", "b32_b64", "str63_u64"])
def test_equals_the_per_range_route(gpu, name):
    from rsos_hip.store import KeyRange
    st, keys, base, touched = _build(name, "delta")
    rng = np.random.default_rng(13)
    try:
        ranges = E.many_ranges(rng, keys, 20, E.special_ranges(rng, keys, base, touched)[1:14])
        first, offs, rows = E.check(st, keys, ranges)
        for j, (a, b) in enumerate(ranges):
            per = list(st.enumerate(KeyRange(a, b)))
            want = [st._key_out(rows[t].tobytes()) for t in range(int(offs[j]), int(offs[j + 1]))]
            assert [k for k, _ in per] == want
            assert [r for _, r in per] == list(range(int(first[j]), int(first[j]) + len(want)))
    finally:
        st.close()
