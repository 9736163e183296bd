"""Fixed-width values under string keys in the column store: (RH_KEY_STR, 16 | 32 | 64) x
(RH_VAL_UNIT | RH_VAL_U32 | RH_VAL_U64) -- FingerprintTreeMap<String, u32> and <&str, u32>
(rsos/src/fingerprint_tree_map/tests/basic.rs:205,226), ReplicatedSet<String> = ReplicatedMap<String, ()>
(src/replicated_set.rs:56), String -> u64 counters.

Expected fingerprints come from the oracle alone: every record's canonical bytes are built by
tests/records_common.py with oracle/pyref.py's typed model and hashed by the C oracle
(oracle.lift_encoded) -- never by the product's encoder or a second GPU kernel.
"""
import bisect
import ctypes as C
import functools

import numpy as np
import pytest

import records_common as RC
from recon_common import _outcome, reconcile
from records_common import BOUND_KINDS, KINDS, DictModel, agg_int, fold, host_cols, to_device, value_column

WIDTHS = (16, 32, 64)
VALUES = ("unit", "u32", "u64")
VBYTES = {vk: RC.val_width(vk) for vk in VALUES}
STR = "str63"  # for canonical() and msg_len(): they take the string, whatever row it travels in
N_LIFT = 600  # two whole 256-row blocks + an 88-row tail
SHAPES = [("plain", False), ("dated", True), ("dated", False), ("projection", True), ("projection", False)]
SHAPE_IDS = ["plain", "dated-tags", "dated-untagged", "projection-tags", "projection-untagged"]


def schema_of(w, vk, kind):
    from rsos_hip import RecordSchema
    return getattr(RecordSchema, kind)(f"str{w - 1}", vk)


def msg_len(kind, vk, klen, tomb=False):
    return RC.msg_len(STR, vk, kind, klen, tomb=tomb)


# ---- the lift's inputs ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lift_case(w, vk, kind, tags=True):
    """600 records of one shape (records_common.build_lift_case).  Row i's key has i % w random
    bytes.  With tags every 5th row is a tombstone: gcd(w, 5) = 1, so every key length occurs both
    present and as a tombstone within 5 w <= 320 rows.  Values are seeded-random with 0, 2^32 - 1
    and 2^64 - 1 (masked to the value's width) among the first rows."""
    return RC.build_lift_case(f"str{w - 1}", vk, kind, tags, N_LIFT,
                              7000 * w + 100 * VBYTES[vk] + sum(kind.encode()) + int(tags),
                              edge_vals=((0, 0), (1, (1 << 32) - 1), (2, (1 << 64) - 1), (5, 0), (6, (1 << 64) - 1)))


@functools.lru_cache(maxsize=None)
def lift_want(w, vk, kind, tags=True):
    import oracle as O
    return O.lift_encoded(lift_case(w, vk, kind, tags)["blobs"], threads=4)


# ---- CPU ------------------------------------------------------------------------------------------

def test_schema_helpers(rsos_hip_lib):
    """supported() and record_len() for all 27 (W, value, kind) combinations: the lengths are those
    of the empty key.  A byte-array value under a string key stays refused."""
    from rsos_hip import RecordSchema, _abi as A
    seen = 0
    for w in WIDTHS:
        for vk in VALUES:
            for kind in KINDS:
                s = schema_of(w, vk, kind)
                assert (s.key_kind, s.key_len, s.key_row, s.value_row) == (A.KEY_STR, w, w, VBYTES[vk])
                assert s.is_str and not s.is_var
                assert s.supported(), (w, vk, kind)
                assert s.record_len() == msg_len(kind, vk, 0)
                assert s.record_len(True) == msg_len(kind, vk, 0, tomb=kind != "plain")
                seen += 1
    assert seen == 27
    assert RecordSchema.dated("str15", "u64").record_len() == 40
    assert RecordSchema.dated("str15", "u64").record_len(True) == 32
    assert RecordSchema.projection("str31", "u32").record_len() == 16
    assert RecordSchema.projection("str31", "u32").record_len(True) == 12
    assert RecordSchema.plain("str63", "unit").record_len() == 8
    lib = A.lib()
    other = A.Schema(A.KEY_STR, 32, A.VAL_BYTES, 64, A.REC_DATED, 0)
    assert lib.rh_schema_supported(C.byref(other)) == 0
    assert not RecordSchema.dated("str31", "bytes64").supported()
    assert RecordSchema.dated("str31", "var").supported()  # as before
    bad = A.Schema(A.KEY_STR, 24, A.VAL_U64, 8, A.REC_PLAIN, 0)
    assert lib.rh_schema_supported(C.byref(bad)) == A.ERR_ARG and b"RH_KEY_STR" in lib.rh_last_error()


def test_encode_row(rsos_hip_lib):
    from rsos_hip import Entry, RecordSchema
    from rsos_hip.fmap import encode_row
    assert encode_row(RecordSchema.plain("str15", "u32"), 7) == ((7).to_bytes(4, "little"), 0, 0, 0, 0)
    assert encode_row(RecordSchema.plain("str31", "u64"), (1 << 64) - 1) == (b"\xff" * 8, 0, 0, 0, 0)
    assert encode_row(RecordSchema.dated("str63", "u64"), Entry(5, 1, 2, 3)) == ((5).to_bytes(8, "little"), 1, 2, 3, 0)
    assert encode_row(RecordSchema.dated("str15", "u32"), Entry(0, 1, 2, 3, tombstone=True)) == (bytes(4), 1, 2, 3, 1)
    assert encode_row(RecordSchema.projection("str31", "u32"), Entry(9)) == ((9).to_bytes(4, "little"), 0, 0, 0, 0)
    for unit in (b"", None, ()):
        assert encode_row(RecordSchema.plain("str63", "unit"), unit) == (b"", 0, 0, 0, 0)
    assert encode_row(RecordSchema.dated("str15", "unit"), Entry(b"", 4, 5, 6)) == (b"", 4, 5, 6, 0)
    assert encode_row(RecordSchema.dated("str15", "unit"), Entry(None, 4, 5, 6, tombstone=True)) == (b"", 4, 5, 6, 1)
    with pytest.raises(ValueError):
        encode_row(RecordSchema.plain("str15", "unit"), 3)  # an integer needs a u32 / u64 column
    with pytest.raises(ValueError):
        encode_row(RecordSchema.plain("str15", "u32"), b"12345")
    with pytest.raises(OverflowError):
        encode_row(RecordSchema.plain("str15", "u32"), 1 << 32)
    with pytest.raises(ValueError):
        encode_row(RecordSchema.plain("str15", "u32"), Entry(1, tombstone=True))  # a plain map has no state


@pytest.mark.parametrize("w", WIDTHS)
def test_generated_inputs_cover_the_cases(rsos_hip_lib, w):
    """The lift test's inputs themselves (a condition on the generator, no GPU)."""
    for vk in VALUES:
        for kind, tags in SHAPES:
            c = lift_case(w, vk, kind, tags)
            n = c["n"]
            assert n == 600 == 2 * 256 + 88
            L = [len(s) for s in c["strs"]]
            present = [i for i in range(n) if not c["tomb"][i]]
            assert {L[i] for i in present} == set(range(w))
            assert all(len(c["blobs"][i]) == msg_len(kind, vk, L[i], bool(c["tomb"][i])) for i in range(n))
            mask = (1 << (8 * VBYTES[vk])) - 1
            assert {0, ((1 << 32) - 1) & mask, mask} <= {c["vals"][i] for i in present}
            if c["tags"] is not None:
                tombs = [i for i in range(n) if c["tomb"][i]]
                assert tombs == list(range(4, n, 5)) and {L[i] for i in tombs} == set(range(w))
                if vk != "unit":
                    assert all(c["values"][i].any() for i in tombs)  # nonzero value rows, ignored
            else:
                assert not c["tomb"].any()
            lens = {len(b) for b in c["blobs"]}
            assert max(lens) == msg_len(kind, vk, w - 1) <= 103
            assert (max(lens) > 64) == (w == 64 or (w == 32 and kind == "dated" and vk != "unit"))
    # the messages of exactly 64 and 65 bytes the block edge is tested with
    for (ww, vk, kind, tomb), ls in {(32, "u64", "dated", False): (24, 25), (64, "u64", "dated", True): (32, 33),
                                     (64, "u64", "projection", False): (44, 45), (64, "u32", "plain", False): (52, 53)}.items():
        assert [msg_len(kind, vk, l, tomb) for l in ls] == [64, 65]
        if ww == w:
            c = lift_case(w, vk, kind, kind != "plain")
            for l in ls:
                assert any(len(c["strs"][i]) == l and bool(c["tomb"][i]) == tomb for i in range(c["n"]))


# ---- GPU: the lift ---------------------------------------------------------------------------------

def check_lift(gpu, schema, case, want, n):
    RC.check_lift(schema, to_device(host_cols(case, schema, n), gpu), case, want, n,
                  tell=("key lengths", "message lengths", "tombstones"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,tags", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("vk", VALUES)
@pytest.mark.parametrize("w", WIDTHS)
def test_lift_parity(gpu, oracle_lib, w, vk, kind, tags):
    """Every row's fingerprint and every 256-row block sum equal the oracle's, for 600 rows and for
    the first 1, 255, 256 and 257 of them."""
    case, want, schema = lift_case(w, vk, kind, tags), lift_want(w, vk, kind, tags), schema_of(w, vk, kind)
    for n in (600, 1, 255, 256, 257):
        check_lift(gpu, schema, case, want, n)


@pytest.mark.gpu
@pytest.mark.parametrize("vk", VALUES)
@pytest.mark.parametrize("w", WIDTHS)
def test_dual_lift_equals_both_single_oracles(gpu, oracle_lib, w, vk):
    import oracle as O
    from rsos_hip import lift_dual
    case = lift_case(w, vk, "dated")
    fd, bd, fp, bp = lift_dual(schema_of(w, vk, "dated"), to_device(host_cols(case, schema_of(w, vk, "dated")), gpu))
    want_d = lift_want(w, vk, "dated")
    want_p = O.lift_encoded([RC.canonical(STR, vk, "projection", case["strs"][i], case["vals"][i], tomb=bool(case["tomb"][i]))
                             for i in range(case["n"])], threads=4)
    assert np.array_equal(fd.cpu().numpy(), want_d) and np.array_equal(fp.cpu().numpy(), want_p)
    for got, want in ((bd, want_d), (bp, want_p)):
        got = got.cpu().numpy()
        assert [int.from_bytes(got[g].tobytes(), "little") for g in range(3)] == [fold(want[256 * g:256 * g + 256]) for g in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_malformed_device_rows_are_clipped_and_masked(gpu, oracle_lib, w):
    """Device key rows with 0xA5 in their padding, and rows whose length byte is 200 (caller
    errors): the fingerprints are those of the masked key -- the row's bytes below the length, the
    length clipped to w - 1 -- as the header states."""
    import oracle as O
    rng = np.random.default_rng(w)
    for vk, kind in (("u64", "dated"), ("u32", "projection"), ("unit", "plain")):
        case, want = lift_case(w, vk, kind), lift_want(w, vk, kind).copy()
        keys = case["keys"].copy()
        clipped, blobs = [i for i in range(case["n"]) if i % 7 == 3], []
        for i, s in enumerate(case["strs"]):
            keys[i, len(s):w - 1] = 0xA5
            if i % 7 == 3:
                keys[i, :w - 1] = rng.integers(0, 256, w - 1, dtype=np.uint8)
                keys[i, w - 1] = 200
                blobs.append(RC.canonical(STR, vk, kind, keys[i, :w - 1].tobytes(), case["vals"][i],
                                       (int(case["phys"][i]), int(case["logical"][i]), int(case["node"][i])),
                                       bool(case["tomb"][i])))
        assert kind == "plain" or any(case["tomb"][i] for i in clipped)
        want[clipped] = O.lift_encoded(blobs, threads=4)
        schema = schema_of(w, vk, kind)
        from rsos_hip import lift_records
        fps, _ = lift_records(schema, to_device(host_cols(case, schema, keys=keys), gpu))
        assert np.array_equal(fps.cpu().numpy(), want), (vk, kind)


@pytest.mark.gpu
def test_lift_host_parity(gpu, oracle_lib):
    """rh_lift_host on the 600-row cases; a bad host key row is RH_ERR_ARG naming the row."""
    from rsos_hip import _abi as A
    for w, vk, kind in ((16, "u64", "dated"), (32, "u32", "projection"), (64, "unit", "plain"), (64, "u64", "dated")):
        case, schema = lift_case(w, vk, kind), schema_of(w, vk, kind)
        h = host_cols(case, schema)
        cols = A.Columns(*[None if h.get(k) is None else h[k].ctypes.data for k in
                           ("keys", "phys", "logical", "node", "tags", "values")])
        sc, out = schema.c(), np.zeros((case["n"], 32), np.uint8)
        A.check(A.lib().rh_lift_host(0, C.byref(sc), C.byref(cols), case["n"], out.ctypes.data), "rh_lift_host")
        assert np.array_equal(out, lift_want(w, vk, kind))
        h["keys"][17, w - 1] = w
        assert A.lib().rh_lift_host(0, C.byref(sc), C.byref(cols), case["n"], out.ctypes.data) == A.ERR_ARG
        assert b"RH_KEY_STR" in A.lib().rh_last_error() and b"row 17 " in A.lib().rh_last_error()


# ---- GPU: the row / string trap --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("vk", ["u64", "unit"])
def test_string_store_hashes_the_string_not_the_row(gpu, oracle_lib, vk):
    """A (str15, v) store and a (bytes16, v) store loaded with the same 300 rows: to every kernel
    built for b16 rows the two look alike.  The STR store's root is the oracle's fold over the
    *strings*, and differs from the BYTES store's -- also after a 5-row batch, which a b16 store
    sends down the small-batch path."""
    import oracle as O
    from rsos_hip import GpuFingerprintStore, RecordSchema, pack_str_keys
    rng = np.random.default_rng(300)
    strs = sorted({rng.integers(0, 256, int(rng.integers(0, 16)), dtype=np.uint8).tobytes() for _ in range(400)})[:305]
    vals = [int(x) for x in rng.integers(0, 1 << 63, len(strs), dtype=np.uint64)]
    rows = pack_str_keys(strs, 16)

    def cols(lo, hi):
        c = {"keys": rows[lo:hi].copy()}
        if vk == "u64":
            c["values"] = value_column(vk, vals[lo:hi])
        return c
    want = O.lift_encoded([RC.canonical(STR, vk, "plain", s, v) for s, v in zip(strs, vals)])
    roots = {}
    for name in ("str15", "bytes16"):
        st = GpuFingerprintStore(RecordSchema.plain(name, vk), host_tier=False)
        st.load_bulk(cols(0, 300))
        roots[name, 300] = agg_int(st.aggregate())
        assert st.apply(cols(300, 305), np.zeros(5, np.uint8)) == (5, 0, 0)
        roots[name, 305] = agg_int(st.aggregate())
        assert st.size() == 305
        assert (st.batch_stats()["small"] == 0) == (name == "str15")
        st.close()
    for n in (300, 305):
        assert roots["str15", n] == fold(want[:n])
        assert roots["str15", n] != roots["bytes16", n]


# ---- GPU: the store against a dict model -----------------------------------------------------------

class Model(DictModel):
    """string -> (record, oracle fingerprint); a record is (key, (phys, logical, node), tomb, value)."""

    def __init__(self, w, vk, kind):
        super().__init__(f"str{w - 1}", vk, kind)
        self.vk = vk

    def check(self, st):
        """len and root, aggregate_keys over all nine bound-kind pairs, ranks / select / keys, and
        that no batch took the small path."""
        from rsos_hip import pack_str_keys, _abi as A
        from rsos_hip.store import _np_ptr
        ks = sorted(self.rows)
        n, fps = len(ks), [self.rows[k][1] for k in ks]
        assert st.size() == n
        assert agg_int(st.aggregate()) == fold(fps)
        probes = [ks[i] for i in range(0, n, max(n // 9, 1))] + [b"", b"\xff" * (self.w - 1), b"no such key"[:self.w - 1]]
        RC.check_key_ranges(st, ks, fps, ((lk, hk, *sorted((probes[(i * 3) % len(probes)], probes[(i * 5 + 4) % len(probes)])))
                                          for i, (lk, hk) in enumerate((a, b) for a in BOUND_KINDS for b in BOUND_KINDS)))
        asked = probes + [k + b"\x01" for k in probes if len(k) < self.w - 1]
        assert st.ranks(pack_str_keys(asked, self.w)).tolist() == [bisect.bisect_left(ks, k) for k in asked]
        for r in (0, 1, n // 2, n - 1):
            assert st.select(r) == ks[r]
        lo, q = n // 3, 70
        buf = np.zeros(q * self.w, np.uint8)
        A.check(st._f("keys")(st._h, lo, lo + q, _np_ptr(buf)), "rh_store_keys")
        assert buf.tobytes() == pack_str_keys(ks[lo:lo + q], self.w).tobytes()
        assert st.batch_stats()["small"] == 0


def records(rng, keys, vk, kind):
    mask = (1 << (8 * VBYTES[vk])) - 1
    out = []
    for k in keys:
        tomb = int(kind != "plain" and rng.integers(0, 8) == 0)
        stamp = (int(rng.integers(1, 1 << 40)), int(rng.integers(0, 1 << 20)), int(rng.integers(1, 1 << 40))) if kind == "dated" else (0, 0, 0)
        out.append((k, stamp, tomb, int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + 1 & mask))
    return out


def string_pool(rng, n, w):
    """n distinct strings of 0..w-1 bytes: names with shared prefixes, random bytes, trailing zeros."""
    pool = {b"", b"\0", b"\0\0", b"a", b"a\0", b"\xff" * (w - 1), b"\xff" * (w - 2)}
    i = 0
    while len(pool) < n:
        if i % 2:
            pool.add((b"ns-%d/pod-%06x" % (i % 13, int(rng.integers(0, 1 << 24))))[:w - 1])
        else:
            pool.add(rng.integers(0, 256, int(rng.integers(0, w)), dtype=np.uint8).tobytes())
        i += 1
    return list(pool)


@pytest.mark.gpu
@pytest.mark.parametrize("tier", [False, True], ids=["device", "tier"])
@pytest.mark.parametrize("w,vk,kind", [(16, "u64", "dated"), (32, "u32", "projection"), (64, "unit", "plain")],
                         ids=["str15-u64-dated", "str31-u32-projection", "str63-unit-plain"])
def test_store_against_model(gpu, oracle_lib, w, vk, kind, tier):
    """A base of 2,000 rows; host batches of 1, 7 and 700 rows (small-path sizes for a b16 / b32
    store) and of 3,000; apply_device and a 3-batch apply_device_many; stage with a key staged three
    times; deletes, an overwrite with the same value, a compaction -- after each step the store
    answers as a dict model lifted by the oracle does.  Bad host key rows change nothing."""
    import torch
    from rsos_hip import GpuFingerprintStore, _abi as A
    rng = np.random.default_rng(1000 * w + int(tier))
    pool = string_pool(rng, 7400, w)
    rng.shuffle(pool)
    base, fresh = sorted(pool[:2000]), pool[2000:]
    schema = schema_of(w, vk, kind)
    st, m = GpuFingerprintStore(schema, host_tier=tier), Model(w, vk, kind)
    recs = records(rng, base, vk, kind)
    st.load_bulk(m.cols(recs))
    m.apply(recs, [0] * len(recs))
    m.check(st)

    at = 0
    for size in (1, 7, 700, 3000):  # new keys, overwrites and deletes of held keys, shuffled
        n_del, n_ow = size // 10, size // 5
        held = sorted(m.rows)
        pick = [held[i] for i in rng.choice(len(held), n_del + n_ow, replace=False)]
        new = fresh[at:at + size - n_del - n_ow]
        at += len(new)
        batch = records(rng, new + pick[:n_ow], vk, kind) + [(k, (0, 0, 0), 0, 0) for k in pick[n_ow:]]
        ops = [0] * (len(new) + n_ow) + [1] * n_del
        perm = rng.permutation(size)
        batch, ops = [batch[i] for i in perm], [ops[i] for i in perm]
        assert st.apply(m.cols(batch), np.array(ops, np.uint8)) == (len(new), n_ow, n_del), size
        m.apply(batch, ops)
        m.check(st)

    # an overwrite with the same value: a zero delta
    root = agg_int(st.aggregate())
    same = [m.rows[k][0] for k in sorted(m.rows)[100:140]]
    assert st.apply(m.cols(same), np.zeros(40, np.uint8)) == (0, 40, 0)
    assert (st.size(), agg_int(st.aggregate())) == (len(m.rows), root)
    m.check(st)

    dev = records(rng, fresh[at:at + 150] + sorted(m.rows)[:50], vk, kind)
    at += 150
    dops = np.zeros(200, np.uint8)
    dops[10:20] = 1  # deletes of keys the store does not hold
    assert st.apply_device(to_device(m.cols(dev), gpu), torch.from_numpy(dops).to(gpu)) == (140, 50, 0)
    m.apply(dev, dops.tolist())
    m.check(st)

    qs = [records(rng, fresh[at + 100 * j:at + 100 * j + 100] + sorted(m.rows)[60 * j:60 * j + 20], vk, kind) for j in range(3)]
    at += 300
    assert st.apply_device_many([to_device(m.cols(q), gpu) for q in qs]) == [(100, 20, 0)] * 3
    for q in qs:
        m.apply(q, [0] * len(q))
    m.check(st)

    again = fresh[at]
    staged = records(rng, [again] + fresh[at + 1:at + 25] + [again] + sorted(m.rows)[500:523] + [again], vk, kind)
    sops = [0] * 50
    for j in (5, 30, 31):
        sops[j] = 1
    for lo, hi in ((0, 20), (20, 35), (35, 50)):
        st.stage(m.cols(staged[lo:hi]), np.array(sops[lo:hi], np.uint8))
    m.apply(staged, sops)
    m.check(st)  # the first question flushes
    assert m.rows[again][0] == staged[-1]  # the last op wins

    st.compact()
    m.check(st)

    good = m.cols(records(rng, fresh[at + 30:at + 40], vk, kind))
    bads = []
    k = good["keys"].copy()
    k[3, w - 1] = w  # a length byte no row of this width can hold
    bads.append((3, dict(good, keys=k)))
    k = good["keys"].copy()
    row = next(i for i in range(10) if k[i, w - 1] < w - 2)
    k[row, w - 2] = 1  # nonzero padding
    bads.append((row, dict(good, keys=k)))
    for row, bad in bads:
        for call in (lambda: st.apply(bad, np.zeros(10, np.uint8)), lambda: st.stage(bad, np.zeros(10, np.uint8)),
                     lambda: st.load_bulk(bad)):
            with pytest.raises(A.RsosHipError) as e:
                call()
            assert e.value.code == A.ERR_ARG and "RH_KEY_STR" in str(e.value) and f"row {row} " in str(e.value)
    m.check(st)
    st.close()


# ---- GPU: reconciliation ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tier", [False, True], ids=["device", "tier"])
def test_reconciliation_converges(gpu, oracle_lib, tier):
    """Two (str31, u64) dated stores of 2,000 rows that differ in 10 keys reconcile through
    rsos_hip.rbsr: the enumerated ranges hold exactly the differing keys, and after each side takes
    the other's newer records in those ranges both roots equal the oracle's fold of the union."""
    from rsos_hip import GpuFingerprintStore, rbsr as R
    rng = np.random.default_rng(31)
    pool = sorted(string_pool(rng, 2010, 32))
    rng.shuffle(pool)
    shared = records(rng, pool[:1995], "u64", "dated")
    a_recs, b_recs = list(shared), list(shared)
    for j in (321, 1500):  # a newer value on b
        k, stamp, tomb, v = shared[j]
        b_recs[j] = (k, (stamp[0] + 1, stamp[1], stamp[2]), 0, v ^ 1)
    # three keys only a holds, three only b holds, two that both hold with different stamps and values
    a_recs += records(rng, pool[1995:1998] + pool[2001:2003], "u64", "dated")
    b_recs += records(rng, pool[1998:2001] + pool[2001:2003], "u64", "dated")
    want = {shared[321][0], shared[1500][0], *pool[1995:2003]}
    assert len(a_recs) == len(b_recs) == 2000 and len(want) == 10
    stores, models = [], []
    for recs in (a_recs, b_recs):
        recs.sort(key=lambda r: r[0])
        m = Model(32, "u64", "dated")
        m.apply(recs, [0] * len(recs))
        st = GpuFingerprintStore(schema_of(32, "u64", "dated"), host_tier=tier)
        st.load_bulk(m.cols(recs))
        stores.append(st), models.append(m)
    (a, b), (ma, mb) = stores, models
    assert agg_int(a.aggregate()) == fold(v[1] for v in ma.rows.values()) != agg_int(b.aggregate())
    pol = R.FixedFanOut(16)
    log, ea, eb = reconcile(a, b, lambda v, act, ch, en: _outcome(R.protocol_round_with_policy(v, pol, act, ch, en)),
                            R.initial_ranges, max_rounds=100)
    ranges = ea + eb
    assert len(log) > 2

    def inside(key):
        return any((s is None or key >= s) and (e is None or key < e) for s, e in ranges)
    fa, fb = {k: v[1] for k, v in ma.rows.items()}, {k: v[1] for k, v in mb.rows.items()}
    differ = {k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k)}
    assert differ == want and len(differ) == 10 and all(inside(k) for k in differ)
    # each side takes the other's records in the enumerated ranges where they are newer (LWW)
    for st, m, other in ((a, ma, mb), (b, mb, ma)):
        take = [r for k, (r, _) in other.rows.items() if inside(k) and (k not in m.rows or m.rows[k][0][1] < r[1])]
        take.sort(key=lambda r: r[0])
        if take:
            st.apply(m.cols(take), np.zeros(len(take), np.uint8))
            m.apply(take, [0] * len(take))
    assert ma.rows == mb.rows and len(ma.rows) == 2003
    root = fold(v[1] for v in ma.rows.values())
    assert agg_int(a.aggregate()) == agg_int(b.aggregate()) == root and a.size() == b.size() == 2003
    assert a.batch_stats()["small"] == b.batch_stats()["small"] == 0
    a.close()
    b.close()


# ---- GPU: the sharded store ------------------------------------------------------------------------

@pytest.mark.gpu
def test_sharded_store_answers_as_one_store(gpu, oracle_lib):
    """3 shards on device 0, (str31, u64) dated: load, apply, stage and one protocol round answer as
    one store and the dict model do; a batch with one bad key row in the last shard's range is
    RH_ERR_ARG and leaves every shard's root as it was."""
    from rsos_hip import GpuFingerprintStore, RecordSchema, rbsr as R, _abi as A
    from rsos_hip.sharded import ShardedStore
    rng = np.random.default_rng(3)
    w, vk, kind = 32, "u64", "dated"
    schema = schema_of(w, vk, kind)
    pool = string_pool(rng, 2600, w)
    rng.shuffle(pool)
    base, fresh = sorted(pool[:2000]), pool[2000:]
    sh, one, m = ShardedStore(schema, [0, 0, 0]), GpuFingerprintStore(schema), Model(w, vk, kind)
    recs = records(rng, base, vk, kind)
    for st in (sh, one):
        st.load_bulk(m.cols(recs))
    m.apply(recs, [0] * len(recs))
    assert sh.sizes() == [666, 667, 667] and sh.splitters == [base[666], base[1333]]

    def check():
        ks = sorted(m.rows)
        fps = [m.rows[k][1] for k in ks]
        assert sh.size() == one.size() == len(ks)
        assert agg_int(sh.aggregate()) == agg_int(one.aggregate()) == fold(fps)
        assert sum(sh.sizes()) == len(ks)
        assert [agg_int(s.aggregate()) for s in sh.shards] == [
            fold(f for k, f in zip(ks, fps) if lo <= k and (hi is None or k < hi))
            for lo, hi in zip([b""] + sh.splitters, sh.splitters + [None])]
        for r in (0, 665, 666, 667, 1400, len(ks) - 1):
            assert sh.select(r) == one.select(r) == ks[r]
        for z in (ks[5], ks[700], ks[-1], b"zz-absent", b""):
            assert sh.rank(z) == bisect.bisect_left(ks, z)
        assert sh.batch_stats()["small"] == 0
    check()
    held = sorted(m.rows)
    batch = records(rng, fresh[:300] + held[::40], vk, kind) + [(k, (0, 0, 0), 0, 0) for k in held[7::50]]
    ops = [0] * 350 + [1] * 40
    perm = rng.permutation(len(batch))
    batch, ops = [batch[i] for i in perm], [ops[i] for i in perm]
    for st in (sh, one):
        assert st.apply(m.cols(batch), np.array(ops, np.uint8)) == (300, 50, 40)
    m.apply(batch, ops)
    check()
    staged = records(rng, fresh[300:340] + [fresh[300]], vk, kind)
    for st in (sh, one):
        st.stage(m.cols(staged), np.zeros(len(staged), np.uint8))
    m.apply(staged, [0] * len(staged))
    check()
    # one protocol round against a peer that lacks 3 keys
    peer = GpuFingerprintStore(schema)
    prs = [m.rows[k][0] for k in sorted(m.rows) if k not in (fresh[0], fresh[150], fresh[310])]
    peer.load_bulk(m.cols(prs))
    pol = R.FixedFanOut(16)
    outs = [R.protocol_round_segments(st, pol, R.initial_segments(peer)) for st in (sh, one)]
    (c1, e1, o1), (c2, e2, o2) = outs
    assert _outcome(o1) == _outcome(o2) and o1.split == 1 and len(c1) == 16
    assert c1.items(schema) == c2.items(schema) and e1.n == e2.n == 0
    peer.close()
    # a bad key row in the last shard's range: nothing changes anywhere
    roots = [agg_int(s.aggregate()) for s in sh.shards]
    bad_recs = sorted(records(rng, fresh[400:430], vk, kind), key=lambda r: r[0])
    cols = m.cols(bad_recs)
    assert bad_recs[-1][0] >= sh.splitters[1] and bad_recs[0][0] < sh.splitters[0]
    cols["keys"][-1, w - 1] = w
    for call in (lambda: sh.apply(cols, np.zeros(30, np.uint8)), lambda: sh.stage(cols, np.zeros(30, np.uint8)),
                 lambda: sh.load_bulk(cols)):
        with pytest.raises(A.RsosHipError) as e:
            call()
        assert e.value.code == A.ERR_ARG and "RH_KEY_STR" in str(e.value) and "row 29 " in str(e.value)
        assert [agg_int(s.aggregate()) for s in sh.shards] == roots
    check()
    with pytest.raises(A.RsosHipError) as e:
        ShardedStore(RecordSchema.dated("str31", "var"), [0, 0])
    assert e.value.code == A.ERR_UNSUPPORTED and "VARBYTES" in str(e.value)
    sh.close()
    one.close()


# ---- GPU: the rest ---------------------------------------------------------------------------------

@pytest.mark.gpu
def test_fingerprint_map_with_string_keys_and_fixed_values(gpu, oracle_lib):
    """FingerprintMap over str keys: a set of names (unit), a u32 map, and Entry values with
    tombstones under a dated u64 schema."""
    from rsos_hip import Entry, FingerprintMap, RecordSchema
    O = oracle_lib
    names = ["", "a", "default/pod-1", "kube-system/coredns-5d78c9869d-abcde", "x" * 63, "näme"]
    fm = FingerprintMap(RecordSchema.plain("str63", "unit"))
    for k in names:
        assert fm.insert(k, b"") is None
    assert fm.delete("a") == b"" and fm.delete("a") is None
    left = sorted((k for k in names if k != "a"), key=str.encode)
    agg = fm.aggregate()
    assert (agg.size, agg_int(agg)) == (5, fold(O.lift_encoded([RC.canonical(STR, "unit", "plain", k.encode(), None) for k in left])))
    assert [k for k, _ in fm.enumerate()] == left
    fm.close()
    fm = FingerprintMap(RecordSchema.plain("str15", "u32"))
    model = {"hello": 7, "world": (1 << 32) - 1, "": 0, "fifteen bytes..": 15}
    for k, v in model.items():
        fm.insert(k, v)
    assert fm.insert("hello", 8) == 7
    model["hello"] = 8
    agg = fm.aggregate()
    assert (agg.size, agg_int(agg)) == (4, fold(O.lift_encoded([RC.canonical(STR, "u32", "plain", k.encode(), v) for k, v in model.items()])))
    with pytest.raises(ValueError):
        fm.insert("sixteen bytes...", 1)
    fm.close()
    fm = FingerprintMap(RecordSchema.dated("str31", "u64"))
    rows = {"counter/a": Entry(5, 10, 0, 1), "counter/b": Entry((1 << 64) - 1, 11, 1, 2),
            "counter/gone": Entry(0, 12, 0, 3, tombstone=True), "k" * 31: Entry(1, 13, 0, 4)}
    for k, e in rows.items():
        fm.insert(k, e)
    agg = fm.aggregate()
    want = O.lift_encoded([RC.canonical(STR, "u64", "dated", k.encode(), e.value, (e.phys, e.logical, e.node), e.tombstone)
                           for k, e in rows.items()])
    assert (agg.size, agg_int(agg)) == (4, fold(want))
    assert fm.store.batch_stats()["small"] == 0
    fm.close()


@pytest.mark.gpu
def test_snapshot_refusals_name_the_key_kind(gpu):
    from rsos_hip import GpuFingerprintStore, RecordSchema, _abi as A
    from rsos_hip.snapshot import load_snapshot
    schema = RecordSchema.dated("str15", "u64")
    st = GpuFingerprintStore(schema)
    pr = GpuFingerprintStore(RecordSchema.projection("str15", "u64"))
    for kw in ({"dated": st}, {"projection": pr}, {"dated": st, "projection": pr}):
        for form in ("vec", "array"):
            with pytest.raises(A.RsosHipError) as e:
                load_snapshot(bytes(64), key_form=form, **kw)
            assert e.value.code == A.ERR_UNSUPPORTED and "RH_KEY_STR" in str(e.value)
    assert st.size() == 0
    st.close()
    pr.close()
    sc, none, info = schema.c(), A.Columns(), A.SnapshotInfo()
    for form in (0, 1):  # refused before the bytes are looked at
        assert A.lib().rh_snapshot_decode_device(C.byref(sc), form, None, 0, C.byref(none), 0, C.byref(info),
                                                 None) == A.ERR_UNSUPPORTED
        assert b"RH_KEY_STR" in A.lib().rh_last_error()
    # a byte-array value under a string key: refused by name everywhere, as before
    other = A.Schema(A.KEY_STR, 32, A.VAL_BYTES, 64, A.REC_DATED, 0)
    h = C.c_void_p()
    assert A.lib().rh_store_create(0, C.byref(other), C.byref(h)) == A.ERR_UNSUPPORTED
    assert b"RH_KEY_STR" in A.lib().rh_last_error() and not h.value
    cols = A.Columns()
    assert A.lib().rh_lift_records_async(C.byref(other), C.byref(cols), 0, None, None, None) == A.ERR_UNSUPPORTED
    assert b"RH_KEY_STR" in A.lib().rh_last_error()


def test_wire_codec_round_trip(rsos_hip_lib):
    """Range aggregates with string bounds under a (STR, u64) schema: RH_FORM_VEC round-trips and
    its bytes are the oracle codec's Vec<u8> encoding of the strings."""
    import wire as OW  # oracle/wire.py
    from rsos_hip import RecordSchema, wire
    from rsos_hip.fingerprint import Aggregate, Fingerprint
    schema = RecordSchema.dated("str31", "u64")
    ks = [b"", b"k", b"counter/requests", bytes(range(1, 32))]
    rng = np.random.default_rng(5)
    enc, _ = OW.key_codec("vec")
    items, want = [], b""
    for i, (s, e) in enumerate([(a, b) for a in ks + [None] for b in ks + [None]]):
        limbs = tuple(int(x) for x in rng.integers(0, 1 << 63, 4))
        items.append(wire.RangeAggregate(s, e, Aggregate(i * 7, Fingerprint(limbs))))
        want += OW.encode_range_aggregate(OW.RangeAggregate(s, e, limbs, i * 7), enc, None)
    data = wire.encode(schema, items, key_form="vec", msg_tag=None)
    assert data == want
    back, used = wire.decode_stream(schema, data, len(items), key_form="vec", msg_tag=None)
    assert back == items and used == len(data)
