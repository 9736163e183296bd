"""Short string keys in the column store (RH_KEY_STR): a `String` / `Vec<u8>` key of at most 15 /
31 bytes in a 16- / 32-byte row whose memcmp order is the strings' Ord, under `String` values
(RH_VAL_VARBYTES) -- the reference's own example map, ReplicatedMap<String, String>
(examples/k8s/main.rs:53).

Expected fingerprints come from the oracle alone: every record's canonical bytes are built by
tests/records_common.py with oracle/pyref.py's typed model and hashed by the C oracle
(oracle.lift_encoded) -- never by the product's encoder or a second GPU kernel.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyref as P  # oracle/pyref.py
import records_common as RC
from recon_common import DictView, _norm, _outcome, reconcile
from records_common import KINDS, STR_TOTALS as TOTALS, DictModel, agg_int, case_value, fold, ragged_records

SMALL = (0, 1, 2, 3, 4, 5, 7, 8)
WIDTHS = (16, 32)
N_LIFT = 600  # two whole 256-row blocks + an 88-row tail

# the order test's fixed strings: prefix families over the padding byte, the longest strings
FIXED = [b"", b"\0", b"\0\0", b"a", b"a\0", b"a\0\0", b"a\x01", b"ab", b"b", b"\xff" * 31, b"\xff" * 30,
         b"fifteen bytes..", b"sixteen bytes ..."[:16]]


def key_name(w):
    return f"str{w - 1}"


def schema_of(w, kind):
    from rsos_hip import RecordSchema
    return getattr(RecordSchema, kind)(key_name(w), "var")


tail_len = RC.tail_len
prefix_len = functools.partial(RC.prefix_len, "str31")  # (kind, key length): the width does not enter


@functools.lru_cache(maxsize=None)
def lift_case(w, kind, tags=True):
    """600 records of one shape (records_common.build_lift_case).  Row i's key has i % w bytes, but
    for a few rows below (every length 0..w-1: all four byte alignments of the fields behind it,
    every word shift).  Two present rows carry each TOTALS message length (a row whose prefix is
    longer than the total, 63 against 71, takes a shorter key instead), others the SMALL lengths.
    (Row 599 is a tombstone of the tagged kinds.)"""
    return RC.build_lift_case(key_name(w), "var", kind, tags, N_LIFT, 1000 * w + sum(kind.encode()) + int(tags),
                              totals=TOTALS, per_total=2, small=SMALL)


@functools.lru_cache(maxsize=None)
def lift_want(w, kind, tags=True):
    import oracle as O
    return O.lift_encoded(lift_case(w, kind, tags)["blobs"], threads=4)


# ---- CPU ------------------------------------------------------------------------------------------

def test_schema_helpers(rsos_hip_lib):
    from rsos_hip import RecordSchema, _abi as A
    for name, w in (("str15", 16), ("str31", 32)):
        for kind in KINDS:
            s = getattr(RecordSchema, kind)(name, "var")
            assert (s.key_kind, s.key_len, s.key_row) == (A.KEY_STR, w, w)
            assert s.supported()
            # an empty key and an empty value: 8 + stamp + variant + 8; "add L" for a key of L bytes
            assert s.record_len() == prefix_len(kind, 0) == 8 + tail_len(kind)
            assert s.record_len(True) == (8 + tail_len(kind) - 8 if kind != "plain" else 16)
    assert RecordSchema.dated("str31", "var").record_len() == 40
    assert RecordSchema.dated("str31", "var").record_len(True) == 32
    assert RecordSchema.projection("str15", "var").record_len(True) == 12
    bad = A.Schema(A.KEY_STR, 24, A.VAL_VARBYTES, 0, A.REC_PLAIN, 0)
    assert A.lib().rh_schema_supported(C.byref(bad)) == A.ERR_ARG
    assert b"RH_KEY_STR" in A.lib().rh_last_error()
    assert A.lib().rh_schema_record_len(C.byref(bad), 0) == A.ERR_ARG
    other = A.Schema(A.KEY_STR, 32, A.VAL_BYTES, 64, A.REC_DATED, 0)
    assert A.lib().rh_schema_supported(C.byref(other)) == 0
    assert not RecordSchema.dated("str31", "bytes64").supported()
    with pytest.raises(ValueError):
        RecordSchema.plain("var", "var")
    with pytest.raises(ValueError):
        RecordSchema.plain("u64", "str31")


def order_strings():
    rng = np.random.default_rng(5)
    rand = [rng.integers(0, 256, int(rng.integers(0, 32)), dtype=np.uint8).tobytes() for _ in range(500)]
    # (random bytes seldom share a prefix: extend some by zero bytes and by one more byte)
    fam = [s[:20] + t for s in rand[:40] for t in (b"\0", b"\0\0", b"\x01")]
    return FIXED + rand + fam


def test_row_order_is_string_order():
    from rsos_hip import pack_str_keys, unpack_str_keys
    strs = order_strings()
    assert len(FIXED[-2]) == 15 and len(FIXED[-1]) == 16
    rows = pack_str_keys(strs, 32)
    assert rows.shape == (len(strs), 32) and rows.dtype == np.uint8
    assert unpack_str_keys(rows) == strs
    by_rows = sorted(range(len(strs)), key=lambda i: (rows[i].tobytes(), i))
    by_strs = sorted(range(len(strs)), key=lambda i: (strs[i], i))
    assert by_rows == by_strs
    assert [rows[i].tobytes() for i in by_rows] == sorted(r.tobytes() for r in rows)
    short = [s for s in strs if len(s) <= 15]
    rows16 = pack_str_keys(short, 16)
    assert unpack_str_keys(rows16) == short
    assert sorted(range(len(short)), key=lambda i: (rows16[i].tobytes(), i)) == \
        sorted(range(len(short)), key=lambda i: (short[i], i))
    assert pack_str_keys(["héllo"], 16)[0, 15] == 6 and unpack_str_keys(pack_str_keys(["héllo"], 16)) == ["héllo".encode()]
    with pytest.raises(ValueError):
        pack_str_keys([b"x" * 32], 32)
    with pytest.raises(ValueError):
        pack_str_keys([b"x" * 16], 16)


@pytest.mark.parametrize("msg_tag", [None, 0])
def test_wire_codec(rsos_hip_lib, msg_tag):
    """STR keys of lengths 0, 1, 15 and 31 on bounded and unbounded sides: RH_FORM_VEC round-trips
    and its bytes are the oracle codec's Vec<u8> encoding of the strings."""
    import wire as W  # oracle/wire.py
    from rsos_hip import RecordSchema, wire, _abi as A
    from rsos_hip.fingerprint import Aggregate, Fingerprint
    schema = RecordSchema.dated("str31", "var")
    ks = [b"", b"k", b"fifteen bytes..", bytes(range(1, 32))]
    assert [len(k) for k in ks] == [0, 1, 15, 31]
    rng = np.random.default_rng(2)
    items, want = [], b""
    enc, _ = W.key_codec("vec")
    for i, (s, e) in enumerate([(None, None)] + [(a, b) for a in ks + [None] for b in ks + [None]]):
        limbs = tuple(int(x) for x in rng.integers(0, 1 << 63, 4))
        items.append(wire.RangeAggregate(s, e, Aggregate(i * 300, Fingerprint(limbs))))
        want += W.encode_range_aggregate(W.RangeAggregate(s, e, limbs, i * 300), enc, msg_tag)
    data = wire.encode(schema, items, key_form="vec", msg_tag=msg_tag)
    assert data == want
    back, used = wire.decode_stream(schema, data, len(items), key_form="vec", msg_tag=msg_tag)
    assert back == items and used == len(data)
    short = RecordSchema.plain("str15", "var")
    fit = [it for it in items if all(k is None or len(k) <= 15 for k in (it.start, it.end))]
    assert len(fit) == 17 and wire.decode_stream(short, wire.encode(short, fit, key_form="vec"), 99, key_form="vec")[0] == fit
    # a key of 32 bytes does not fit the row: RH_ERR_DATA, as a 16-byte one for a 16-byte row
    long_item = W.encode_range_aggregate(W.RangeAggregate(b"x" * 32, None, (1, 2, 3, 4), 5), enc, msg_tag)
    for sc, blob in ((schema, long_item), (short, W.encode_range_aggregate(W.RangeAggregate(None, b"y" * 16, (1, 2, 3, 4), 5), enc, msg_tag))):
        with pytest.raises(A.RsosHipError) as e:
            wire.decode_stream(sc, blob, 4, key_form="vec", msg_tag=msg_tag)
        assert e.value.code == A.ERR_DATA
    for call in (lambda: wire.encode(schema, items, key_form="array", msg_tag=msg_tag),
                 lambda: wire.decode_stream(schema, data, 4, key_form="array", msg_tag=msg_tag)):
        with pytest.raises(A.RsosHipError) as e:
            call()
        assert e.value.code == A.ERR_ARG


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", WIDTHS)
def test_generated_inputs_cover_the_cases(rsos_hip_lib, w, kind):
    """The lift test's inputs themselves: every key length, every alignment of a value's start
    against every alignment of the prefix's end, every target total, empty values, the tombstone
    pattern, and (width 32 dated) prefixes that end in block 1."""
    from rsos_hip import unpack_str_keys
    c = lift_case(w, kind)
    n = c["n"]
    assert n == N_LIFT and n > 2 * 256 and n % 256
    assert c["offsets"][0] == 0 and int(c["offsets"][n]) == len(c["heap"])
    assert all(int(c["offsets"][i + 1] - c["offsets"][i]) == c["lens"][i] for i in range(n))
    assert unpack_str_keys(c["keys"]) == c["strs"] and c["keys"].shape == (n, w)
    assert {len(s) for s in c["strs"]} == set(range(w))
    present = [i for i in range(n) if not c["tomb"][i]]
    assert {len(c["strs"][i]) for i in present} == set(range(w))
    assert {(int(c["offsets"][i]) % 4, len(c["strs"][i]) % 4) for i in present if c["lens"][i]} == \
        {(a, b) for a in range(4) for b in range(4)}
    totals = [len(c["blobs"][i]) for i in present]
    assert all(totals.count(t) >= 2 for t in TOTALS)
    assert all(len(c["blobs"][i]) == prefix_len(kind, len(c["strs"][i])) + int(c["lens"][i]) for i in present)
    assert any(c["lens"][i] == 0 for i in present) and all(any(c["lens"][i] == s for i in present) for s in SMALL)
    plens = {prefix_len(kind, len(c["strs"][i])) for i in present}
    assert min(plens) == 8 + tail_len(kind) and max(plens) == 8 + w - 1 + tail_len(kind) <= 71
    if (w, kind) == (32, "dated"):
        # prefixes past block 0, with empty, short and block-filling values behind them
        over = [i for i in present if prefix_len(kind, len(c["strs"][i])) > 64]
        assert {prefix_len(kind, len(c["strs"][i])) for i in over} == set(range(65, 72))
        assert any(c["lens"][i] > 64 for i in over) and any(0 < c["lens"][i] < 50 for i in over)
    if kind != "plain":
        assert all(c["tomb"][i] == (i % 5 == 4) for i in range(n))
        assert c["lens"][9] > 0 and c["tomb"][9]
        assert all(len(c["blobs"][i]) == prefix_len(kind, len(c["strs"][i])) - 8 for i in range(n) if c["tomb"][i])
        assert {len(c["strs"][i]) % 4 for i in range(n) if c["tomb"][i]} == {0, 1, 2, 3}
    last = present[-1]
    assert last >= n - 2 and c["lens"][last] > 0 and int(c["offsets"][last + 1]) == len(c["heap"])


# ---- GPU: the lift ---------------------------------------------------------------------------------

def check_lift(gpu, w, kind, tags, lead, slack):
    RC.check_var_lift(gpu, schema_of(w, kind), lift_case(w, kind, tags), lift_want(w, kind, tags), lead, slack,
                      tell=("key lengths", "message lengths"))


@pytest.mark.gpu
@pytest.mark.parametrize("tight", [False, True], ids=["slack", "tight"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", WIDTHS)
def test_lift_parity(gpu, oracle_lib, w, kind, tight):
    """Every row's fingerprint and every 256-row block sum equal the oracle's: once with filler
    before and after the values, once with the first value at heap offset 0 and bytes_len =
    round_up(offsets[n], 4)."""
    check_lift(gpu, w, kind, True, 0 if tight else 5, 0 if tight else 64)


@pytest.mark.gpu
def test_lift_parity_without_a_tag_column(gpu, oracle_lib):
    """A dated batch with no tag column: every row present."""
    check_lift(gpu, 32, "dated", False, 0, 0)


@pytest.mark.gpu
def test_padding_is_not_hashed(gpu, oracle_lib):
    """The device key column's padding bytes set to 0xA5 (a caller error): the fingerprints are
    still those of the strings, since the lift masks the row at and past the string's length."""
    from rsos_hip import lift_records
    case, want = lift_case(32, "dated"), lift_want(32, "dated")
    keys = case["keys"].copy()
    for i, s in enumerate(case["strs"]):
        keys[i, len(s):31] = 0xA5
    assert (keys != case["keys"]).any(axis=1).sum() == sum(1 for s in case["strs"] if len(s) < 31)
    schema = schema_of(32, "dated")
    fps, _ = lift_records(schema, RC.device_cols(case, schema, gpu, 5, 64, keys=keys))
    assert np.array_equal(fps.cpu().numpy(), want)


@pytest.mark.gpu
def test_framing(gpu, oracle_lib):
    """lift("ab", "c") != lift("a", "bc"): the lengths are hashed (rsos/src/fingerprint/tests.rs:99)."""
    import torch
    from rsos_hip import RecordSchema, lift_records, pack_str_keys
    schema = RecordSchema.plain("str15", "var")
    heap = np.frombuffer(b"cbc\0", np.uint8).copy()
    fps, _ = lift_records(schema, {"keys": torch.from_numpy(pack_str_keys(["ab", "a"], 16)).to(gpu),
                                   "values": torch.from_numpy(heap).to(gpu),
                                   "value_offsets": torch.tensor([0, 1, 3], dtype=torch.int64, device=gpu)})
    got = fps.cpu().numpy()
    assert got[0].tobytes() != got[1].tobytes()
    assert got[0].tobytes() == P.lift(P.Str(b"ab"), P.Str(b"c"))
    assert got[1].tobytes() == P.lift(P.Str(b"a"), P.Str(b"bc"))


@pytest.mark.gpu
def test_dual_lift_equals_the_two_single_lifts(gpu, oracle_lib):
    import oracle as O
    from rsos_hip import lift_dual, lift_records
    case = lift_case(32, "dated")
    schema = schema_of(32, "dated")
    cols = RC.device_cols(case, schema, gpu, 5, 64)
    fd, bd, fp, bp = lift_dual(schema, cols)
    f1, b1 = lift_records(schema, cols)
    f2, b2 = lift_records(schema_of(32, "projection"), {k: v for k, v in cols.items()
                                                         if k not in ("phys", "logical", "node")})
    for a, b in ((fd, f1), (bd, b1), (fp, f2), (bp, b2)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(f1.cpu().numpy(), lift_want(32, "dated"))
    blobs = [RC.canonical("str31", "var", "projection", case["strs"][i], case_value(case, i), tomb=bool(case["tomb"][i]))
             for i in range(case["n"])]
    assert np.array_equal(fp.cpu().numpy(), O.lift_encoded(blobs, threads=4))


# ---- GPU: the store against a model ----------------------------------------------------------------

def string_pool(rng, n):
    """n distinct strings of 0..31 bytes: the order test's prefix families, names, random bytes."""
    pool = set(s for s in order_strings() if len(s) <= 31)
    i = 0
    while len(pool) < n:
        pool.add(b"node-%d/%s" % (i, b"x" * int(rng.integers(0, 12))) if i % 2 else
                 rng.integers(0, 256, int(rng.integers(0, 32)), dtype=np.uint8).tobytes())
        i += 1
    return list(pool)


@pytest.mark.gpu
@pytest.mark.parametrize("tier", [False, True], ids=["device", "tier"])
def test_store_against_model(gpu, oracle_lib, tier):
    """load, apply (new / overwrite with another length / delete), the same batch again, a staged
    batch with a key staged three times, a device batch, a compaction -- size, root, 16 rank
    ranges, the keys as strings in sorted() order, every fingerprint, rank / select and key-range
    aggregates with string bounds equal a dict model lifted by the oracle after each; malformed
    host key rows and bad host offsets are RH_ERR_ARG and change nothing."""
    import torch
    from rsos_hip import GpuFingerprintStore, RecordSchema, _abi as A
    rng = np.random.default_rng(11)
    pool = string_pool(rng, 1400)
    fixed = [s for s in FIXED if len(s) <= 31]
    rest = [s for s in pool if s not in set(fixed)]
    rng.shuffle(rest)
    base = sorted(fixed + rest[:1000 - len(fixed)])  # the prefix families are loaded
    fresh = rest[1000 - len(fixed):]
    absent = fresh[380:400] + [b"a\0\0\0", b"\xff" * 29]
    schema = RecordSchema.dated("str31", "var")
    st, m = GpuFingerprintStore(schema, host_tier=tier), DictModel("str31", "var")
    recs = ragged_records(rng, base, long_every=90)
    st.load_bulk(m.cols(recs))
    m.apply(recs, [0] * len(recs))
    m.check(st, absent)
    assert len(base) == 1000 and max(len(r[3]) for r in recs) == 5000

    ow = [base[i] for i in rng.choice(1000, 200, replace=False)]
    batch = ragged_records(rng, fresh[:100] + ow[:100], long_every=40) + [(k, (0, 0, 0), 0, b"") for k in ow[100:]]
    ops = [0] * 200 + [1] * 100
    perm = rng.permutation(300)
    batch, ops = [batch[i] for i in perm], [ops[i] for i in perm]
    for k in ow[:100]:  # an overwrite's new value has another length
        old = m.rows[k][0]
        new = next(r for r in batch if r[0] == k)
        if len(new[3]) == len(old[3]) and not new[2]:
            batch[batch.index(new)] = (k, new[1], 0, new[3] + b"!")
    assert st.apply(m.cols(batch), np.array(ops, np.uint8)) == (100, 100, 100)
    m.apply(batch, ops)
    m.check(st, absent)
    root = agg_int(st.aggregate())
    # delivered again: every insert meets its own record, every delete a key already gone
    k_ins = sum(1 for op in ops if op == 0)
    assert st.apply(m.cols(batch), np.array(ops, np.uint8)) == (0, k_ins, 0)
    assert (st.size(), agg_int(st.aggregate())) == (len(m.rows), root)
    m.check(st, absent)
    assert st.batch_stats()["small"] == 0

    again = fresh[100]
    staged = ragged_records(rng, [again] + fresh[101:125] + [again] + ow[:23] + [again], long_every=25)
    sops = [0] * 50
    for j in (5, 30, 31):  # a few staged deletes, one of a key never inserted
        sops[j] = 1
    assert len(staged) == 50 and staged[0][3] != staged[-1][3]
    for lo, hi in ((0, 20), (20, 35), (35, 50)):  # in three calls
        st.stage(m.cols(staged[lo:hi]), np.array(sops[lo:hi], np.uint8))
    m.apply(staged, sops)
    m.check(st, absent)  # the first question flushes
    assert m.rows[again][0][3] == staged[-1][3]

    dev = ragged_records(rng, fresh[200:232] + ow[40:72], long_every=16)
    assert st.apply_device(RC.to_device(m.cols(dev), gpu), torch.zeros(64, dtype=torch.uint8, device=gpu)) == (32, 32, 0)
    m.apply(dev, [0] * 64)
    m.check(st, absent)

    st.compact()
    m.check(st, absent)
    assert st.batch_stats()["small"] == 0

    good = m.cols(ragged_records(rng, fresh[300:310]))
    bads = []
    k = good["keys"].copy()
    k[3, 31] = 32  # a length byte no 32-byte row can hold
    bads.append(("length", dict(good, keys=k)))
    k = good["keys"].copy()
    row = next(i for i in range(10) if k[i, 31] < 30)
    k[row, 30] = 1  # nonzero padding
    bads.append(("padding", dict(good, keys=k)))
    offs = good["value_offsets"].copy()
    offs[4], offs[5] = offs[3] + 1, offs[3]
    assert offs[5] < offs[4]
    bads.append(("offsets", dict(good, value_offsets=offs)))
    offs = good["value_offsets"].copy()
    offs[-1] = good["values"].size + 1
    bads.append(("offsets", dict(good, value_offsets=offs)))
    for what, bad in bads:
        for call in (lambda: st.apply(bad, np.zeros(10, np.uint8)), lambda: st.stage(bad, np.zeros(10, np.uint8)),
                     lambda: st.load_bulk(bad)):
            with pytest.raises(A.RsosHipError) as e:
                call()
            assert e.value.code == A.ERR_ARG, what
            if what != "offsets":
                assert "RH_KEY_STR" in str(e.value) and "row" in str(e.value)
    m.check(st, absent)
    st.close()


# ---- GPU: reconciliation ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def recon_sides():
    """Two replicas of 3,000 rows that differ in 7 keys: one changed value, three keys only a
    holds, three only b holds -- among them a string (only a) and its one-byte extension (only b)."""
    rng = np.random.default_rng(23)
    pool = sorted(string_pool(rng, 3010))
    pool = [s for s in pool if s not in (b"host-7", b"host-7\0")]
    rng.shuffle(pool)
    shared = [(k, s, 0, v) for k, s, _, v in ragged_records(rng, sorted(pool[:2997]), long_every=300)]
    a_recs, b_recs = list(shared), list(shared)
    ch = shared[321]
    b_recs[321] = (ch[0], ch[1], 0, ch[3] + b"\0")  # same key and stamp: one trailing value byte
    only_a = [b"host-7", pool[2997], pool[2998]]
    only_b = [b"host-7\0", pool[2999], pool[3000]]
    a_recs += [(k, (5, 5, 5), 0, b"only a") for k in only_a]
    b_recs += [(k, (5, 5, 5), 0, b"only b") for k in only_b]
    want = {ch[0], *only_a, *only_b}
    assert len(want) == 7 and len(a_recs) == len(b_recs) == 3000
    models = []
    for recs in (a_recs, b_recs):
        recs.sort(key=lambda r: r[0])
        m = DictModel("str31", "var")
        m.apply(recs, [0] * len(recs))
        models.append((recs, m))
    return models, want


@pytest.mark.gpu
@pytest.mark.parametrize("tier", [False, True], ids=["device", "tier"])
@pytest.mark.parametrize("policy", ["fixed16", "sqrt"])
def test_reconciliation_matches_the_literal_driver(gpu, oracle_lib, policy, tier):
    """rsos_hip.rbsr's rounds between two str31 stores equal oracle/rbsr.py's literal driver over
    the same rows round by round, and the enumerated ranges hold exactly the differing keys."""
    import rbsr as OR  # oracle/rbsr.py
    from rsos_hip import GpuFingerprintStore, RecordSchema, rbsr as R
    (ra, ma), (rb, mb) = recon_sides()[0]
    want_keys = recon_sides()[1]
    schema = RecordSchema.dated("str31", "var")
    stores = []
    for recs, m in ((ra, ma), (rb, mb)):
        st = GpuFingerprintStore(schema, host_tier=tier)
        st.load_bulk(m.cols(recs))
        stores.append(st)
    a, b = stores
    assert a.size() == b.size() == 3000
    pol, decide = {"fixed16": (R.FixedFanOut(16), OR.fixed_fan_out(16)), "sqrt": (R.SqrtFanOut(), OR.sqrt_fan_out)}[policy]
    want_log = reconcile(DictView(ma), DictView(mb), lambda v, act, ch, en: OR.protocol_round(v, decide, act, ch, en),
                         OR.initial_ranges, max_rounds=100)[0]
    got_log, ea, eb = reconcile(a, b, lambda v, act, ch, en: _outcome(R.protocol_round_with_policy(v, pol, act, ch, en)),
                                R.initial_ranges, max_rounds=100)
    ranges = ea + eb
    assert len(got_log) == len(want_log) > 2
    for (gc, ge, go), (wc, we, wo) in zip(got_log, want_log):
        assert go == wo and ge == we and gc == wc

    def inside(key):
        return any((s is None or key >= s) and (e is None or key < e) for s, e in ranges)
    fa = {k: v[1] for k, v in ma.rows.items()}
    fb = {k: v[1] for k, v in mb.rows.items()}
    assert {k for k in set(fa) | set(fb) if inside(k) and fa.get(k) != fb.get(k)} == want_keys
    assert all(fa.get(k) == fb.get(k) for k in set(fa) | set(fb) if not inside(k))
    # the same rounds in SoA form, each round's children through the wire codec (Vec<u8> keys)
    from rsos_hip import wire
    active, k = R.initial_segments(a), 0
    while len(active):
        ch, en, o = R.protocol_round_segments((b, a)[k % 2], pol, active)
        assert _outcome(o) == want_log[k][2] and _norm(ch.items(schema)) == want_log[k][0]
        items = ch.items(schema)
        data = wire.encode(schema, items, key_form="vec", msg_tag=wire.COMPARISON_ITEM)
        back, used = wire.decode_stream(schema, data, len(items), key_form="vec", msg_tag=wire.COMPARISON_ITEM)
        assert back == items and used == len(data)
        active, k = R.Segments.from_items(schema, back), k + 1
    assert k == len(want_log)
    a.close()
    b.close()


# ---- GPU: FingerprintMap ---------------------------------------------------------------------------

@pytest.mark.gpu
def test_fingerprint_map_with_string_keys(gpu, oracle_lib):
    from rsos_hip import Entry, FingerprintMap, RecordSchema
    from rsos_hip.store import KeyRange
    O = oracle_lib
    fm = FingerprintMap(RecordSchema.dated("str31", "var"))
    model = {}

    def put(k, v, stamp, tomb=False):
        old = fm.insert(k, Entry("" if tomb else v, *stamp, tombstone=tomb))
        assert (old is None) == (k not in model) and (old is None or old.value == model[k][0])
        model[k] = ("" if tomb else v, stamp, tomb)
    put("pod/web-0", "Running", (10, 0, 1))
    put("pod/web-1", "Pending", (11, 0, 1))
    put("pod/web", "", (12, 1, 2))
    put("", "the empty key", (13, 0, 2))
    put("näme", "ü" * 700, (14, 0, 3))  # UTF-8 key bytes; a value of more than one chunk
    put("x" * 31, "longest key", (15, 0, 3))
    put("pod/web-1", "Running, after a restart", (16, 0, 1))
    put("pod/web-0", None, (17, 0, 1), tomb=True)
    assert fm.delete("pod/web").value == "" and fm.delete("pod/web") is None and fm.delete("nope") is None
    del model["pod/web"]
    with pytest.raises(ValueError):
        fm.insert("y" * 32, Entry("too long a key", 1, 1, 1))
    assert fm.size() == len(model) == 5
    assert fm.get("pod/web-1").value == "Running, after a restart" and fm.get("pod/web") is None

    def fp(k):
        v, stamp, tomb = model[k]
        return O.lift_encoded([RC.canonical("str31", "var", "dated", k.encode(), v.encode(), stamp, tomb)])[0].tobytes()
    order = sorted(model, key=str.encode)
    assert order == sorted(model)  # code point order is UTF-8 byte order
    agg = fm.aggregate()
    assert (agg.size, agg_int(agg)) == (len(model), fold(fp(k) for k in order))
    assert [k for k, _ in fm.enumerate()] == order
    assert [k for k, _ in fm.store.enumerate()] == [k.encode() for k in order]
    part = fm.aggregate(KeyRange("pod/", "pod0"))
    inside = [k for k in order if "pod/" <= k < "pod0"]
    assert len(inside) == 2 and (part.size, agg_int(part)) == (2, fold(fp(k) for k in inside))
    assert fm.rank("pod/web-1") == order.index("pod/web-1") == fm.store.rank("pod/web-1")
    assert fm.store.select(0) == b""
    fm.close()


# ---- GPU: what VARBYTES lacks, STR keys lack too ---------------------------------------------------

@pytest.mark.gpu
def test_refusals(gpu):
    from rsos_hip import GpuFingerprintStore, RecordSchema, _abi as A
    from rsos_hip.snapshot import load_snapshot
    schema = RecordSchema.dated("str31", "var")
    st = GpuFingerprintStore(schema)
    with pytest.raises(A.RsosHipError) as e:
        load_snapshot(bytes(64), dated=st, key_form="vec")
    assert e.value.code == A.ERR_UNSUPPORTED and "VARBYTES" in str(e.value)
    st.close()
    s = schema.c()
    cols, out = A.Columns(), (C.c_uint8 * 32)()
    assert A.lib().rh_lift_host(0, C.byref(s), C.byref(cols), 1, out) == A.ERR_UNSUPPORTED
    assert b"VARBYTES" in A.lib().rh_last_error()
    # a value kind other than VARBYTES under string keys: refused by name
    other = A.Schema(A.KEY_STR, 32, A.VAL_BYTES, 64, A.REC_DATED, 0)
    h = C.c_void_p()
    assert A.lib().rh_store_create(0, C.byref(other), C.byref(h)) == A.ERR_UNSUPPORTED
    assert b"RH_KEY_STR" in A.lib().rh_last_error() and not h.value
