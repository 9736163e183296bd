"""String keys of up to 63 bytes in 64-byte rows (RH_KEY_STR, key_len 64; 'str63'): the width at
which the reference's example map -- ReplicatedMap<String, String> keyed by Kubernetes object
names, examples/k8s/main.rs:53 -- stays in the column store.  At this width the key, the fields
behind it and the first value words can straddle the edge between message blocks 0 and 1, and a
tombstone's message can take two blocks.

Expected fingerprints come from the oracle alone, as in test_str_keys.py: canonical bytes built by
tests/records_common.py with oracle/pyref.py's typed model and hashed by the C oracle
(oracle.lift_encoded).
"""
import bisect
import ctypes as C
import functools

import numpy as np
import pytest

import records_common as RC
from recon_common import DictView, _norm, _outcome, reconcile
from records_common import (BOUND_KINDS, KINDS, STR_TOTALS as TOTALS, DictModel, agg_int, case_value, fold, ragged_records,
                            tail_len, to_device)

W = 64
N_LIFT = 600  # two whole 256-row blocks + an 88-row tail
prefix_len = functools.partial(RC.prefix_len, "str63")  # (kind, key length)
SMALL = tuple(range(9))  # values of 0..8 bytes
QUESTIONS = (1, 32, 33, 64, 65, 200)  # around the one-launch query's 64 and half of it


def schema_of(kind):
    from rsos_hip import RecordSchema
    return getattr(RecordSchema, kind)("str63", "var")


# ---- the lift's inputs ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lift_case(kind, tags=True):
    """600 records (records_common.build_lift_case).  Row i's key has i % 64 bytes, but for the rows
    below: every length 0..63, so every byte alignment and word shift, keys that end at the block
    edge (56) and past it (57..63), prefixes that end in block 0, at byte 64 and in block 1.  Two
    present rows carry each TOTALS message length, others values of 0..8 bytes; these special rows
    come from rows 128..: rows 0..127 keep every key length twice among the present rows, with
    their random value lengths.  A prefix that ends in block 0, at byte 64 and in block 1 (twice)
    comes with no value, a value that ends inside that block and one that goes on past it.  With
    tags every 5th row is a tombstone (5 and 64 are coprime: every key length, so messages below,
    at and above 64 bytes)."""
    return RC.build_lift_case("str63", "var", kind, tags, N_LIFT, 64000 + sum(kind.encode()) + int(tags), totals=TOTALS,
                              per_total=2, small=SMALL, slots_from=128, edge_klens=(3, 56 - tail_len(kind), 60, 63))


@functools.lru_cache(maxsize=None)
def lift_want(kind, tags=True):
    import oracle as O
    return O.lift_encoded(lift_case(kind, tags)["blobs"], threads=4)


# ---- CPU ------------------------------------------------------------------------------------------

def test_schema_helpers(rsos_hip_lib):
    from rsos_hip import RecordSchema, _abi as A
    for kind in KINDS:
        s = getattr(RecordSchema, kind)("str63", "var")
        assert (s.key_kind, s.key_len, s.key_row) == (A.KEY_STR, 64, 64)
        assert s.is_str and s.is_var and s.supported()
        # the empty key and an empty value: 8 + stamp + variant + 8; add L for a key of L bytes
        assert s.record_len() == prefix_len(kind, 0) == 8 + tail_len(kind)
        assert s.record_len(True) == (8 + tail_len(kind) - 8 if kind != "plain" else 16)
    assert RecordSchema.dated("str63", "var").record_len() == 40
    assert RecordSchema.dated("str63", "var").record_len(True) == 32
    assert RecordSchema.projection("str63", "var").record_len(True) == 12
    lib = A.lib()
    ok = A.Schema(A.KEY_STR, 64, A.VAL_VARBYTES, 0, A.REC_DATED, 0)
    assert lib.rh_schema_supported(C.byref(ok)) == 1
    assert lib.rh_schema_record_len(C.byref(ok), 0) == 40 and lib.rh_schema_record_len(C.byref(ok), 1) == 32
    other = A.Schema(A.KEY_STR, 64, A.VAL_BYTES, 64, A.REC_DATED, 0)
    assert lib.rh_schema_supported(C.byref(other)) == 0
    assert not RecordSchema.dated("str63", "bytes64").supported()
    for w in (48, 63, 65, 128):  # no other width
        bad = A.Schema(A.KEY_STR, w, A.VAL_VARBYTES, 0, A.REC_PLAIN, 0)
        assert lib.rh_schema_supported(C.byref(bad)) == A.ERR_ARG
        assert b"RH_KEY_STR" in lib.rh_last_error() and b"64" in lib.rh_last_error()
    with pytest.raises(ValueError):
        RecordSchema.plain("u64", "str63")


def order_strings():
    """Sorted by bytes order below; a fixed part and a few thousand random strings over three
    letters (many shared prefixes, many that differ only in trailing zero bytes)."""
    fixed = [b""] + [b"\0" * k for k in (1, 2, 3, 31, 32, 62, 63)] + [b"a" + b"\0" * k for k in (0, 1, 2, 30, 31, 61, 62)]
    fixed += [b"k" * 62 + b"y", b"k" * 62 + b"z"]           # 63 bytes, the last one differs
    fixed += [b"\xff" * 62, b"\xff" * 63]                    # a proper prefix of the longest string
    fixed += [b"pod/web", b"pod/web\0", b"pod/web\0\0", b"pod/web" + b"\0" * 56]  # trailing zeros: the length byte orders
    rng = np.random.default_rng(63)
    alpha = np.frombuffer(b"\0ab", np.uint8)
    rand = [alpha[rng.integers(0, 3, int(rng.integers(0, 64)))].tobytes() for _ in range(3000)]
    return fixed + rand


def test_row_order_is_string_order():
    from rsos_hip import pack_str_keys, unpack_str_keys
    strs = order_strings()
    assert max(len(s) for s in strs) == 63 and min(len(s) for s in strs) == 0
    rows = pack_str_keys(strs, 64)
    assert rows.shape == (len(strs), 64) and rows.dtype == np.uint8
    assert unpack_str_keys(rows) == strs
    assert all(rows[i, 63] == len(s) and not rows[i, len(s):63].any() for i, s in enumerate(strs))
    by_rows = sorted(range(len(strs)), key=lambda i: (rows[i].tobytes(), i))
    by_strs = sorted(range(len(strs)), key=lambda i: (strs[i], i))
    assert by_rows == by_strs
    # strings that tie over all 63 bytes (they differ in trailing zeros alone) are in the list,
    # and the length byte orders them
    padded = {}
    for i, s in enumerate(strs):
        padded.setdefault(rows[i, :63].tobytes(), set()).add(s)
    ties = [v for v in padded.values() if len(v) > 1]
    assert len(ties) > 20 and any(b"pod/web" in v and b"pod/web" + b"\0" * 56 in v for v in ties)
    distinct = sorted(set(strs))
    assert [r.tobytes() for r in pack_str_keys(distinct, 64)] == sorted(r.tobytes() for r in pack_str_keys(distinct, 64))
    assert pack_str_keys(["é" * 31], 64)[0, 63] == 62
    with pytest.raises(ValueError):
        pack_str_keys([b"x" * 64], 64)
    with pytest.raises(ValueError):
        pack_str_keys(["é" * 32], 64)
    with pytest.raises(ValueError):
        pack_str_keys([b"x"], 128)
    bad = rows[:2].copy()
    bad[1, 63] = 64
    with pytest.raises(ValueError):
        unpack_str_keys(bad)


@pytest.mark.parametrize("msg_tag", [None, 0])
def test_wire_codec(rsos_hip_lib, msg_tag):
    """str63 bounds of 0, 1, 31, 32 and 63 bytes on either side: RH_FORM_VEC round-trips and its
    bytes are the oracle codec's Vec<u8> encoding of the strings; a decoded length of 64 is
    RH_ERR_DATA; RH_FORM_ARRAY is RH_ERR_ARG."""
    import wire as OW  # oracle/wire.py
    from rsos_hip import RecordSchema, wire, _abi as A
    from rsos_hip.fingerprint import Aggregate, Fingerprint
    schema = RecordSchema.dated("str63", "var")
    ks = [b"", b"k", bytes(range(1, 32)), b"ns/kube-system/ReplicaSet/core-dns"[:32].ljust(32, b"-"), bytes(range(100, 163))]
    assert [len(k) for k in ks] == [0, 1, 31, 32, 63]
    rng = np.random.default_rng(3)
    items, want = [], b""
    enc, _ = OW.key_codec("vec")
    for i, (s, e) in enumerate([(None, None)] + [(a, b) for a in ks + [None] for b in ks + [None]]):
        limbs = tuple(int(x) for x in rng.integers(0, 1 << 63, 4))
        items.append(wire.RangeAggregate(s, e, Aggregate(i * 300, Fingerprint(limbs))))
        want += OW.encode_range_aggregate(OW.RangeAggregate(s, e, limbs, i * 300), enc, msg_tag)
    data = wire.encode(schema, items, key_form="vec", msg_tag=msg_tag)
    assert data == want
    back, used = wire.decode_stream(schema, data, len(items), key_form="vec", msg_tag=msg_tag)
    assert back == items and used == len(data)
    for s, e in ((b"x" * 64, None), (None, b"y" * 64), (b"z" * 200, b"z")):
        blob = OW.encode_range_aggregate(OW.RangeAggregate(s, e, (1, 2, 3, 4), 5), enc, msg_tag)
        with pytest.raises(A.RsosHipError) as err:
            wire.decode_stream(schema, blob, 4, key_form="vec", msg_tag=msg_tag)
        assert err.value.code == A.ERR_DATA
    for call in (lambda: wire.encode(schema, items, key_form="array", msg_tag=msg_tag),
                 lambda: wire.decode_stream(schema, data, 4, key_form="array", msg_tag=msg_tag)):
        with pytest.raises(A.RsosHipError) as err:
            call()
        assert err.value.code == A.ERR_ARG


@pytest.mark.parametrize("tags", [True, False], ids=["tags", "untagged"])
@pytest.mark.parametrize("kind", KINDS)
def test_generated_inputs_cover_the_cases(rsos_hip_lib, kind, tags):
    """The lift test's inputs themselves (a condition on the generator, no GPU)."""
    from rsos_hip import unpack_str_keys
    c = lift_case(kind, tags)
    n, TL = c["n"], tail_len(kind)
    assert n == N_LIFT == 600 and n == 2 * 256 + 88
    assert c["offsets"][0] == 0 and int(c["offsets"][n]) == len(c["heap"])
    assert all(int(c["offsets"][i + 1] - c["offsets"][i]) == c["lens"][i] for i in range(n))
    assert unpack_str_keys(c["keys"]) == c["strs"] and c["keys"].shape == (n, 64)
    present = [i for i in range(n) if not c["tomb"][i]]
    L = lambda i: len(c["strs"][i])  # noqa: E731
    plen = lambda i: prefix_len(kind, L(i))  # noqa: E731
    # every key length (all four byte alignments, every word shift 0..15), the block edge and past it
    assert {L(i) for i in present} == set(range(64))
    assert {(L(i) & 3, L(i) >> 2) for i in present} == {(a, q) for a in range(4) for q in range(16)}
    assert {56, 57, 58, 59, 60, 61, 62, 63} <= {L(i) for i in present if c["lens"][i] > 0}
    # every alignment of a value's start against every alignment of the prefix's end
    assert {(int(c["offsets"][i]) % 4, L(i) % 4) for i in present if c["lens"][i]} == \
        {(a, b) for a in range(4) for b in range(4)}
    # prefixes: every length from the empty key's to the longest; below, at and past the block edge
    assert {plen(i) for i in present} == set(range(8 + TL, 8 + 63 + TL + 1))
    assert 8 + TL < 64 < 8 + 63 + TL and 8 + 63 + TL == {"plain": 79, "projection": 83, "dated": 103}[kind]
    for lo, hi in ((0, 63), (64, 64), (65, 200)):
        rows = [i for i in present if lo <= plen(i) <= hi]
        # with no value, a value that ends inside the prefix's last block, and one that goes on past it
        assert any(c["lens"][i] == 0 for i in rows), (lo, hi)
        assert any(0 < c["lens"][i] and plen(i) % 64 + c["lens"][i] < 64 for i in rows), (lo, hi)
        assert any(plen(i) % 64 + c["lens"][i] > 64 for i in rows), (lo, hi)
    # the tail words straddle the edge (the key ends in block 0, the prefix in block 1), and the
    # key itself does (8 + L > 64)
    assert any(8 + L(i) < 64 < plen(i) for i in present) and any(8 + L(i) > 64 for i in present)
    totals = [len(c["blobs"][i]) for i in present]
    assert all(totals.count(t) >= 2 for t in TOTALS)
    assert all(len(c["blobs"][i]) == plen(i) + int(c["lens"][i]) for i in present)
    assert all(any(c["lens"][i] == s for i in present) for s in range(9))
    if c["tags"] is not None:
        tombs = [i for i in range(n) if c["tomb"][i]]
        assert all(c["tomb"][i] == (i % 5 == 4) for i in range(n))
        assert c["lens"][9] > 0 and c["tomb"][9] and all(c["lens"][i] == 0 for i in tombs if i != 9)
        assert all(len(c["blobs"][i]) == plen(i) - 8 for i in tombs)
        assert {L(i) for i in tombs} == set(range(64))
        tl = {len(c["blobs"][i]) for i in tombs}
        assert min(tl) < 64 and 64 in tl and max(tl) == 8 + 63 + TL - 8 > 64  # two-block tombstones
    else:
        assert not c["tomb"].any()
    last = present[-1]
    assert last >= n - 2 and c["lens"][last] > 0 and int(c["offsets"][last + 1]) == len(c["heap"])


# ---- GPU: the lift ---------------------------------------------------------------------------------

def check_lift(gpu, kind, tags, lead, slack, keys=None, want=None):
    case = lift_case(kind, tags)
    assert (case["n"] + 255) // 256 == 3
    RC.check_var_lift(gpu, schema_of(kind), case, lift_want(kind, tags) if want is None else want, lead, slack, keys=keys,
                      tell=("key lengths", "message lengths", "tombstones"))


@pytest.mark.gpu
@pytest.mark.parametrize("tight", [False, True], ids=["slack", "tight"])
@pytest.mark.parametrize("kind,tags", [("plain", False), ("dated", True), ("dated", False), ("projection", True),
                                       ("projection", False)],
                         ids=["plain", "dated-tags", "dated-untagged", "projection-tags", "projection-untagged"])
def test_lift_parity(gpu, oracle_lib, kind, tags, tight):
    """Every row's fingerprint and every 256-row block sum equal the oracle's: once with filler
    before and after the values, once with the first value at heap offset 0 and bytes_len =
    round_up(offsets[n], 4)."""
    check_lift(gpu, kind, tags, 0 if tight else 5, 0 if tight else 64)


@pytest.mark.gpu
@pytest.mark.parametrize("tight", [False, True], ids=["slack", "tight"])
def test_padding_and_length_byte_are_not_hashed(gpu, oracle_lib, tight):
    """Device key rows with 0xA5 in their padding, and rows whose length byte is 64..255 (caller
    errors): the fingerprints are those of the masked key -- the row's bytes below the length,
    the length clipped to 63 -- as the header states."""
    import oracle as O
    case, want = lift_case("dated"), lift_want("dated").copy()
    rng = np.random.default_rng(77)
    keys = case["keys"].copy()
    clipped = [i for i in range(case["n"]) if i % 7 == 3]
    blobs = []
    for i, s in enumerate(case["strs"]):
        keys[i, len(s):63] = 0xA5
        if i % 7 == 3:  # 63 bytes of anything under a length byte no row can hold
            keys[i, :63] = rng.integers(0, 256, 63, dtype=np.uint8)
            keys[i, 63] = {3: 64, 10: 255}.get(i, 64 + (i * 37) % 192)
            blobs.append(RC.canonical("str63", "var", "dated", keys[i, :63].tobytes(), case_value(case, i),
                                      (int(case["phys"][i]), int(case["logical"][i]), int(case["node"][i])),
                                      bool(case["tomb"][i])))
    assert {int(keys[i, 63]) for i in clipped} >= {64, 255} and any(case["tomb"][i] for i in clipped)
    want[clipped] = O.lift_encoded(blobs, threads=4)
    assert (keys != case["keys"]).any(axis=1).sum() >= case["n"] - 10
    check_lift(gpu, "dated", True, 0 if tight else 5, 0 if tight else 64, keys=keys, want=want)


@pytest.mark.gpu
def test_dual_lift_equals_the_two_single_lifts(gpu, oracle_lib):
    import oracle as O
    from rsos_hip import lift_dual, lift_records
    case = lift_case("dated")
    schema = schema_of("dated")
    cols = RC.device_cols(case, schema, gpu, 5, 64)
    fd, bd, fp, bp = lift_dual(schema, cols)
    f1, b1 = lift_records(schema, cols)
    f2, b2 = lift_records(schema_of("projection"), {k: v for k, v in cols.items() if k not in ("phys", "logical", "node")})
    for a, b in ((fd, f1), (bd, b1), (fp, f2), (bp, b2)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(f1.cpu().numpy(), lift_want("dated"))
    blobs = [RC.canonical("str63", "var", "projection", case["strs"][i], case_value(case, i), tomb=bool(case["tomb"][i]))
             for i in range(case["n"])]
    assert np.array_equal(fp.cpu().numpy(), O.lift_encoded(blobs, threads=4))


# ---- GPU: the store against a model ----------------------------------------------------------------

PREFIX56 = b"production-eu-west-1/ReplicaSet/frontend-web-7c9d8b6f54-" .ljust(56, b"x")
assert len(PREFIX56) == 56


def deep_family(rng, n):
    """n distinct strings that share their first 56 bytes (so the leading seven of a row's eight
    8-byte sort digits) and differ only in bytes 56..62."""
    out = set()
    while len(out) < n:
        out.add(PREFIX56 + rng.integers(0, 256, int(rng.integers(1, 8)), dtype=np.uint8).tobytes())
    return sorted(out)


def zero_family():
    """Strings that differ only in trailing zero bytes: rows equal over all 63 bytes, ordered by
    the length byte alone."""
    return [b"pod/web" + b"\0" * k for k in range(57)] + [b"\0" * k for k in range(64)]


def string_pool(rng, n):
    """n distinct strings of 0..63 bytes: object names of 40-60 bytes, random bytes."""
    pool = set()
    i = 0
    while len(pool) < n:
        if i % 2:
            pool.add(b"ns-%d/Deployment/%s-%s" % (i % 17, b"svc" * int(rng.integers(1, 9)), b"%010x" % int(rng.integers(0, 1 << 40))))
        else:
            pool.add(rng.integers(0, 256, int(rng.integers(0, 64)), dtype=np.uint8).tobytes())
        i += 1
    assert max(len(s) for s in pool) <= 63
    return list(pool)


def check_questions(st, m):
    """ranks, selects and key dumps of 1 .. 200 questions (the one-launch query holds 64 keys of at
    most 32 bytes) and key-range aggregates over every pair of bound kinds."""
    from rsos_hip import pack_str_keys, _abi as A
    from rsos_hip.store import _np_ptr
    ks = sorted(m.rows)
    n = len(ks)
    fps = [m.rows[k][1] for k in ks]
    rng = np.random.default_rng(n)
    for q in QUESTIONS:
        asked = [ks[int(i)] for i in rng.integers(0, n, q - q // 3)]
        asked += [k[:-1] + b"\x01" if k else b"\x01" for k in asked[:q // 3]]  # mostly absent ones
        assert len(asked) == q
        got = st.ranks(pack_str_keys(asked, 64))
        assert got.tolist() == [bisect.bisect_left(ks, k) for k in asked], q
        lo = int(rng.integers(0, n - q))
        buf = np.zeros(q * 64, np.uint8)
        A.check(st._f("keys")(st._h, lo, lo + q, _np_ptr(buf)), "rh_store_keys")
        assert buf.tobytes() == pack_str_keys(ks[lo:lo + q], 64).tobytes(), q
        for r in {0, q - 1, n - q, n - 1}:
            assert st.select(r) == ks[r]
    probes = [ks[i] for i in range(0, n, n // 7)] + [PREFIX56 + b"\x80", b"pod/web" + b"\0" * 20, b"pod/web\0\x01"]
    RC.check_key_ranges(st, ks, fps, ((lk, hk, *sorted((probes[(i * 3) % len(probes)], probes[(i * 5 + 4) % len(probes)])))
                                      for i, (lk, hk) in enumerate((a, b) for a in BOUND_KINDS for b in BOUND_KINDS)))


@pytest.mark.gpu
@pytest.mark.parametrize("tier", [False, True], ids=["device", "tier"])
def test_store_against_model(gpu, oracle_lib, tier):
    """load; a host batch of new keys, overwrites and deletes in which 2,500 keys share their first
    56 bytes (more than one sort bucket holds: the batch is ordered by the radix sort over all
    eight digits); staged rows; a device batch; queued device batches; a compaction -- after each
    the store answers as a dict model lifted by the oracle does.  Malformed host key rows are
    RH_ERR_ARG naming the row, and change nothing."""
    import torch
    from rsos_hip import GpuFingerprintStore, RecordSchema, _abi as A
    rng = np.random.default_rng(63)
    deep = deep_family(rng, 3000)
    rng.shuffle(deep)
    zeros = zero_family()
    pool = [s for s in string_pool(rng, 2200) if s not in set(zeros)]
    base = sorted(zeros[::2] + deep[:300] + pool[:1200])
    fresh = pool[1200:]
    absent = fresh[900:920] + [PREFIX56, PREFIX56 + b"\0", b"pod/web\0\x01", b"pod/wea" + b"\xff" * 56, b"\xff" * 63]
    schema = RecordSchema.dated("str63", "var")
    st, m = GpuFingerprintStore(schema, host_tier=tier), DictModel("str63", "var")
    recs = ragged_records(rng, base, long_every=150)
    st.load_bulk(m.cols(recs))
    m.apply(recs, [0] * len(recs))
    m.check(st, absent)
    check_questions(st, m)
    assert max(len(r[3]) for r in recs) == 5000 and max(len(k) for k in base) == 63

    # a host batch: 2,500 new keys of the deep family, the other trailing-zero strings, overwrites
    # and deletes of loaded keys (deep ones among them), shuffled
    ow = [base[i] for i in rng.choice(len(base), 300, replace=False)]
    new = deep[300:2800] + zeros[1::2] + fresh[:100]
    batch = ragged_records(rng, new + ow[:150], long_every=400) + [(k, (0, 0, 0), 0, b"") for k in ow[150:]]
    ops = [0] * (len(new) + 150) + [1] * 150
    perm = rng.permutation(len(batch))
    batch, ops = [batch[i] for i in perm], [ops[i] for i in perm]
    assert st.apply(m.cols(batch), np.array(ops, np.uint8)) == (len(new), 150, 150)
    m.apply(batch, ops)
    m.check(st, absent)
    check_questions(st, m)
    root = agg_int(st.aggregate())
    k_ins = sum(1 for op in ops if op == 0)
    assert st.apply(m.cols(batch), np.array(ops, np.uint8)) == (0, k_ins, 0)  # delivered again
    assert (st.size(), agg_int(st.aggregate())) == (len(m.rows), root)

    again = fresh[100]
    staged = ragged_records(rng, [again] + fresh[101:125] + [again] + ow[:23] + [again], long_every=25)
    sops = [0] * 50
    for j in (5, 30, 31):
        sops[j] = 1
    for lo, hi in ((0, 20), (20, 35), (35, 50)):
        st.stage(m.cols(staged[lo:hi]), np.array(sops[lo:hi], np.uint8))
    m.apply(staged, sops)
    m.check(st, absent)  # the first question flushes
    assert m.rows[again][0][3] == staged[-1][3]

    dev = ragged_records(rng, fresh[200:264] + deep[2800:2900] + ow[40:104], long_every=16)
    dops = np.zeros(len(dev), np.uint8)
    dops[70:80] = 1  # deletes of keys the store does not hold
    n_new = 64 + 100 - 10
    assert st.apply_device(to_device(m.cols(dev), gpu), torch.from_numpy(dops).to(gpu)) == (n_new, 64, 0)
    m.apply(dev, dops.tolist())
    m.check(st, absent)

    q1 = ragged_records(rng, fresh[300:400] + deep[2900:2950], long_every=30)
    q2 = ragged_records(rng, fresh[380:480] + deep[2940:3000] + ow[150:170], long_every=30)  # overlaps q1, re-inserts deleted keys
    want2 = (sum(1 for r in q2 if r[0] not in m.rows and r[0] not in {x[0] for x in q1}),
             sum(1 for r in q2 if r[0] in m.rows or r[0] in {x[0] for x in q1}), 0)
    assert st.apply_device_many([to_device(m.cols(q1), gpu), to_device(m.cols(q2), gpu)]) == [(150, 0, 0), want2]
    m.apply(q1, [0] * len(q1))
    m.apply(q2, [0] * len(q2))
    m.check(st, absent)
    check_questions(st, m)

    st.compact()
    m.check(st, absent)
    check_questions(st, m)
    assert st.batch_stats()["small"] == 0

    good = m.cols(ragged_records(rng, fresh[500:510]))
    bads = []
    k = good["keys"].copy()
    k[3, 63] = 64  # a length byte no 64-byte row can hold
    bads.append((3, dict(good, keys=k)))
    k = good["keys"].copy()
    row = next(i for i in range(10) if k[i, 63] < 62)
    k[row, 62] = 1  # nonzero padding
    bads.append((row, dict(good, keys=k)))
    for row, bad in bads:
        for call in (lambda: st.apply(bad, np.zeros(10, np.uint8)), lambda: st.stage(bad, np.zeros(10, np.uint8)),
                     lambda: st.load_bulk(bad)):
            with pytest.raises(A.RsosHipError) as e:
                call()
            assert e.value.code == A.ERR_ARG and "RH_KEY_STR" in str(e.value) and f"row {row} " in str(e.value)
    m.check(st, absent)
    st.close()


# ---- GPU: reconciliation ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def recon_sides():
    """Two replicas of 3,000 rows that differ in 10 keys: two changed values, keys only a holds
    (b's deletes) and keys only b holds (b's inserts) -- among them a 62-byte string and its
    one-byte extensions, and two deep-family keys that differ in byte 62 alone."""
    rng = np.random.default_rng(29)
    deep = deep_family(rng, 800)
    pool = sorted(set(string_pool(rng, 2300)) | set(deep) | set(zero_family()[:40]))
    stem = b"default/Pod/" + b"q" * 50
    d7 = PREFIX56 + b"abcdef"
    special = {stem, stem + b"\0", stem + b"z", d7 + b"0", d7 + b"1"}
    pool = [s for s in pool if s not in special]
    rng.shuffle(pool)
    shared = [(k, s, 0, v) for k, s, _, v in ragged_records(rng, sorted(pool[:2996]), long_every=300)]
    a_recs, b_recs = list(shared), list(shared)
    for j, extra in ((321, b"\0"), (2222, b"changed")):
        ch = shared[j]
        b_recs[j] = (ch[0], ch[1], 0, ch[3] + extra)
    only_a = [stem, d7 + b"0", pool[2996], pool[2997]]
    only_b = [stem + b"\0", stem + b"z", d7 + b"1", pool[2998]]
    a_recs += [(k, (5, 5, 5), 0, b"only a") for k in only_a]
    b_recs += [(k, (5, 5, 5), 0, b"only b") for k in only_b]
    want = {shared[321][0], shared[2222][0], *only_a, *only_b}
    assert len(want) == 10 and len(a_recs) == len(b_recs) == 3000
    models = []
    for recs in (a_recs, b_recs):
        recs.sort(key=lambda r: r[0])
        m = DictModel("str63", "var")
        m.apply(recs, [0] * len(recs))
        models.append((recs, m))
    return models, want


@pytest.mark.gpu
@pytest.mark.parametrize("tier", [False, True], ids=["device", "tier"])
@pytest.mark.parametrize("policy", ["fixed16", "sqrt"])
def test_reconciliation_matches_the_literal_driver(gpu, oracle_lib, policy, tier):
    """rsos_hip.rbsr's rounds between two str63 stores equal oracle/rbsr.py's literal driver over
    the same rows round by round -- rounds of at most 16 segments and rounds of more -- and the
    enumerated ranges hold exactly the differing keys."""
    import rbsr as OR  # oracle/rbsr.py
    from rsos_hip import GpuFingerprintStore, RecordSchema, rbsr as R, wire
    (ra, ma), (rb, mb) = recon_sides()[0]
    want_keys = recon_sides()[1]
    schema = RecordSchema.dated("str63", "var")
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
    # segments entering each round: 1, then the previous round's children
    seg = [1] + [len(ch) for ch, _, _ in want_log[:-1]]
    assert min(seg) <= 16 < max(seg) and sum(1 for s in seg if 0 < s <= 16) >= 1

    def inside(key):
        return any((s is None or key >= s) and (e is None or key < e) for s, e in ranges)
    fa = {k: v[1] for k, v in ma.rows.items()}
    fb = {k: v[1] for k, v in mb.rows.items()}
    assert {k for k in set(fa) | set(fb) if inside(k) and fa.get(k) != fb.get(k)} == want_keys
    assert all(fa.get(k) == fb.get(k) for k in set(fa) | set(fb) if not inside(k))
    # the same rounds in SoA form, each round's children through the wire codec (Vec<u8> keys)
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
    fm = FingerprintMap(RecordSchema.dated("str63", "var"))
    model = {}

    def put(k, v, stamp, tomb=False):
        old = fm.insert(k, Entry("" if tomb else v, *stamp, tombstone=tomb))
        assert (old is None) == (k not in model) and (old is None or old.value == model[k][0])
        model[k] = ("" if tomb else v, stamp, tomb)
    rs = "kube-system/ReplicaSet/coredns-autoscaler-5d4b7c9f8d-"
    assert len(rs) == 53
    put(rs + "x7k2p", "Running", (10, 0, 1))            # 58 bytes: the key ends in block 1
    put(rs + "x7k2q", "Pending", (11, 0, 1))
    put(rs, "", (12, 1, 2))
    put("", "the empty key", (13, 0, 2))
    put("näme/" + "ö" * 20, "ü" * 700, (14, 0, 3))      # UTF-8 key bytes; a value of more than one chunk
    put("x" * 63, "longest key", (15, 0, 3))
    put(rs + "x7k2q", "Running, after a restart", (16, 0, 1))
    put(rs + "x7k2p", None, (17, 0, 1), tomb=True)      # a tombstone of 58 + 32 = 90 bytes: two blocks
    assert fm.delete(rs).value == "" and fm.delete(rs) is None and fm.delete("nope") is None
    del model[rs]
    with pytest.raises(ValueError):
        fm.insert("y" * 64, Entry("too long a key", 1, 1, 1))
    assert fm.size() == len(model) == 5
    assert fm.get(rs + "x7k2q").value == "Running, after a restart" and fm.get(rs) is None

    def fp(k):
        v, stamp, tomb = model[k]
        return O.lift_encoded([RC.canonical("str63", "var", "dated", k.encode(), v.encode(), stamp, tomb)])[0].tobytes()
    order = sorted(model, key=str.encode)
    agg = fm.aggregate()
    assert (agg.size, agg_int(agg)) == (len(model), fold(fp(k) for k in order))
    assert [k for k, _ in fm.enumerate()] == order
    assert [k for k, _ in fm.store.enumerate()] == [k.encode() for k in order]
    part = fm.aggregate(KeyRange(rs, rs + "~"))
    inside = [k for k in order if rs <= k < rs + "~"]
    assert len(inside) == 2 and (part.size, agg_int(part)) == (2, fold(fp(k) for k in inside))
    assert fm.rank(rs + "x7k2q") == order.index(rs + "x7k2q") == fm.store.rank(rs + "x7k2q")
    assert fm.store.select(0) == b"" and fm.store.select(4) == b"x" * 63
    fm.close()
