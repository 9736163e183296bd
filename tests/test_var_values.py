"""Variable-length values in the column store (RH_VAL_VARBYTES): a fixed-width key with a
`String` / `Vec<u8>` value whose length differs per record -- the shape of the reference's own
golden vectors, lift(&50u64, &"Hello") (rsos/src/fingerprint/tests.rs:68-93).

Expected fingerprints come from the oracle alone: every record's canonical bytes are built by
tests/records_common.py with oracle/pyref.py's typed model and hashed by the C oracle
(oracle.lift_encoded) -- never by the product's encoder or a second GPU kernel.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import records_common as RC
from records_common import KINDS, DictModel, agg_int, case_value, fold, prefix_len, ragged_records, to_device

# total message lengths (prefix + value) every shape is run at: block and chunk boundaries on
# either side, two, three and four chunks (the CV stack merges at 2 and 4), an odd tail
TOTALS = (63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 4095, 4096, 4097, 5000)
SMALL = (0, 1, 2, 3, 4, 5, 7, 8)
KEYS = ("u32", "u64", "bytes16", "bytes32")
SHAPES = [(k, r) for k in KEYS for r in KINDS] + [("unit", "plain")]
N_LIFT = 777  # three whole 256-row blocks + a 9-row tail; more than one wave's 256-record range


def schema_of(key, kind):
    from rsos_hip import RecordSchema
    return getattr(RecordSchema, kind)(key, "var")


@functools.lru_cache(maxsize=None)
def lift_case(key, kind, tags=True):
    """777 records of one shape (records_common.build_lift_case).  Present rows carry every
    reachable TOTALS length (len = T - P; a total below P cannot occur) and the SMALL lengths; the
    last record is present."""
    p = prefix_len(key, kind)
    case = RC.build_lift_case(key, "var", kind, tags, N_LIFT, sum((key + kind).encode()) * 1000 + p + int(tags),
                              totals=TOTALS, small=SMALL)
    assert not case["tomb"][N_LIFT - 1]
    return case


@functools.lru_cache(maxsize=None)
def lift_want(key, kind, tags=True):
    import oracle as O
    return O.lift_encoded(lift_case(key, kind, tags)["blobs"], threads=4)


# ---- CPU ------------------------------------------------------------------------------------------

def test_schema_helpers(rsos_hip_lib):
    from rsos_hip import RecordSchema, _abi as A
    assert RecordSchema.plain("u64", "var").supported()
    assert not RecordSchema.plain("bytes12", "var").supported()
    for key in ("unit", "u32", "u64", "bytes16", "bytes32"):
        assert RecordSchema.dated(key, "var").supported()
    want = {("u32", "plain"): 12, ("u64", "plain"): 16, ("bytes16", "dated"): 56, ("bytes32", "projection"): 52,
            ("bytes32", "dated"): 72}
    for (key, kind), p in want.items():
        assert schema_of(key, kind).record_len() == p == prefix_len(key, kind)
    assert RecordSchema.dated("bytes32", "var").record_len(True) == 64  # exactly one block
    assert RecordSchema.dated("bytes16", "var").record_len(True) == 48
    bad = A.Schema(A.KEY_U64, 8, A.VAL_VARBYTES, 5, A.REC_PLAIN, 0)
    assert A.lib().rh_schema_supported(C.byref(bad)) == A.ERR_ARG
    assert A.lib().rh_schema_record_len(C.byref(bad), 0) == A.ERR_ARG
    assert b"value_len 0" in A.lib().rh_last_error()
    with pytest.raises(ValueError):
        RecordSchema.plain("var", "u64")


def test_unsupported_entry_points_refuse_without_a_device(rsos_hip_lib):
    """rh_sstore_create refuses VARBYTES before any device call, naming the kind."""
    from rsos_hip import _abi as A
    s = A.Schema(A.KEY_U64, 8, A.VAL_VARBYTES, 0, A.REC_DATED, 0)
    h, devs = C.c_void_p(), (C.c_int * 2)(0, 0)
    assert A.lib().rh_sstore_create(devs, 2, C.byref(s), C.byref(h)) == A.ERR_UNSUPPORTED
    assert b"VARBYTES" in A.lib().rh_last_error()
    assert not h.value


@pytest.mark.parametrize("key,kind", SHAPES)
def test_generated_inputs_cover_the_cases(key, kind):
    """The lift test's inputs themselves: values packed back to back, all four start alignments
    and every reachable target total among the present rows, the tombstone pattern."""
    c = lift_case(key, kind)
    n, p = c["n"], c["p"]
    assert n == N_LIFT and c["offsets"][0] == 0 and int(c["offsets"][n]) == len(c["heap"])
    assert all(int(c["offsets"][i + 1] - c["offsets"][i]) == c["lens"][i] for i in range(n))
    present = [i for i in range(n) if not c["tomb"][i]]
    assert {int(c["offsets"][i]) % 4 for i in present if c["lens"][i]} == {0, 1, 2, 3}
    totals = {p + int(c["lens"][i]) for i in present}
    assert all(t in totals for t in TOTALS if t >= p)
    assert [t for t in TOTALS if t < p] == ([63, 64, 65] if p == 72 else [])  # below the prefix: unreachable
    assert all(p + s in totals for s in SMALL)
    assert all(len(c["blobs"][i]) == p + int(c["lens"][i]) for i in present)
    if kind != "plain":
        assert all(c["tomb"][i] == (i % 5 == 4) for i in range(n))
        assert c["lens"][9] > 0 and c["tomb"][9]
        assert all(len(c["blobs"][i]) == p - 8 for i in range(n) if c["tomb"][i])
    assert not c["tomb"][n - 1] and c["lens"][n - 1] > 0


def test_fmap_rows_accept_any_length(rsos_hip_lib):
    from rsos_hip import RecordSchema
    from rsos_hip.fmap import Entry, encode_row
    s = RecordSchema.dated("u64", "var")
    for v in (b"", b"a", bytes(5000)):
        assert encode_row(s, Entry(v, 1, 2, 3))[0] == v
    assert encode_row(s, Entry("héllo", 1, 2, 3))[0] == "héllo".encode()
    assert encode_row(s, Entry(b"", 1, 2, 3, tombstone=True)) == (b"", 1, 2, 3, 1)
    with pytest.raises(ValueError):
        encode_row(s, Entry(b"x", 1, 2, 3, tombstone=True))
    with pytest.raises(ValueError):
        encode_row(s, Entry(7, 1, 2, 3))


# ---- GPU: the lift ---------------------------------------------------------------------------------

def check_lift(gpu, key, kind, tags, lead, slack):
    RC.check_var_lift(gpu, schema_of(key, kind), lift_case(key, kind, tags), lift_want(key, kind, tags), lead, slack)


@pytest.mark.gpu
@pytest.mark.parametrize("tight", [False, True], ids=["slack", "tight"])
@pytest.mark.parametrize("key,kind", SHAPES)
def test_lift_parity(gpu, oracle_lib, key, kind, tight):
    """Every row's fingerprint and every 256-row block sum equal the oracle's: once with filler
    before and after the values, once with the first value at offset 0 and bytes_len =
    round_up(offsets[n], 4)."""
    check_lift(gpu, key, kind, True, 0 if tight else 5, 0 if tight else 64)


@pytest.mark.gpu
def test_lift_parity_without_a_tag_column(gpu, oracle_lib):
    """A dated batch with no tag column: every row present."""
    check_lift(gpu, "bytes16", "dated", False, 0, 0)


@pytest.mark.gpu
def test_reference_goldens(gpu, oracle_lib, golden):
    """lift(&50u64, &"Hello") and the sum over (25, "World!"), (50, "Hello"), (75, "Everyone!")
    (rsos/src/fingerprint/tests.rs:68-93), from a u64 key column and a ragged value heap."""
    import torch
    from rsos_hip import GpuFingerprintStore, RecordSchema, lift_records
    vec = {v["name"]: v for v in golden["reference"]["vectors"]}
    limbs = lambda name: sum(int(h, 16) << (64 * i) for i, h in enumerate(vec[name]["limbs"]))  # noqa: E731
    schema = RecordSchema.plain("u64", "var")
    vals = [b"World!", b"Hello", b"Everyone!"]
    keys = np.array([25, 50, 75], np.uint64)
    offs = np.zeros(4, np.uint64)
    offs[1:] = np.cumsum([len(v) for v in vals])
    heap = np.frombuffer(b"".join(vals), np.uint8)
    pad = np.zeros((heap.size + 3) & ~3, np.uint8)
    pad[:heap.size] = heap
    fps, _ = lift_records(schema, {"keys": torch.from_numpy(keys.view(np.int64)).to(gpu),
                                   "values": torch.from_numpy(pad).to(gpu),
                                   "value_offsets": torch.from_numpy(offs.astype(np.int64)).to(gpu)})
    assert int.from_bytes(fps[1].cpu().numpy().tobytes(), "little") == limbs("lift_50u64_Hello")
    st = GpuFingerprintStore(schema)
    st.load_bulk({"keys": keys, "values": heap, "value_offsets": offs})
    assert st.size() == 3
    root = st.aggregate()
    assert root.size == 3 and agg_int(root) == limbs("combined_25_50_75")
    st.close()


@pytest.mark.gpu
def test_dual_lift_equals_the_two_single_lifts(gpu, oracle_lib):
    from rsos_hip import lift_dual, lift_records
    case = lift_case("bytes16", "dated")
    schema = schema_of("bytes16", "dated")
    cols = RC.device_cols(case, schema, gpu, 5, 64)
    fd, bd, fp, bp = lift_dual(schema, cols)
    f1, b1 = lift_records(schema, cols)
    f2, b2 = lift_records(schema_of("bytes16", "projection"), {k: v for k, v in cols.items()
                                                                if k not in ("phys", "logical", "node")})
    for a, b in ((fd, f1), (bd, b1), (fp, f2), (bp, b2)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(f1.cpu().numpy(), lift_want("bytes16", "dated"))
    # the projection of the same rows, from the oracle
    import oracle as O
    blobs = [RC.canonical("bytes16", "var", "projection", case["keys"][i].tobytes(), case_value(case, i),
                          tomb=bool(case["tomb"][i])) for i in range(case["n"])]
    assert np.array_equal(fp.cpu().numpy(), O.lift_encoded(blobs, threads=4))


# ---- GPU: the store against a model ----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tier", [False, True], ids=["device", "tier"])
def test_store_against_model(gpu, oracle_lib, tier):
    """load, apply (new / overwrite with another length / delete), the same batch again, a staged
    batch with a key staged three times, a device batch, a compaction -- size, root, 16 rank
    ranges, the keys and every fingerprint equal a dict model lifted by the oracle after each;
    bad host offsets are RH_ERR_ARG and change nothing."""
    import torch
    from rsos_hip import GpuFingerprintStore, RecordSchema, _abi as A
    rng = np.random.default_rng(11)
    pool = sorted({rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(1400)})
    rng.shuffle(pool)
    base, fresh = sorted(pool[:1000]), pool[1000:]
    schema = RecordSchema.dated("bytes16", "var")
    st, m = GpuFingerprintStore(schema, host_tier=tier), DictModel("bytes16", "var")
    # the batches go the large-batch way, whatever their size
    recs = ragged_records(rng, base, long_every=90)
    st.load_bulk(m.cols(recs))
    m.apply(recs, [0] * len(recs))
    m.check(st)
    assert max(len(r[3]) for r in recs) == 5000

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
    m.check(st)
    root = agg_int(st.aggregate())
    # delivered again: every insert meets its own record (an overwrite that changes nothing), every
    # delete a key already gone -- counts, size and root say so
    assert st.apply(m.cols(batch), np.array(ops, np.uint8)) == (0, sum(1 for r, op in zip(batch, ops) if op == 0 and r[0] in m.rows), 0)
    assert sum(1 for op in ops if op == 0) == 200
    assert (st.size(), agg_int(st.aggregate())) == (len(m.rows), root)
    m.check(st)
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
    m.check(st)  # the first question flushes
    assert m.rows[again][0][3] == staged[-1][3]

    dev = ragged_records(rng, fresh[200:232] + ow[40:72], long_every=16)
    new, over, dele = st.apply_device(to_device(m.cols(dev), gpu), torch.zeros(64, dtype=torch.uint8, device=gpu))
    assert (new, over, dele) == (32, 32, 0)
    m.apply(dev, [0] * 64)
    m.check(st)

    # two more device batches in one call; the first heap's size is no multiple of 4 and is passed
    # as it is (the binding pads its copy), the second batch deletes some of the first's rows
    many = [ragged_records(rng, fresh[232:264] + ow[72:88], long_every=12), ragged_records(rng, fresh[240:256] + fresh[264:280])]
    if sum(len(r[3]) for r in many[0]) % 4 == 0:
        many[0][0] = (many[0][0][0], many[0][0][1], many[0][0][2], many[0][0][3] + b"x")
    mops = [[0] * 48, [1] * 16 + [0] * 16]
    tcs = [to_device(m.cols(recs), gpu, pad_heap=False) for recs in many]
    assert tcs[0]["values"].numel() % 4 != 0
    got = st.apply_device_many(tcs, [torch.from_numpy(np.array(o, np.uint8)).to(gpu) for o in mops])
    assert got == [(32, 16, 0), (16, 0, 16)]
    for recs, o in zip(many, mops):
        m.apply(recs, o)
    m.check(st)

    st.compact()
    m.check(st)
    with pytest.raises(ValueError, match="value_offsets"):
        st.load_bulk({k: v for k, v in m.cols(many[1]).items() if k not in ("values", "value_offsets")})

    good = m.cols(ragged_records(rng, fresh[300:310]))
    for breakage in ("decrease", "exceed"):
        bad = dict(good)
        offs = good["value_offsets"].copy()
        if breakage == "decrease":
            offs[4], offs[5] = offs[3] + 1, offs[3]
            assert offs[5] < offs[4]
        else:
            offs[-1] = good["values"].size + 1
        bad["value_offsets"] = offs
        for call in (lambda: st.apply(bad, np.zeros(10, np.uint8)), lambda: st.stage(bad, np.zeros(10, np.uint8)),
                     lambda: st.load_bulk(bad)):
            with pytest.raises(A.RsosHipError) as e:
                call()
            assert e.value.code == A.ERR_ARG
    m.check(st)
    st.close()


# ---- GPU: reconciliation ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tier", [False, True], ids=["device", "tier"])
def test_reconciliation_finds_the_differing_keys(gpu, oracle_lib, tier):
    """Two u64-key dated var stores of 2,000 rows that differ in 3 keys, one of them only by a
    trailing zero byte of its value: the one-call device rounds (FixedFanOut 16) enumerate ranges
    whose differing entries are exactly those keys."""
    from rsos_hip import GpuFingerprintStore, RecordSchema, rbsr as R
    rng = np.random.default_rng(23)
    ks = sorted({int(x) for x in rng.integers(0, 1 << 63, 2100)})[:2001]
    kb = [k.to_bytes(8, "little") for k in ks]
    shared = ragged_records(rng, kb[:2000], long_every=300)
    shared = [(k, s, 0, v) for k, s, _, v in shared]
    ia, ib = 321, 1200
    a_recs, b_recs = list(shared), list(shared)
    a_recs[ia] = (kb[ia], shared[ia][1], 0, b"ab")
    b_recs[ia] = (kb[ia], shared[ia][1], 0, b"ab\x00")  # same key and stamp: one trailing byte
    del b_recs[ib]                                         # only a has it
    b_recs.append((kb[2000], (5, 5, 5), 0, b"only b"))     # only b has it (the largest key)
    want = {ks[ia], ks[ib], ks[2000]}
    schema = RecordSchema.dated("u64", "var")
    sides = []
    for recs in (a_recs, b_recs):
        st, m = GpuFingerprintStore(schema, host_tier=tier), DictModel("u64", "var")
        st.load_bulk(m.cols(recs))
        m.apply(recs, [0] * len(recs))
        sides.append((st, m))
    (a, ma), (b, mb) = sides
    assert a.size() == 2000 and b.size() == 2000
    pol = R.FixedFanOut(16)
    active, k, ranges = R.initial_segments(a), 0, []
    while len(active):
        assert k < 64
        side = (b, a)[k % 2]
        active, en, _ = R.protocol_round_segments(side, pol, active)
        ranges += [en.bounds(schema, i) for i in range(en.n)]
        k += 1
    assert ranges

    def inside(key):
        return any((s is None or key >= s) and (e is None or key < e) for s, e in ranges)
    fa = {int.from_bytes(kk, "little"): v[1] for kk, v in ma.rows.items()}
    fb = {int.from_bytes(kk, "little"): v[1] for kk, v in mb.rows.items()}
    found = {key for key in set(fa) | set(fb) if inside(key) and fa.get(key) != fb.get(key)}
    assert found == want
    # ... and little else is enumerated: FixedFanOut(16) lists a range once it spans at most 16 rows
    # on the deciding side (one more where the peer holds an extra key), and a differing key ends in
    # one listed range per side -- at most 3 keys x 2 sides x 17 of the 2,001 keys
    listed = sum(1 for key in set(fa) | set(fb) if inside(key))
    print("keys inside enumerated ranges:", listed, "ranges:", len(ranges))
    assert listed <= 3 * 2 * 17
    assert all(fa.get(key) == fb.get(key) for key in set(fa) | set(fb) if not inside(key))
    a.close()
    b.close()


# ---- GPU: FingerprintMap ---------------------------------------------------------------------------

@pytest.mark.gpu
def test_fingerprint_map_with_string_values(gpu, oracle_lib):
    from rsos_hip import FingerprintMap, RecordSchema
    O = oracle_lib
    fm = FingerprintMap(RecordSchema.plain("u64", "var"))
    model = {}
    for k, v in ((50, b"Hello"), (25, b"World!"), (75, b"Everyone!"), (7, b""), (9, bytes(range(200)) * 9)):
        assert fm.insert(k, v) is None
        model[k] = v
    assert fm.insert(50, b"Hello, a longer value than before") == b"Hello"
    model[50] = b"Hello, a longer value than before"
    assert fm.delete(25) == b"World!" and fm.delete(26) is None
    del model[25]

    def want():
        return fold(O.lift_encoded([RC.canonical("u64", "var", "plain", k.to_bytes(8, "little"), v) for k, v in sorted(model.items())]))
    agg = fm.aggregate()
    assert (agg.size, agg_int(agg)) == (len(model), want())
    assert fm.insert(9, b"short now") == bytes(range(200)) * 9
    model[9] = b"short now"
    agg = fm.aggregate()
    assert (agg.size, agg_int(agg)) == (len(model), want())
    fm.close()
