"""EnumerateBelowThreshold rounds inside the library (rh_store_protocol_round_threshold,
rh_sstore_protocol_round_threshold) against oracle/rbsr.py's literal round with the policy restated
locally (threshold_common.below_threshold): children, enumerations and outcome, in order and exact.
The expected fingerprints are the oracle's (records_common.DictModel)."""
import bisect
import ctypes as C

import numpy as np
import pytest

import rbsr as OR  # oracle/rbsr.py
from records_common import M256, DictModel, fp_int
from recon_common import _norm, _outcome, reconcile
from threshold_common import below_threshold, covered, to_product

T, B = 32, 16
SHAPES = {"u64": ("u64", "u64"), "b16": ("bytes16", "u64"), "str63": ("str63", "u64")}  # str63: 64-byte rows, the general device path


class ModelView:
    """oracle/rbsr.py's view (size / rank / select / aggregate) over a DictModel's rows in the key
    type's order, keys as the Python surface gives them (ints for u64)."""

    def __init__(self, model):
        raw = model.order()
        self.ks = [model.api_key(k) for k in raw]
        self.pre = [0]
        for k in raw:
            self.pre.append((self.pre[-1] + fp_int(model.rows[k][1])) % M256)

    def size(self):
        return len(self.ks)

    def rank(self, k):
        return bisect.bisect_left(self.ks, k)

    def select(self, r):
        return self.ks[r]

    def aggregate(self, start, end):
        lo = 0 if start is None else self.rank(start)
        hi = len(self.ks) if end is None else self.rank(end)
        if hi <= lo:
            return (0, 0, 0, 0), 0
        v = (self.pre[hi] - self.pre[lo]) % M256
        return tuple((v >> (64 * i)) & (2**64 - 1) for i in range(4)), hi - lo


def _records(rng, shape, n, taken=()):
    """n plain records of a shape with distinct keys outside `taken`"""
    key = SHAPES[shape][0]
    seen, out = set(taken), []
    while len(out) < n:
        if key == "u64":
            k = int(rng.integers(0, 1 << 62)).to_bytes(8, "little")
        elif key == "bytes16":
            k = rng.bytes(16)
        else:
            k = bytes(rng.integers(97, 123, int(rng.integers(1, 40)), dtype=np.uint8))
        if k not in seen:
            seen.add(k)
            out.append((k, (0, 0, 0), 0, int(rng.integers(0, 1 << 62))))
    return out


def _sorted(model, recs):
    return sorted(recs, key=lambda r: model.key_order(r[0]))


_CACHE = {}


def _contents(shape, state):
    """(model, what to load, batch records, batch ops) -- built once a module: "base70k", a 70,000-row
    base (past one 65,536-row super-block); "delta", a 5,000-row base and a 300-row batch of inserts,
    overwrites and deletes left in the delta run"""
    if (shape, state) in _CACHE:
        return _CACHE[shape, state]
    rng = np.random.default_rng(17)
    model = DictModel(*SHAPES[shape], kind="plain")
    if state == "base70k":
        base = _sorted(model, _records(rng, shape, 70_000))
        model.apply(base, [0] * len(base))
        out = (model, base, [], [])
    else:
        base = _sorted(model, _records(rng, shape, 5_000))
        model.apply(base, [0] * len(base))
        pick = [base[int(i)] for i in rng.choice(5_000, 160, replace=False)]
        batch = _records(rng, shape, 140, {r[0] for r in base})                       # inserts
        batch += [(r[0], r[1], 0, r[3] ^ 0x5A5A) for r in pick[:90]] + pick[90:]  # overwrites; deletes
        ops = [0] * 230 + [1] * 70
        order = rng.permutation(300)
        batch, ops = [batch[i] for i in order], [ops[i] for i in order]
        model.apply(batch, ops)
        out = (model, base, batch, ops)
    _CACHE[shape, state] = out
    return out


def _fill(st, model, base, batch, ops):
    st.load_bulk(model.cols(base))
    if batch:
        assert tuple(st.apply(model.cols(batch), np.array(ops, np.uint8))) == (140, 90, 70)
    return st


def _store(shape, state, tier=False):
    from rsos_hip import GpuFingerprintStore, RecordSchema
    model, base, batch, ops = _contents(shape, state)
    st = _fill(GpuFingerprintStore(RecordSchema.plain(*SHAPES[shape]), host_tier=tier), model, base, batch, ops)
    assert (st.stats()["delta_rows"] > 0) == bool(batch)  # the batch sits in the delta run
    if tier:
        st.tier_sync()
    return st, ModelView(model)


def _other(fp, size, how):
    """a remote aggregate against local (fp, size): equal, empty, another fingerprint, another size"""
    if how == 0:
        return fp, size
    if how == 1:
        return (0, 0, 0, 0), 0
    if how == 2:
        return (fp[0] ^ 1, fp[1], fp[2], fp[3]), size
    return fp, size + 3  # the same fingerprint with another size: must not skip


def _specials(v, cross=None):
    """The segments every round holds: a skip; a span-0 range against a non-empty remote side (an IDLIST
    bounced back, not a stride-1 split); spans of exactly t and of t + 1; an inverted segment; both
    sides unbounded, and each alone; a span of 1 against a larger remote side; an empty remote side;
    `cross`: a range of 100 rows around this rank (a shard's splitter)."""
    n = v.size()
    seg = lambda a, b, how: (a, b, _other(*v.aggregate(a, b), how))  # noqa: E731
    k = v.select
    out = [seg(k(10), k(90), 0),
           (k(200), k(200), ((1, 2, 3, 4), 5)),
           seg(k(300), k(300 + T), 2), seg(k(400), k(400 + T + 1), 2),
           (k(700), k(600), ((9, 9, 9, 9), 12)),
           seg(None, None, 3), seg(None, k(T - 1), 2), seg(k(n - T - 5), None, 2),
           seg(k(500), k(501), 3), seg(k(800), k(1000), 1), seg(k(1200), k(1200 + 16 * T + 1), 2)]
    if cross is not None:
        out.append(seg(k(cross - 50), k(cross + 50), 2))
    return out


def _segments(v, r, seed, cross=None):
    """r segments in no order: the specials among random ranges of 0 to 200 rows with equal, empty and
    differing remote sides; r = 1: the special `seed` picks"""
    rng = np.random.default_rng(seed)
    n = v.size()
    if r == 1:
        sp = _specials(v, cross)
        return [sp[seed % len(sp)]]
    out = _specials(v, cross)
    while len(out) < r:
        a = int(rng.integers(0, n - 201))
        c = int(rng.integers(0, 201))
        s, e = v.select(a), v.select(a + c)
        out.append((s, e, _other(*v.aggregate(s, e), int(rng.integers(0, 4)))))
    out = out[:r]
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def _round(st, active, t=T, b=B):
    """one native round: (children, enumerations, outcome) in the oracle's forms, and the raw Segments"""
    from rsos_hip import rbsr as R
    ch, en, oc = R.protocol_round_segments(st, R.EnumerateBelowThreshold(t, b), R.Segments.from_items(st.schema, to_product(active)))
    return (_norm(ch.items(st.schema)), [en.bounds(st.schema, i) for i in range(en.n)], _outcome(oc)), (ch, en)


def _want(v, active, t=T, b=B):
    ch, en = [], []
    oc = OR.protocol_round(v, below_threshold(t, b), active, ch, en)
    return ch, en, oc


def _check_round(st, v, active, **kw):
    got, raw = _round(st, active, **kw)
    wc, we, wo = _want(v, active, **kw)
    assert got[2] == wo, (got[2], wo)
    assert got[1] == we
    assert got[0] == wc
    return raw, wo


def _holds_every_kind(outcomes):
    sk, en, sp, ch, dr = (sum(o[i] for o in outcomes) for i in range(5))
    assert sk and en and sp and dr and ch > sp


# ---- the boundary ------------------------------------------------------------------------------------

def test_new_symbols_resolve_and_refuse_null(rsos_hip_lib):
    from rsos_hip import _abi as A
    L = A.lib()
    seg, ch, en, oc = A.Segments(), A.Segments(), A.Segments(), A.RoundOutcome()
    for fn in (L.rh_store_protocol_round_threshold, L.rh_sstore_protocol_round_threshold):
        assert fn(None, 32, 16, C.byref(seg), C.byref(ch), C.byref(en), C.byref(oc)) == A.ERR_ARG
        assert b"NULL" in L.rh_last_error()
    assert L.rh_abi_version() == 1


@pytest.mark.gpu
def test_argument_checks_come_before_any_device_call(gpu):
    """A NULL argument and a bound kind above 1 are RH_ERR_ARG on both entry points; the two-policy
    call keeps refusing any other policy number."""
    from rsos_hip import GpuFingerprintStore, RecordSchema, _abi as A
    from rsos_hip.sharded import ShardedStore
    L = A.lib()
    sch = RecordSchema.plain("u64", "u64")
    one, four = GpuFingerprintStore(sch, host_tier=False), ShardedStore(sch, [0] * 4, host_tier=False)
    try:
        kinds, two, key = np.ones(1, np.uint8), np.full(1, 2, np.uint8), np.zeros(8, np.uint8)
        agg = np.zeros(5, np.uint64)
        ch, en, oc = A.Segments(), A.Segments(), A.RoundOutcome()
        for st, name in ((one, "rh_store_"), (four, "rh_sstore_")):
            fn = getattr(L, name + "protocol_round_threshold")
            ok = A.Segments(kinds.ctypes.data, key.ctypes.data, kinds.ctypes.data, key.ctypes.data, agg.ctypes.data, 1, 1)
            assert fn(st._h, 32, 16, None, C.byref(ch), C.byref(en), C.byref(oc)) == A.ERR_ARG
            assert fn(st._h, 32, 16, C.byref(ok), None, C.byref(en), C.byref(oc)) == A.ERR_ARG
            assert fn(st._h, 32, 16, C.byref(ok), C.byref(ch), None, C.byref(oc)) == A.ERR_ARG
            for bad in (A.Segments(two.ctypes.data, key.ctypes.data, kinds.ctypes.data, key.ctypes.data, agg.ctypes.data, 1, 1),
                        A.Segments(kinds.ctypes.data, key.ctypes.data, two.ctypes.data, key.ctypes.data, agg.ctypes.data, 1, 1),
                        A.Segments(kinds.ctypes.data, None, kinds.ctypes.data, key.ctypes.data, agg.ctypes.data, 1, 1),
                        A.Segments(kinds.ctypes.data, key.ctypes.data, kinds.ctypes.data, key.ctypes.data, None, 1, 1)):
                assert fn(st._h, 32, 16, C.byref(bad), C.byref(ch), C.byref(en), C.byref(oc)) == A.ERR_ARG
            assert getattr(L, name + "protocol_round")(st._h, 2, 16, C.byref(ok), C.byref(ch), C.byref(en), C.byref(oc)) == A.ERR_ARG
            assert b"unknown policy" in L.rh_last_error()
    finally:
        one.close(), four.close()


# ---- one round ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("r", [1, 16, 17, 1024, 1025])
def test_round_on_a_base_past_one_super_block(gpu, shape, r):
    """70,000 rows, base only; r in each of the four dispatch ranges (one launch, k_round_small,
    k_round_plan_scan, the three-launch plan)."""
    st, v = _store(shape, "base70k")
    try:
        outcomes = []
        for seed in (range(11) if r == 1 else (r,)):
            outcomes.append(_check_round(st, v, _segments(v, r, seed))[1])
        _holds_every_kind(outcomes)
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tier", [False, True], ids=["device", "host_tier"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("r", [1, 16, 17, 1024, 1025])
def test_round_over_base_and_delta_run(gpu, shape, r, tier):
    """A 5,000-row base with a 300-row delta run of inserts, overwrites and deletes, read in place;
    with the host tier on, the rounds of up to 128 segments are its own (HostTier::round)."""
    st, v = _store(shape, "delta", tier)
    try:
        outcomes = []
        for seed in (range(11) if r == 1 else (r,)):
            outcomes.append(_check_round(st, v, _segments(v, r, seed))[1])
        _holds_every_kind(outcomes)
        assert st.stats()["delta_rows"] > 0  # no compaction on the way
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["base70k", "delta"])
@pytest.mark.parametrize("shape", ["u64", "b16"])
@pytest.mark.parametrize("r", [1, 16])
def test_round_unfused(gpu, monkeypatch, shape, r, state):
    """RSOS_HIP_ROUND_FUSED=0: the two searches and k_round_small(_view) instead of k_round_tiny."""
    monkeypatch.setenv("RSOS_HIP_ROUND_FUSED", "0")
    st, v = _store(shape, state)
    try:
        outcomes = []
        for seed in (range(11) if r == 1 else (r,)):
            outcomes.append(_check_round(st, v, _segments(v, r, seed))[1])
        _holds_every_kind(outcomes)
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [(0, 0), (1, 2), (2, 3), (31, 16), (33, 16), (1 << 31, 16)], ids=lambda x: "t%d-b%d" % x)
def test_round_parameters(gpu, tb):
    """t = 0 raised to 1 and b < 2 to 2 by the library; t and b around the paper's; a t above every span."""
    st, v = _store("u64", "delta")
    try:
        _check_round(st, v, _segments(v, 40, 5), t=tb[0], b=tb[1])
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["base70k", "delta"])
@pytest.mark.parametrize("shape", ["u64", "b16"])
def test_sharded_round_equals_one_store(gpu, shape, state):
    """The same rounds on a map of 4 shards on device 0, with segments straddling a splitter (and
    every splitter: both sides unbounded): the oracle's round, and one store's bytes."""
    from rsos_hip import RecordSchema
    from rsos_hip.sharded import ShardedStore
    model, base, batch, ops = _contents(shape, state)
    one, v = _store(shape, state)
    four = _fill(ShardedStore(RecordSchema.plain(*SHAPES[shape]), [0] * 4, host_tier=False), model, base, batch, ops)
    try:
        assert all(four.sizes())
        cross = v.rank(four.splitters[1])
        for r in (1, 16, 17, 1024, 1025):
            for seed in ((11,) if r == 1 else (r,)):  # r = 1: the straddling range alone
                active = _segments(v, r, seed, cross)
                (c1, e1), _ = _check_round(one, v, active)
                (c4, e4), _ = _check_round(four, v, active)
                for f in ("start_kinds", "start_keys", "end_kinds", "end_keys", "aggregates"):
                    assert getattr(c1, f)[:c1.n].tobytes() == getattr(c4, f)[:c4.n].tobytes(), f
                for f in ("start_kinds", "start_keys", "end_kinds", "end_keys"):
                    assert getattr(e1, f)[:e1.n].tobytes() == getattr(e4, f)[:e4.n].tobytes(), f
    finally:
        one.close(), four.close()


# ---- whole drives ------------------------------------------------------------------------------------

def _drive(a, b, pol):
    """native rounds, each side under its own policy: (log, a's enumerations, b's enumerations)"""
    from rsos_hip import rbsr as R
    return reconcile(a, b, lambda st, act, ch, en: _outcome(R.protocol_round_with_policy(st, pol[id(st)], act, ch, en)),
                     R.initial_ranges)


@pytest.mark.gpu
@pytest.mark.parametrize("tier", [False, True], ids=["device", "host_tier"])
@pytest.mark.parametrize("mixed", [False, True], ids=["threshold_both", "threshold_vs_fixed"])
@pytest.mark.parametrize("d", [1, 37])
def test_drives(gpu, d, mixed, tier):
    """Two stores that differ in d keys (one-sided on either side, and changed values): every round
    equals the oracle's with the same policy per side; each side's enumerated keys hold every differing
    key it has, and every enumerated range holds a differing key; under EnumerateBelowThreshold on both
    sides the drive takes no more rounds than FixedFanOut(16) on the same pair."""
    from rsos_hip import GpuFingerprintStore, RecordSchema
    from rsos_hip import rbsr as R
    rng = np.random.default_rng(100 + d)
    ma, mb = DictModel(*SHAPES["u64"], kind="plain"), DictModel(*SHAPES["u64"], kind="plain")
    common = _records(rng, "u64", 6_000)
    diff = _records(rng, "u64", d, {r[0] for r in common})
    only_a, only_b, changed = diff[0::3], diff[1::3], diff[2::3]
    ra = _sorted(ma, common + only_a + changed)
    rb = _sorted(mb, common + only_b + [(r[0], r[1], 0, r[3] ^ 1) for r in changed])
    ma.apply(ra, [0] * len(ra)), mb.apply(rb, [0] * len(rb))
    sch = RecordSchema.plain(*SHAPES["u64"])
    a, b = GpuFingerprintStore(sch, host_tier=tier), GpuFingerprintStore(sch, host_tier=tier)
    try:
        a.load_bulk(ma.cols(ra)), b.load_bulk(mb.cols(rb))
        va, vb = ModelView(ma), ModelView(mb)
        ebt, fixed = R.EnumerateBelowThreshold(T, B), R.FixedFanOut(16)
        pol = {id(a): ebt, id(b): fixed if mixed else ebt}
        dec = {id(va): below_threshold(T, B), id(vb): OR.fixed_fan_out(16) if mixed else below_threshold(T, B)}
        log, ea, eb = _drive(a, b, pol)
        want = reconcile(va, vb, lambda v, act, ch, en: OR.protocol_round(v, dec[id(v)], act, ch, en), OR.initial_ranges)
        assert len(log) == len(want[0])
        for (gc, ge, go), (wc, we, wo) in zip(log, want[0]):
            assert go == wo and ge == we and gc == wc
        key = lambda r: int.from_bytes(r[0], "little")  # noqa: E731
        da, db = {key(r) for r in only_a + changed}, {key(r) for r in only_b + changed}
        for st, en, mine in ((a, ea, da), (b, eb, db)):
            listed = {k for ks in R.enumerate_ranges(st, en) for k in ks} if en else set()
            assert mine <= listed
            for rg in en:
                assert any(covered(k, [rg]) for k in da | db), rg
        if not mixed:
            assert len(log) <= len(_drive(a, b, {id(a): fixed, id(b): fixed})[0])
    finally:
        a.close(), b.close()
