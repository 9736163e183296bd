"""A whole reconciliation whose IDLISTs come from the batched Enumerate: two 50,000-row u32 -> u32
stores that differ in 40 rows (15 keys only on each side, 10 changed values) are driven to completion
with FixedFanOut(16) through rh_store_protocol_round (rsos_hip.rbsr.protocol_round_segments, the
round's raw output handed to the peer), and every round's enumeration ranges are answered by
rsos_hip.rbsr.enumerate_ranges on the round's own `enumerations`.  The per-round key lists equal those
of oracle/rbsr.py's literal driver over the oracle's FingerprintTreeMap of the same records, whose
enumeration is a slice of its sorted keys (Rsos::enumerate, rsos_trait.rs:73-83); their union holds
the symmetric difference."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, ONLY, CHANGED = 50_000, 15, 10


def _records(O, k, v):
    order = np.argsort(k)
    k, v = np.ascontiguousarray(k[order]), np.ascontiguousarray(v[order])
    cols = {"keys": k.view(np.uint8).reshape(-1, 4), "values": v.view(np.uint8).reshape(-1, 4)}
    return k, cols, O.Records(O.Schema(O.KEY_U32, 4, O.VAL_U32, 4, O.REC_PLAIN, 0), cols["keys"], cols["values"])


@pytest.mark.parametrize("tier", [False, True])
def test_drive_with_batched_enumerate(gpu, oracle_lib, tier):
    import rbsr as OR  # oracle/rbsr.py
    from rsos_hip import GpuFingerprintStore, RecordSchema
    from rsos_hip import rbsr as R
    O = oracle_lib
    rng = np.random.default_rng(77)
    pool = rng.choice(1 << 31, N + ONLY, replace=False).astype(np.uint32)
    common, only_a, only_b = pool[:N - ONLY], pool[N - ONLY:N], pool[N:]
    val = rng.integers(0, 1 << 32, N + ONLY, dtype=np.uint32)
    changed = common[:: len(common) // CHANGED][:CHANGED]
    ka, va = np.concatenate([common, only_a]), np.concatenate([val[:N - ONLY], val[N - ONLY:N]])
    kb, vb = np.concatenate([common, only_b]), np.concatenate([val[:N - ONLY], val[N:]])
    vb[np.isin(kb, changed)] ^= np.uint32(0x5A5A)
    sch = RecordSchema.plain("u32", "u32")
    sa, sb = GpuFingerprintStore(sch, host_tier=tier), GpuFingerprintStore(sch, host_tier=tier)
    try:
        sides, views = [], []
        for st, k, v in ((sa, ka, va), (sb, kb, vb)):
            ks, cols, recs = _records(O, k, v)
            st.load_bulk(cols)
            t = O.FingerprintTreeMap(recs)
            t.fill(0, recs.n)
            sides.append(st), views.append((OR.FtmView(t, True), ks))
        assert sa.size() == sb.size() == N

        # the oracle's drive: a's root at b, then ping-pong; each enumeration = a slice of sorted keys
        want, active = [], OR.initial_ranges(views[0][0])
        for k in range(64):
            view, ks = views[(k + 1) % 2]
            ch, en = [], []
            OR.protocol_round(view, OR.fixed_fan_out(16), active, ch, en)
            want.append([ks[(0 if s is None else np.searchsorted(ks, s)):(len(ks) if e is None else np.searchsorted(ks, e))].tolist()
                         for s, e in en])
            active = ch
            if not active:
                break
        assert not active

        # the product's: every round's raw output to the peer, its enumerations to enumerate_ranges
        got, active = [], R.initial_segments(sa)
        for k in range(64):
            st = sides[(k + 1) % 2]
            ch, en, oc = R.protocol_round_segments(st, R.FixedFanOut(16), active, raw=True)
            assert len(en) == oc.enumerated
            got.append(R.enumerate_ranges(st, en))
            active = ch  # (still valid: the enumerate call leaves the round's children alone)
            if not len(active):
                break
        assert got == want
        assert sum(len(r) for r in got) >= 20  # rounds with IDLISTs of their own
        listed = {x for r in got for keys in r for x in keys}
        assert set(only_a.tolist()) | set(only_b.tolist()) | set(changed.tolist()) <= listed
    finally:
        sa.close(), sb.close()
