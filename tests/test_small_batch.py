"""The store's small-batch path (csrc/small_batch.hpp) against the large-batch path and the oracle.

A batch of up to small_batch_max rows (1,024; 512 for 32-byte keys) is sorted, lifted, searched and
turned into delta records by one workgroup, then merged into the delta run by a second launch --
the path of a replica's network merge (src/replica/dispatch.rs:188-196) and of a staged
Rsos::insert.  Every case runs twice, with the small path on (the default) and off
(RSOS_HIP_SMALL_MAX=0: every batch through the large-batch path), through host batches
(rh_store_apply), device batches (rh_store_apply_device) and staged rows (rh_store_stage, where a key
staged more than once keeps its last operation), across compactions; after every batch the size
and root, and at the end the whole rank order (keys and fingerprints), ranks and selects, equal a
model folded with FingerprintTreeMap's semantics (insert-or-overwrite replaces the element's
fingerprint, remove drops it: rsos/src/fingerprint_tree_map/mutate.rs:23-154) over the oracle's
lifts (oracle/oracle.c)."""
import numpy as np
import pytest

from records_common import ColumnModel, _batch, _gen, _order

SCHEMAS = [("dated", "bytes16", "bytes64", True), ("plain", "u64", "u64", False),
           ("projection", "bytes32", "bytes64", True), ("dated", "u32", "u32", True)]


def _run(O, spec, small_on, monkeypatch, seed=3):
    import torch
    from rsos_hip import GpuFingerprintStore, RecordSchema
    if small_on:
        monkeypatch.delenv("RSOS_HIP_SMALL_MAX", raising=False)
    else:
        monkeypatch.setenv("RSOS_HIP_SMALL_MAX", "0")
    kind, kname, vname, tomb = spec
    sch = getattr(RecordSchema, kind)(kname, vname)
    rng = np.random.default_rng(seed)
    model = ColumnModel(O, sch)
    base = _gen(rng, sch, 6000, tomb)
    _, first = np.unique(base["keys"], axis=0, return_index=True)
    base = {c: v[np.sort(first)] for c, v in base.items()}
    order = sorted(range(len(base["keys"])), key=lambda i: _order(sch, base["keys"][i].tobytes()))
    base = {c: np.ascontiguousarray(v[order]) for c, v in base.items()}
    model.apply(base, np.zeros(len(base["keys"]), np.uint8))
    st = GpuFingerprintStore(sch)
    st.set_compaction(2, 1500)  # compactions every few batches
    st.load_bulk(base)
    sbm = 512 if sch.key_row == 32 else 1024
    sizes = [1, 2, 3, 63, 64, 65, 300, sbm, sbm + 1, 5, 1, 700, 1]
    trace = []
    for bi, m in enumerate(sizes):
        how = ("host", "device", "staged")[bi % 3]
        cols, ops = _batch(rng, sch, model, m, tomb, repeats=how == "staged")
        if how == "host":
            got = st.apply(cols, ops)
        elif how == "device":
            dc = {c: torch.from_numpy(np.ascontiguousarray(v)).cuda() for c, v in cols.items()}
            got = st.apply_device(dc, torch.from_numpy(ops).cuda())
        else:
            st.stage(cols, ops)
            got = None
        want = model.apply(cols, ops)
        if got is not None:
            assert got == want, (how, m)
        root, size = model.root()
        agg = st.aggregate()
        assert agg.size == size == st.size(), (how, m)
        assert agg.fingerprint.to_int() == root, (how, m)
        trace.append((got, agg.size, agg.fingerprint.to_int()))
    # a batch with a repeated key through apply is refused, the store unchanged
    cols, ops = _batch(rng, sch, model, 4, tomb)
    cols = {c: np.concatenate([v, v[:1]]) for c, v in cols.items()}
    ops = np.concatenate([ops, ops[:1]])
    with pytest.raises(Exception):
        st.apply(cols, ops)
    assert st.aggregate().fingerprint.to_int() == model.root()[0]
    # the whole rank order, ranks and selects
    keys = model.sorted_keys()
    fps = st.fingerprints()
    assert np.array_equal(fps, np.stack([np.frombuffer(model.d[k], np.uint8) for k in keys]))
    for r in list(range(0, len(keys), 97)) + [len(keys) - 1]:
        k = st.select(r)
        kb = k.to_bytes(sch.key_row, "little") if isinstance(k, int) else k
        assert kb == keys[r]
        assert st.rank(k) == r
    stats = st.batch_stats()
    comps = st.stats()["compactions"]
    st.close()
    return trace, stats, comps


@pytest.mark.gpu
@pytest.mark.parametrize("spec", SCHEMAS, ids=lambda s: "%s-%s-%s" % s[:3])
def test_small_batch_path_equals_large_path_and_oracle(gpu, oracle_lib, monkeypatch, spec):
    small, s_stats, s_comp = _run(oracle_lib, spec, True, monkeypatch)
    large, l_stats, l_comp = _run(oracle_lib, spec, False, monkeypatch)
    assert small == large
    assert s_stats["small"] >= 10 and l_stats["small"] == 0 and l_stats["large"] >= 12
    assert s_comp > 0 and l_comp > 0


@pytest.mark.gpu
def test_staged_large_batch_keeps_last_operation(gpu, oracle_lib, monkeypatch):
    """A staged batch past the small path (5,000 rows, a third of the keys repeated with mixed
    operations) is sorted on the device and reduced to the last row of each key: the same root and
    rank order as the model folding the rows in order, with no host sort."""
    from rsos_hip import GpuFingerprintStore, RecordSchema
    monkeypatch.delenv("RSOS_HIP_SMALL_MAX", raising=False)
    sch = RecordSchema.dated("bytes16", "bytes64")
    rng = np.random.default_rng(11)
    model = ColumnModel(oracle_lib, sch)
    st = GpuFingerprintStore(sch)
    for rnd in range(3):
        cols, ops = _batch(rng, sch, model, 5000, True, repeats=True)
        st.stage(cols, ops)
        model.apply(cols, ops)
        root, size = model.root()
        agg = st.aggregate()
        assert (agg.size, agg.fingerprint.to_int()) == (size, root), rnd
    keys = model.sorted_keys()
    assert np.array_equal(st.fingerprints(), np.stack([np.frombuffer(model.d[k], np.uint8) for k in keys]))
    assert st.batch_stats()["large"] >= 3
    st.close()


@pytest.mark.gpu
def test_failed_small_merge_is_reported_and_sticks_until_a_load(gpu, oracle_lib):
    """A small batch commits on the host once its first kernel's result word lands, with the delta
    merge still queued behind it.  If that merge fails, the next call on the store reports it
    (RH_ERR_HIP, naming the small batch's merge), and so does every call after it -- the host's
    bookkeeping is ahead of the device -- until a load replaces the contents (fail point
    "small_batch.merge" stands in for the device fault)."""
    from rsos_hip import GpuFingerprintStore, RecordSchema, _abi as A
    sch = RecordSchema.plain("u64", "u64")
    rng = np.random.default_rng(9)
    st = GpuFingerprintStore(sch)
    cols = _gen(rng, sch, 2000, False)
    order = np.argsort(cols["keys"].copy().view("<u8").ravel())
    cols = {c: v[order] for c, v in cols.items()}
    _, first = np.unique(cols["keys"], axis=0, return_index=True)
    cols = {c: v[np.sort(first)] for c, v in cols.items()}
    st.load_bulk(cols)
    n0 = st.size()
    one = _gen(rng, sch, 1, False)
    A.check(A.lib().rh_debug_fail_point(b"small_batch.merge"), "fail point")
    st.apply(one, np.zeros(1, np.uint8))  # commits: the merge's failure is not known yet
    for _ in range(2):
        with pytest.raises(A.RsosHipError) as e:
            st.size()
        assert e.value.code == A.ERR_HIP and "small batch's delta merge failed" in str(e.value)
    with pytest.raises(A.RsosHipError):
        st.aggregate()
    st.load_bulk(cols)  # a load replaces the contents: the store works again
    assert st.size() == n0
    st.apply(one, np.zeros(1, np.uint8))
    assert st.size() == n0 + 1
    assert st.batch_stats()["small"] >= 2
    st.close()
