"""The lift kernel's two compression forms against the oracle.

k_lift's whole-message path compresses with compress_prio (the wave's issue priority follows the
instruction class) unless RSOS_HIP_LIFT_PRIO=0, which is read at every launch and
selects the plain compression.  Both forms must give the oracle's bytes: fingerprints and 256-row
block sums of dated 16 B / 64 B records at every size around a wave, a block and a tail block, with
and without tombstones; the other lift forms (dual, projection, plain integers, the streamed 1 KiB
value); and the batch path's scattered lift through a store.
"""
import os

import numpy as np
import pytest

from records_common import M256, fp_int, limbs_int, oracle_records

pytestmark = pytest.mark.gpu

SWITCH = "RSOS_HIP_LIFT_PRIO"
SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 4099]
NMAX = max(SIZES)


class form:
    """with form(prio): launches inside read the switch as set here"""

    def __init__(self, prio: bool):
        self.value = "1" if prio else "0"

    def __enter__(self):
        self.old = os.environ.get(SWITCH)
        os.environ[SWITCH] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = self.old


def head(cols, n):
    return {c: t[:n].contiguous() for c, t in cols.items()}


def check_against(O, want, fps, bs, n):
    got = fps.cpu().numpy()
    bad = np.nonzero((got != want[:n]).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} mismatching rows, first {bad[:5]}"
    bounds = list(range(0, n, 256)) + [n]
    sums = O.range_aggregates(want[:n], bounds)
    bsn = bs.cpu().numpy()
    assert bsn.shape[0] == len(sums)
    for g, (limbs, size) in enumerate(sums):
        assert size == bounds[g + 1] - bounds[g]
        assert fp_int(bsn[g]) == limbs_int(limbs), f"block sum {g}"


@pytest.fixture(scope="module")
def dated_sets(gpu, oracle_lib):
    """One 4,099-row dated 16 B / 64 B set with ~10 % tombstones in every wave and one without, and
    the oracle's lift of each; every size below is a prefix of them."""
    from rsos_hip import RecordSchema
    from rsos_hip.synth import make_records, to_host
    s = RecordSchema.dated("bytes16", "bytes64")
    out = {}
    for tags in (False, True):
        cols = make_records(s, NMAX, seed=21, tombstone_fraction=0.1 if tags else 0.0)
        want = oracle_records(oracle_lib, s, to_host(cols)).lift(threads=8)
        want.setflags(write=False)
        out[tags] = (cols, want)
    assert 0.05 * NMAX < int(out[True][0]["tags"].sum()) < 0.15 * NMAX
    return s, out


@pytest.mark.parametrize("tags", [False, True], ids=["present", "tombstones"])
@pytest.mark.parametrize("n", SIZES)
def test_dated_small_records_both_forms(gpu, oracle_lib, dated_sets, n, tags):
    import torch
    from rsos_hip import lift_records
    s, sets = dated_sets
    cols, want = sets[tags]
    for prio in (True, False):
        with form(prio):
            fps, bs = lift_records(s, head(cols, n))
            torch.cuda.synchronize()
        check_against(oracle_lib, want, fps, bs, n)


OTHER = [("projection", "bytes16", "bytes64"), ("plain", "u64", "u64"), ("plain", "u32", "u32"),
         ("dated", "bytes16", "bytes1024")]


@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("kind,key,value", OTHER, ids=[f"{k}-{a}-{b}" for k, a, b in OTHER])
def test_other_lift_forms(gpu, oracle_lib, kind, key, value, n):
    """The projection alone, plain integer records and the 1 KiB value (the streamed path, through
    the shared compression in either setting of the switch)."""
    import torch
    from rsos_hip import RecordSchema, lift_records
    from rsos_hip.synth import make_records, to_host
    s = getattr(RecordSchema, kind)(key, value)
    cols = make_records(s, n, seed=5, tombstone_fraction=0.1 if kind != "plain" else 0.0)
    want = oracle_records(oracle_lib, s, to_host(cols)).lift(threads=8)
    for prio in (True, False):
        with form(prio):
            fps, bs = lift_records(s, cols)
            torch.cuda.synchronize()
        check_against(oracle_lib, want, fps, bs, n)


@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("value", ["bytes64", "bytes1024"])
def test_dual_lift_both_forms(gpu, oracle_lib, value, n):
    """Dated + projection fingerprints from one read of the records, each against the oracle."""
    import torch
    from rsos_hip import RecordSchema, lift_dual
    from rsos_hip.synth import make_records, to_host
    d = RecordSchema.dated("bytes16", value)
    p = d.with_kind(2)
    cols = make_records(d, n, seed=6, tombstone_fraction=0.1)
    h = to_host(cols)
    want_d = oracle_records(oracle_lib, d, h).lift(threads=8)
    want_p = oracle_records(oracle_lib, p, {k: v for k, v in h.items() if k in ("keys", "values", "tags")}).lift(threads=8)
    for prio in (True, False):
        with form(prio):
            fd, bd, fpj, bpj = lift_dual(d, cols)
            torch.cuda.synchronize()
        check_against(oracle_lib, want_d, fd, bd, n)
        check_against(oracle_lib, want_p, fpj, bpj, n)


def test_scattered_lift_through_a_store(gpu, oracle_lib):
    """A 1,000-row and a 70,000-row batch of new random keys applied to a store (the batch path
    lifts each record into its sorted row); the root is the oracle's fold over every record."""
    import torch
    from rsos_hip import GpuFingerprintStore, RecordSchema
    from rsos_hip.synth import make_records, to_host
    s = RecordSchema.dated("bytes16", "bytes64")

    def lifted_sum(cols):
        return sum(fp_int(f) for f in oracle_records(oracle_lib, s, to_host(cols)).lift(threads=8))

    base = make_records(s, 5000, seed=42, key_space=5000)
    batches = [make_records(s, m, seed=70 + m, random_keys=True) for m in (1000, 70_000)]
    wants, acc, size = [], lifted_sum(base), 5000
    for b in batches:
        acc += lifted_sum(b)
        size += b["keys"].shape[0]
        wants.append((acc % M256, size))
    for prio in (True, False):
        with form(prio):
            st = GpuFingerprintStore(s)
            st.load_bulk_device(base)
            for b, (root, size) in zip(batches, wants):
                assert st.apply_device(b) == (b["keys"].shape[0], 0, 0)
                a = st.aggregate()
                assert a.size == size and a.fingerprint.to_int() == root
            st.close()
            torch.cuda.synchronize()


def test_switch_selects_identical_bytes(gpu, dated_sets):
    """RSOS_HIP_LIFT_PRIO=0 and the default give the same fingerprints and block sums (n = 4,099)."""
    import torch
    from rsos_hip import lift_records
    s, sets = dated_sets
    for tags in (False, True):
        cols, _ = sets[tags]
        with form(True):
            a, ab = lift_records(s, cols)
            torch.cuda.synchronize()
        with form(False):
            b, bb = lift_records(s, cols)
            torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(ab, bb)
