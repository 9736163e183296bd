"""What the reconciliation tests share: the ping-pong loop over protocol rounds, the forms its
log compares in, the oracle's FingerprintTreeMap over u32 pairs, a dict model's view for
oracle/rbsr.py's literal driver, and the fixture that runs a module's stores from the device and
then from the host tier."""
import bisect

import numpy as np
import pytest

import oracle as O
from records_common import M256, fp_int


@pytest.fixture(autouse=True, params=["device", "host_tier"])
def store_tier(request):
    """Every GPU store of the importing module answers from the device, then from the host tier
    (rh_store_set_host_tier): the answers must be identical.  Autouse where it is imported by name."""
    import rsos_hip.store as S
    old = S.DEFAULT_HOST_TIER
    S.DEFAULT_HOST_TIER = request.param == "host_tier"
    yield request.param
    S.DEFAULT_HOST_TIER = old


def _u32_recs(pairs):
    pairs = sorted(pairs)
    k = np.array([a for a, _ in pairs], np.uint32)
    v = np.array([b for _, b in pairs], np.uint32)
    n = len(pairs)
    return O.Records(O.Schema(O.KEY_U32, 4, O.VAL_U32, 4, O.REC_PLAIN, 0), k.view(np.uint8).reshape(n, 4),
                     v.view(np.uint8).reshape(n, 4))


def _ftm(recs):
    t = O.FingerprintTreeMap(recs)
    t.fill(0, recs.n)
    return t


def _agg_t(a):
    """rsos_hip Aggregate -> the oracle's (fp limbs, size)."""
    return tuple(int(x) for x in a.fingerprint.limbs), int(a.size)


def _norm(children):
    """A round's children, the product's RangeAggregates as the oracle's (start, end, aggregate) tuples."""
    return [c if isinstance(c, tuple) else (c.start, c.end, _agg_t(c.aggregate)) for c in children]


def _outcome(o):
    return (o.skipped, o.enumerated, o.split, o.children, o.dropped_malformed)


def reconcile(a, b, round_fn, init, max_rounds=200):
    """Ping-pong rounds starting from a's root at b: (log, a's enumerations, b's enumerations),
    the log per round (children, enumerations, outcome)."""
    active = init(a)
    sides = [b, a]
    log, enums = [], {id(a): [], id(b): []}
    for k in range(max_rounds):
        if not active:
            return log, enums[id(a)], enums[id(b)]
        side = sides[k % 2]
        children, en = [], []
        outcome = round_fn(side, active, children, en)
        log.append((_norm(children), list(en), outcome))
        enums[id(side)].extend(en)
        active = children
    raise AssertionError("reconciliation did not terminate")


class DictView:
    """The view oracle/rbsr.py's literal driver asks (size / aggregate / rank / select) over a
    records_common.DictModel's rows: keys in bytes order, fingerprints from the oracle."""

    def __init__(self, model):
        self.ks = sorted(model.rows)
        self.pre = [0]
        for k in self.ks:
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
