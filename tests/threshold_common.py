"""What the EnumerateBelowThreshold tests share: the policy's decision restated for oracle/rbsr.py's
literal driver, the decision a round must come to (the reference's non-progress rule and child count
on top of it), a two-call adapter over any view, and small helpers for drives.

The restatement follows rbsr/src/policy/enumerate_below_threshold.rs:141-153 in oracle/rbsr.py's
convention (decide(local, remote, children) over (fp limbs, size) pairs, `_split` for a stride): SKIP
when the aggregates agree, IDLIST when span <= t, else SPLIT with stride ceil(span / b); t = 0 is
raised to 1 (:117-122) and b < 2 to 2 (FanOut::new)."""
import numpy as np

import rbsr as OR  # oracle/rbsr.py


def below_threshold(t: int = 32, b: int = 16):
    t = 1 if t == 0 else t
    b = 2 if b < 2 else b

    def decide(local, remote, children):
        if local == remote:
            return ("skip",)
        if local[1] <= t:
            return ("enumerate",)
        return OR._split((local[1] + b - 1) // b)
    return decide


def expected_decision(decide, lo, hi, local, remote):
    """(kind, stride, children, enums) of one segment with raw ranks [lo, hi), as protocol_round of
    oracle/rbsr.py comes to it: kind 0 skip, 1 IDLIST, 2 SPLIT, 3 dropped; the stride only of a SPLIT."""
    if hi < lo:
        return 3, None, 0, 0
    d = decide(local, remote, 0)
    if d[0] == "split" and local[1] > 1 and d[1] >= local[1]:
        d = ("enumerate",)
    if d[0] == "skip":
        return 0, None, 0, 0
    if d[0] == "enumerate":
        return 1, None, int(remote[1] != 0), 1
    return 2, d[1], len(range(lo + d[1], hi, d[1])) + 1, 0


class TwoCall:
    """rsos_hip.rbsr's two batched questions (resolve_segments, split_segments) answered by a view
    with size / rank / select / aggregate: the two-call path of protocol_round_with_policy, no store."""

    def __init__(self, view):
        self.v = view

    def size(self):
        return self.v.size()

    def _agg(self, start, end):
        from rsos_hip import Aggregate, Fingerprint
        fp, size = self.v.aggregate(start, end)
        return Aggregate(size, Fingerprint(tuple(fp)))

    def aggregate(self):
        return self._agg(None, None)

    def resolve_segments(self, segs):
        n = self.v.size()
        lo = np.array([0 if s.start is None else self.v.rank(s.start) for s in segs], np.uint64)
        hi = np.array([n if s.end is None else self.v.rank(s.end) for s in segs], np.uint64)
        return lo, hi, [self._agg(s.start, s.end) for s in segs]

    def split_segments(self, sel, lo, hi):
        n = self.v.size()
        keys = [self.v.select(int(r)) for r in sel]
        aggs = [self._agg(None if a == 0 else self.v.select(int(a)), None if b >= n else self.v.select(int(b)))
                for a, b in zip(lo, hi)]
        return keys, aggs


def to_product(segs):
    """oracle (start, end, (fp, size)) tuples as the product's RangeAggregates"""
    from rsos_hip import Aggregate, Fingerprint
    from rsos_hip.wire import RangeAggregate
    return [RangeAggregate(s, e, Aggregate(a[1], Fingerprint(tuple(a[0])))) for s, e, a in segs]


def covered(k, ranges):
    return any((s is None or s <= k) and (e is None or k < e) for s, e in ranges)
