"""Time the responder's enumeration of a reconciliation's IDLIST ranges: one
rh_store_enumerate_segments call per round beside the per-range loop of examples/rbsr_latency.c
(rh_store_ranks for a range's bounds, then rh_store_keys for its rows).

Two --n-row (default 10 M) u64 -> u64 stores that differ in d rows (d = 10^4 and d = 1: half changed
values, half keys only one side holds) are driven to completion with rh_store_protocol_round,
FixedFanOut(16).  For every round that returns enumerations, both ways answer the same ranges on the
responder, in this process, on that store, alternating, --reps times each (a round of at most 100
ranges at least 200 times; the median is kept, with the minimum and maximum beside it per round),
with the host tier off and then on.  The loop uses only calls that exist without
the batched Enumerate, so it is the baseline; its bound keys and output buffer are prepared outside
the timed region, and both ways pay the same ctypes call overhead per call.  The two answers are
compared before anything is timed.
One JSON line per (d, tier) goes to --out (default profiles/enumerate_probe.jsonl): the rounds, the
IDLIST ranges and rows, the summed medians of both ways in microseconds, their ratio, and per round
[median, min, max] of both.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("RSOS_HIP_TREE") or os.path.join(HERE, "..", "reconcile-rs_amd"))
import numpy as np  # noqa: E402
from rsos_hip import GpuFingerprintStore, RecordSchema, _abi as A  # noqa: E402
from rsos_hip import rbsr as R  # noqa: E402


def build(n, d, seed):
    """stores a and b of n rows each, differing in d rows"""
    rng = np.random.default_rng(seed)
    sch = RecordSchema.plain("u64", "u64")
    changed = d // 2                   # rows whose value differs
    only_a = (d - changed) // 2        # keys only a holds
    only_b = d - changed - only_a      # keys only b holds
    m = n + only_b                     # a holds n of these keys, b holds n + only_b - only_a
    keys = np.arange(m, dtype=np.uint64) * np.uint64(7) + np.uint64(3)
    vals = rng.integers(0, 1 << 62, m, dtype=np.uint64)
    swap = rng.choice(m, only_a + only_b, replace=False)
    in_a, in_b = np.ones(m, bool), np.ones(m, bool)
    in_a[swap[:only_b]] = False
    in_b[swap[only_b:]] = False
    vb = vals.copy()
    both = np.flatnonzero(in_a & in_b)
    vb[rng.choice(both, changed, replace=False)] ^= np.uint64(1)
    stores = []
    for mask, v in ((in_a, vals), (in_b, vb)):
        st = GpuFingerprintStore(sch, host_tier=False)
        st.load_bulk({"keys": keys[mask].view(np.uint8).reshape(-1, 8), "values": v[mask].view(np.uint8).reshape(-1, 8)})
        stores.append(st)
    return stores


def timed_us(fns, reps):
    """every fn timed reps times, alternating: sorted microseconds per fn"""
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            t[i].append((time.perf_counter() - t0) * 1e6)
    return [sorted(x) for x in t]


def enumerate_both(st, en, reps):
    """the ranges `en` (a copied rbsr.Segments) on store st: (loop's sorted us, the one call's, rows);
    a round of at most 100 ranges is repeated at least 200 times (its calls take microseconds)"""
    L, h, r = A.lib(), st._h, en.n
    ranks, keys_fn, one = L.rh_store_ranks, L.rh_store_keys, L.rh_store_enumerate_segments
    # the loop's questions, prepared: both bounds' keys of range j side by side, as rbsr_latency.c asks them
    q = np.zeros((r, 2), np.uint64)
    nq = np.zeros(r, np.int64)
    sk, ek = en.start_kinds[:r].astype(bool), en.end_kinds[:r].astype(bool)
    skey, ekey = en.start_keys[:r].copy().view("<u8").ravel(), en.end_keys[:r].copy().view("<u8").ravel()
    for j in range(r):
        if sk[j]:
            q[j, nq[j]] = skey[j]
            nq[j] += 1
        if ek[j]:
            q[j, nq[j]] = ekey[j]
            nq[j] += 1
    size = st.size()
    qp = [q[j].ctypes.data for j in range(r)]
    rk = (C.c_uint64 * 2)()
    first, offs, rows = st.enumerate_segments(en)
    buf = np.zeros(max(int(np.diff(offs).max(initial=0)), 1) * 8, np.uint8)
    bp = buf.ctypes.data
    plan = [(qp[j], int(nq[j]), bool(sk[j]), bool(ek[j])) for j in range(r)]

    def loop(check=None):
        for j, (p, m, s, e) in enumerate(plan):
            lo, hi = 0, size
            if m:
                ranks(h, p, m, rk)
                if s:
                    lo = rk[0]
                if e:
                    hi = rk[m - 1]
            if hi > lo:
                keys_fn(h, lo, hi, bp)
            if check is not None:
                check(j, lo, max(hi, lo), buf)

    def same(j, lo, hi, b):  # the loop's answer is the one call's
        assert lo == first[j] and hi - lo == offs[j + 1] - offs[j], (j, lo, hi)
        assert np.array_equal(b[:(hi - lo) * 8], rows[int(offs[j]):int(offs[j + 1])].ravel()), j
    loop(same)
    cs, out = en.c(), A.Enumerated()

    def one_call():
        one(h, C.byref(cs), 0, C.byref(out))
    one_call()
    assert out.rows == rows.shape[0]
    lp, oc = timed_us([loop, one_call], reps if r > 100 else max(reps, 200))
    return lp, oc, int(out.rows)


def drive(a, b, reps):
    """one reconciliation; every round's enumerations answered both ways on the responder"""
    active, sides = R.initial_segments(a), [b, a]
    res = {"rounds": 0, "idlist_rounds": 0, "idlist_ranges": 0, "rows": 0, "loop_us": 0.0, "one_call_us": 0.0, "per_round": []}
    for k in range(64):
        st = sides[k % 2]
        ch, en, _ = R.protocol_round_segments(st, R.FixedFanOut(16), active, copy=True)
        res["rounds"] += 1
        if en.n:
            lp, oc, rows = enumerate_both(st, en, reps)
            res["idlist_rounds"] += 1
            res["idlist_ranges"] += en.n
            res["rows"] += rows
            res["loop_us"] += lp[len(lp) // 2]
            res["one_call_us"] += oc[len(oc) // 2]
            res["per_round"].append({"ranges": en.n, "rows": rows, "reps": len(lp),
                                     "loop_us": [round(x, 2) for x in (lp[len(lp) // 2], lp[0], lp[-1])],
                                     "one_call_us": [round(x, 2) for x in (oc[len(oc) // 2], oc[0], oc[-1])]})
        active = ch
        if not active.n:
            break
    res["loop_us"], res["one_call_us"] = round(res["loop_us"], 2), round(res["one_call_us"], 2)
    res["loop_over_one_call"] = round(res["loop_us"] / res["one_call_us"], 2) if res["one_call_us"] else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, nargs="*", default=[10_000, 1])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "enumerate_probe.jsonl"))
    args = ap.parse_args()
    lines = []
    for d in args.d:
        a, b = build(args.n, d, 5)
        for tier in (0, 1):
            for st in (a, b):
                st.set_host_tier(bool(tier))
                if tier:
                    st.tier_sync()
            res = drive(a, b, args.reps)
            lines.append(dict({"probe": "enumerate", "n": args.n, "d": d, "host_tier": tier, "reps": args.reps}, **res))
            print(json.dumps(lines[-1]), flush=True)
        a.close(), b.close()
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
