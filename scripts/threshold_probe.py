"""Whole reconciliation drives under FixedFanOut(16) and EnumerateBelowThreshold(32, 16), and the d = 1
enumerate call with the one-launch kernel on and off.

Two --n-row (default 10 M) u64 -> u64 stores that differ in d rows (enumerate_probe.build: half changed
values, half keys only one side holds; d = 1, 100 and 10^4) are driven to completion inside the library
(rh_store_protocol_round / rh_store_protocol_round_threshold), the responder answering every round's
IDLIST ranges with one rh_store_enumerate_segments call, with the host tier off and then on.  Per
(d, tier, policy): the rounds, the segments sent (the root and every child), the IDLIST ranges and
the enumerated keys of a drive -- counts, the same every drive -- and the drive's time on the host
clock: the median of --reps drives, with the minimum and maximum.
Then, for d = 1 with the tier off, the drive's one enumerate call (one range) alone on stores created
with RSOS_HIP_ENUM_FUSED=1 and =0: --reps repeats of 200 calls each; the median of the repeats'
medians, and their range.
One JSON line per case goes to --out (default profiles/threshold_probe.jsonl).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get("RSOS_HIP_TREE") or os.path.join(HERE, "..", "reconcile-rs_amd"))
from enumerate_probe import build  # noqa: E402
from rsos_hip import _abi as A  # noqa: E402
from rsos_hip import rbsr as R  # noqa: E402


def drive(a, b, policy):
    """one reconciliation: (rounds, segments sent, IDLIST ranges, enumerated keys, the last round's
    enumerations on its store)"""
    active, sides = R.initial_segments(a), [b, a]
    rounds = segments = ranges = keys = 0
    last = None
    for k in range(64):
        st = sides[k % 2]
        segments += len(active)
        ch, en, _ = R.protocol_round_segments(st, policy, active, raw=True)
        rounds += 1
        if len(en):
            out = A.Enumerated()
            cs = en.c()
            A.check(A.lib().rh_store_enumerate_segments(st._h, C.byref(cs), 0, C.byref(out)), "enumerate")
            ranges += len(en)
            keys += int(out.rows)
            last = (st, R._wrap(en.cs, st.schema.key_row, True, False))
        if not len(ch):
            break
        active = ch
    return rounds, segments, ranges, keys, last


def timed_drives(a, b, policy, reps):
    drive(a, b, policy)  # warm
    us, counts = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = drive(a, b, policy)
        us.append((time.perf_counter() - t0) * 1e6)
        counts = res[:4]
    us.sort()
    return counts, us


def enumerate_call(n, reps, fused):
    """the d = 1 drive's enumerate call on stores created with RSOS_HIP_ENUM_FUSED=fused"""
    os.environ["RSOS_HIP_ENUM_FUSED"] = str(fused)
    a, b = build(n, 1, 5)
    del os.environ["RSOS_HIP_ENUM_FUSED"]
    st, en = drive(a, b, R.FixedFanOut(16))[4]
    cs, out = en.c(), A.Enumerated()
    call, h = A.lib().rh_store_enumerate_segments, st._h
    meds = []
    for _ in range(reps):
        t = []
        for _ in range(200):
            t0 = time.perf_counter()
            call(h, C.byref(cs), 0, C.byref(out))
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        meds.append(t[100])
    stats = st.enumerate_stats()
    a.close(), b.close()
    meds.sort()
    return {"ranges": en.n, "rows": int(out.rows), "median_us": round(meds[len(meds) // 2], 2),
            "repeat_medians_us": [round(x, 2) for x in meds], "one_launch_calls": stats["one_launch"],
            "general_calls": stats["general"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, nargs="*", default=[1, 100, 10_000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "threshold_probe.jsonl"))
    args = ap.parse_args()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
    policies = (("FixedFanOut(16)", R.FixedFanOut(16)), ("EnumerateBelowThreshold(32,16)", R.EnumerateBelowThreshold(32, 16)))
    for d in args.d:
        a, b = build(args.n, d, 5)
        for tier in (0, 1):
            for st in (a, b):
                st.set_host_tier(bool(tier))
                if tier:
                    st.tier_sync()
            for name, policy in policies:
                (rounds, segments, ranges, keys), us = timed_drives(a, b, policy, args.reps)
                emit({"probe": "threshold_drive", "n": args.n, "d": d, "host_tier": tier, "policy": name, "reps": args.reps,
                      "rounds": rounds, "segments": segments, "idlist_ranges": ranges, "enumerated_keys": keys,
                      "drive_us": [round(x, 1) for x in (us[len(us) // 2], us[0], us[-1])]})
        a.close(), b.close()
    for fused in (1, 0):
        emit(dict({"probe": "enumerate_d1", "n": args.n, "enum_fused": fused, "reps": args.reps},
                  **enumerate_call(args.n, max(args.reps, 5), fused)))
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
