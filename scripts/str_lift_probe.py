"""Time the short-string-key lift (RH_KEY_STR, lift_str.hpp) against the route such maps take
without it: rh_lift_encoded_async over the same records' canonical bytes, already resident (the
host's encoding work is left out, which favours the baseline).

10 M seeded records, str31 keys (--width 32; 16, 32 and 64 are the row widths, several may be
given), dated, a tag column (all present), value lengths uniform in [0, 256), two key-length mixes:
  uniform  key lengths uniform in 0..W-1
  full     every key W-1 bytes
Per mix the two routes alternate in one process, each launch between two device events, `--reps`
launches each after a warm-up; the two outputs are compared before anything is timed.  One JSON
line per mix goes to --out:
  bytes moved by the byte model (str: the W-byte row + stamp + tag + one 8 B offset + the value bytes
  in, 32 B out, per record; encoded: the canonical bytes + one 8 B offset in, 32 B out), GiB/s and
  records/s of both routes (medians), their ratio, and the baseline's spread over its alternated
  repetitions: (p90 - p10) / median of its launch times.
Criterion: str median <= encoded median * (1 + spread).
With --width 32,64 in one run, each width-64 line also carries the str63 target: its ratio to the
encoded route at most the str31 ratio of the same mix and run, times (1 + the encoded route's spread).

Kernel times: a separate run under `rocprofv3 --kernel-trace --stats -- python scripts/str_lift_probe.py`.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("RSOS_HIP_TREE") or
                os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "reconcile-rs_amd"))
import torch  # noqa: E402
from rsos_hip import RecordSchema, lift_encoded, lift_records  # noqa: E402

TAIL = 20 + 4 + 8  # stamp, State variant, the value's u64 length


def key_rows(mix, n, g, W):
    """n rows in RH_KEY_STR form: L bytes, zero padding, L in byte W - 1."""
    if mix == "uniform":
        klen = torch.randint(0, W, (n,), dtype=torch.int64, device="cuda", generator=g)
    else:
        klen = torch.full((n,), W - 1, dtype=torch.int64, device="cuda")
    rows = torch.randint(0, 256, (n, W), dtype=torch.uint8, device="cuda", generator=g)
    rows *= (torch.arange(W, device="cuda")[None, :] < klen[:, None]).to(torch.uint8)
    rows[:, W - 1] = klen.to(torch.uint8)
    return rows, klen


def canonical_bytes(cols, klen, lens, voffs, W, chunk=1 << 19):
    """The records' canonical encodings, packed: u64 L, the L key bytes, stamp, variant 0, u64
    value length, the value."""
    n = lens.numel()
    plen = 8 + klen + TAIL
    cum = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    cum[1:] = torch.cumsum(plen, 0)
    eoffs = voffs + cum
    enc = torch.zeros(((int(eoffs[-1]) + 3) // 4 * 4,), dtype=torch.uint8, device="cuda")
    col = torch.arange(8 + (W - 1) + TAIL, dtype=torch.int64, device="cuda")
    is_key, is_tail = (col >= 8) & (col < 8 + W - 1), col >= 8 + W - 1
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        kl = klen[a:b, None]
        pre = torch.cat([klen[a:b].view(torch.uint8).view(-1, 8), cols["keys"][a:b, :W - 1],
                         cols["phys"][a:b].view(torch.uint8).view(-1, 8),
                         cols["logical"][a:b].view(torch.uint8).view(-1, 4),
                         cols["node"][a:b].view(torch.uint8).view(-1, 8),
                         torch.zeros((b - a, 4), dtype=torch.uint8, device="cuda"),  # State::Present
                         lens[a:b].view(torch.uint8).view(-1, 8)], dim=1)
        keep = ~is_key[None, :] | (col[None, :] - 8 < kl)          # key bytes below L only
        pos = torch.where(is_tail[None, :], col[None, :] - (W - 1) + kl, col[None, :])  # the tail follows the key
        enc[(eoffs[a:b, None] + pos)[keep]] = pre[keep]
        v0, v1 = int(voffs[a]), int(voffs[b])
        if v1 > v0:
            rec = torch.repeat_interleave(torch.arange(a, b, device="cuda"), lens[a:b])
            src = torch.arange(v0, v1, dtype=torch.int64, device="cuda")
            enc[src + cum[rec + 1]] = cols["values"][v0:v1]
    return enc, eoffs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "min_ms": s[0], "max_ms": s[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--mixes", default="uniform,full")
    ap.add_argument("--width", default="32", help="row widths, comma separated (16, 32, 64)")
    ap.add_argument("--out", default=None, help="default: profiles/str_lift_probe.jsonl; with a width of 64, "
                                                "profiles/str63_lift_probe.jsonl")
    args = ap.parse_args()
    n = args.records
    widths = [int(w) for w in args.width.split(",")]
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                "str63_lift_probe.jsonl" if 64 in widths else "str_lift_probe.jsonl")
    g = torch.Generator(device="cuda")
    lines = []
    for W, mix in ((w, m) for w in widths for m in args.mixes.split(",")):
        schema = RecordSchema.dated(f"str{W - 1}", "var")
        g.manual_seed(200 + len(mix))
        lens = torch.randint(0, 256, (n,), dtype=torch.int64, device="cuda", generator=g)
        voffs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        voffs[1:] = torch.cumsum(lens, 0)
        total_v = int(voffs[-1])
        rows, klen = key_rows(mix, n, g, W)
        cols = {"keys": rows,
                "phys": torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g),
                "logical": torch.randint(0, 1 << 31, (n,), dtype=torch.int32, device="cuda", generator=g),
                "node": torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g),
                "tags": torch.zeros(n, dtype=torch.uint8, device="cuda"),
                "values": torch.randint(0, 256, ((total_v + 3) // 4 * 4,), dtype=torch.uint8, device="cuda", generator=g),
                "value_offsets": voffs}
        enc, eoffs = canonical_bytes(cols, klen, lens, voffs, W)
        total_k = int(klen.sum())
        fps_s = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        bs_s = torch.empty(((n + 255) // 256, 32), dtype=torch.uint8, device="cuda")
        run_str = lambda: lift_records(schema, cols, fps=fps_s, bsums=bs_s)  # noqa: E731
        run_enc = lambda: lift_encoded(enc, eoffs)  # noqa: E731
        run_str()
        fe, be = run_enc()
        torch.cuda.synchronize()
        if not (torch.equal(fps_s, fe) and torch.equal(bs_s, be)):
            raise SystemExit(f"mix {mix}: the two routes' outputs differ")
        del fe, be
        routes = {"str": run_str, "encoded": run_enc}
        t_end = time.perf_counter() + 0.4  # clock spin-up, and every route warm
        while time.perf_counter() < t_end:
            for fn in routes.values():
                fn()
            torch.cuda.synchronize()
        ev = {k: [] for k in routes}
        for _ in range(args.reps):  # alternating, one process
            for k, fn in routes.items():
                ev[k].append(timed(fn))
        torch.cuda.synchronize()
        st = {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
        moved = {"str": n * (W + 20 + 1 + 8 + 32) + total_v,
                 "encoded": n * (8 + TAIL + 8 + 32) + total_k + total_v}
        line = {"probe": "str_lift", "width": W, "mix": mix, "records": n, "key_bytes": total_k, "value_bytes": total_v,
                "reps": args.reps}
        for k in routes:
            t = st[k]["median_ms"] / 1e3
            line[k] = dict(st[k], bytes_moved=moved[k], gib_per_s=moved[k] / t / 2**30, records_per_s=n / t)
        base = st["encoded"]
        spread = (base["p90_ms"] - base["p10_ms"]) / base["median_ms"]
        line["encoded_spread"] = spread
        line["str_over_encoded"] = st["str"]["median_ms"] / base["median_ms"]
        line["str_within_spread"] = st["str"]["median_ms"] <= base["median_ms"] * (1 + spread)
        ref = [x for x in lines if x["width"] == 32 and x["mix"] == mix]
        if W == 64 and ref:  # the str63 target, against the str31 ratio of this run
            line["str31_over_encoded"] = ref[0]["str_over_encoded"]
            line["target_ratio"] = ref[0]["str_over_encoded"] * (1 + spread)
            line["meets_target"] = line["str_over_encoded"] <= line["target_ratio"]
        print(json.dumps(line), flush=True)
        lines.append(line)
        del cols, enc, eoffs, fps_s, bs_s, rows
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
