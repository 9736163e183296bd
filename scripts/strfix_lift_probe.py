"""Time the short-string-key lift with fixed-width values (RH_KEY_STR under RH_VAL_U64,
lift_strfix.hpp) against two baselines:

  (a) the route such maps took without it: rh_lift_encoded_async over the same records' canonical
      bytes, already resident (the host's encoding work is left out, which favours the baseline);
  (b) for W = 16 and the `full` mix only, the b16_u64 dated schema kernel on the same rows: the same
      row width and one block (56 B against 55 B), so the ratio isolates what composing the string's
      message costs.  Reported, no threshold.

10 M seeded dated records, u64 values, a tag column (all present), row widths 16 / 32 / 64
(--width), two key-length mixes:
  uniform  key lengths uniform in 0..W-1
  full     every key W-1 bytes
Per mix the routes alternate in one process, each launch between two device events, `--reps`
launches each after a warm-up; the outputs of the new lift and the encoded route are compared before
anything is timed.  One JSON line per (width, mix) goes to --out: bytes moved by the byte model
(strfix: the W-byte row + stamp + tag + the 8 B value in, 32 B out, per record; encoded: the
canonical bytes + one 8 B offset in, 32 B out), GiB/s and records/s of the routes (medians), the
ratios, and the encoded route's spread over its alternated repetitions: (p90 - p10) / median of its
launch times.
Criterion: strfix median <= encoded median * (1 + spread).
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
from str_lift_probe import key_rows, stats, timed  # noqa: E402  (scripts/str_lift_probe.py)

TAIL = 20 + 4 + 8  # stamp, State variant, the u64 value


def canonical_bytes(cols, klen, W, chunk=1 << 20):
    """The records' canonical encodings, packed: u64 L, the L key bytes, stamp, variant 0, the u64 value."""
    n = klen.numel()
    plen = 8 + klen + TAIL
    eoffs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    eoffs[1:] = torch.cumsum(plen, 0)
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
                         cols["values"][a:b]], dim=1)
        keep = ~is_key[None, :] | (col[None, :] - 8 < kl)          # key bytes below L only
        pos = torch.where(is_tail[None, :], col[None, :] - (W - 1) + kl, col[None, :])  # the tail follows the key
        enc[(eoffs[a:b, None] + pos)[keep]] = pre[keep]
    return enc, eoffs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--mixes", default="uniform,full")
    ap.add_argument("--width", default="16,32,64", help="row widths, comma separated (16, 32, 64)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "strfix_lift_probe.jsonl"))
    args = ap.parse_args()
    n = args.records
    g = torch.Generator(device="cuda")
    lines = []
    for W, mix in ((int(w), m) for w in args.width.split(",") for m in args.mixes.split(",")):
        schema = RecordSchema.dated(f"str{W - 1}", "u64")
        g.manual_seed(300 + len(mix))
        rows, klen = key_rows(mix, n, g, W)
        cols = {"keys": rows,
                "phys": torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g),
                "logical": torch.randint(0, 1 << 31, (n,), dtype=torch.int32, device="cuda", generator=g),
                "node": torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g),
                "tags": torch.zeros(n, dtype=torch.uint8, device="cuda"),
                "values": torch.randint(0, 256, (n, 8), dtype=torch.uint8, device="cuda", generator=g)}
        enc, eoffs = canonical_bytes(cols, klen, W)
        total_k = int(klen.sum())
        fps_s = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        bs_s = torch.empty(((n + 255) // 256, 32), dtype=torch.uint8, device="cuda")
        routes = {"strfix": lambda: lift_records(schema, cols, fps=fps_s, bsums=bs_s),
                  "encoded": lambda: lift_encoded(enc, eoffs)}
        routes["strfix"]()
        fe, be = routes["encoded"]()
        torch.cuda.synchronize()
        if not (torch.equal(fps_s, fe) and torch.equal(bs_s, be)):
            raise SystemExit(f"width {W}, mix {mix}: the two routes' outputs differ")
        del fe, be
        if W == 16 and mix == "full":  # the row hashed as a [u8; 16] key: other fingerprints, the same traffic
            b16 = RecordSchema.dated("bytes16", "u64")
            fps_b, bs_b = torch.empty_like(fps_s), torch.empty_like(bs_s)
            routes["b16_u64"] = lambda: lift_records(b16, cols, fps=fps_b, bsums=bs_b)
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
        moved = {"strfix": n * (W + 20 + 1 + 8 + 32), "encoded": n * (8 + TAIL + 8 + 32) + total_k,
                 "b16_u64": n * (W + 20 + 1 + 8 + 32)}
        line = {"probe": "strfix_lift", "width": W, "mix": mix, "records": n, "key_bytes": total_k, "reps": args.reps}
        for k in routes:
            t = st[k]["median_ms"] / 1e3
            line[k] = dict(st[k], bytes_moved=moved[k], gib_per_s=moved[k] / t / 2**30, records_per_s=n / t)
        base = st["encoded"]
        spread = (base["p90_ms"] - base["p10_ms"]) / base["median_ms"]
        line["encoded_spread"] = spread
        line["strfix_over_encoded"] = st["strfix"]["median_ms"] / base["median_ms"]
        line["strfix_within_spread"] = st["strfix"]["median_ms"] <= base["median_ms"] * (1 + spread)
        if "b16_u64" in st:
            line["strfix_over_b16_u64"] = st["strfix"]["median_ms"] / st["b16_u64"]["median_ms"]
        print(json.dumps(line), flush=True)
        lines.append(line)
        del cols, enc, eoffs, fps_s, bs_s, rows, routes
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
