"""Time the variable-length-value lift (RH_VAL_VARBYTES, lift_var.hpp) against the only route such
records had before it: rh_lift_encoded_async over the same records' canonical bytes, already
resident (the host's encoding work is left out, which favours the baseline).

10 M seeded records, bytes16 key, dated, a tag column (all present), three value-length mixes:
  i    every value 64 B
  ii   lengths uniform in [0, 256)
  iii  1 % of the values 4 KiB, the rest 32 B
Per mix the two routes alternate in one process, each launch between two device events, `--reps`
launches each after a warm-up; the two outputs are compared before anything is timed.  One JSON
line per mix goes to --out:
  bytes moved by the byte model (var: key + stamp + tag + one 8 B offset + the value bytes in, 32 B
  out, per record; encoded: the canonical bytes + one 8 B offset in, 32 B out), GiB/s and records/s
  of both routes (medians), their ratio, and the baseline's spread over its alternated
  repetitions: (p90 - p10) / median of its launch times (robust to one slow launch; min and max
  are reported beside it).
Criterion (mix ii): var median <= encoded median * (1 + spread).
Mix i is also timed against the fixed-width schema kernel (dated bytes16 / bytes64), for information.

Kernel times: a separate run under `rocprofv3 --kernel-trace --stats -- python scripts/var_lift_probe.py`.
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

P = 56  # bytes16 dated prefix: 8 + 16 key, 20 stamp, 4 variant, 8 value length


def lengths(mix, n, g):
    if mix == "i":
        return torch.full((n,), 64, dtype=torch.int64, device="cuda")
    if mix == "ii":
        return torch.randint(0, 256, (n,), dtype=torch.int64, device="cuda", generator=g)
    big = torch.rand((n,), device="cuda", generator=g) < 0.01
    return torch.where(big, torch.tensor(4096, device="cuda"), torch.tensor(32, device="cuda")).to(torch.int64)


def canonical_bytes(cols, lens, voffs, chunk=1 << 20):
    """The records' canonical encodings, packed: per record the 56 prefix bytes, then its value."""
    n = lens.numel()
    eoffs = voffs + P * torch.arange(n + 1, dtype=torch.int64, device="cuda")
    enc = torch.empty(((int(eoffs[-1]) + 3) // 4 * 4,), dtype=torch.uint8, device="cuda")
    enc[int(eoffs[-1]):] = 0
    klen = torch.tensor([16, 0, 0, 0, 0, 0, 0, 0], dtype=torch.uint8, device="cuda")
    col = torch.arange(P, dtype=torch.int64, device="cuda")
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        pre = torch.cat([klen.expand(b - a, 8), cols["keys"][a:b], cols["phys"][a:b].view(torch.uint8).view(-1, 8),
                         cols["logical"][a:b].view(torch.uint8).view(-1, 4),
                         cols["node"][a:b].view(torch.uint8).view(-1, 8),
                         torch.zeros((b - a, 4), dtype=torch.uint8, device="cuda"),  # State::Present
                         lens[a:b].view(torch.uint8).view(-1, 8)], dim=1)
        enc[(eoffs[a:b, None] + col).reshape(-1)] = pre.reshape(-1)
        v0, v1 = int(voffs[a]), int(voffs[b])
        if v1 > v0:
            rec = torch.repeat_interleave(torch.arange(a, b, device="cuda"), lens[a:b])
            src = torch.arange(v0, v1, dtype=torch.int64, device="cuda")
            enc[src + P * (rec + 1)] = cols["values"][v0:v1]
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
    ap.add_argument("--mixes", default="i,ii,iii")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "var_lift_probe.jsonl"))
    args = ap.parse_args()
    n = args.records
    var_schema, fixed_schema = RecordSchema.dated("bytes16", "var"), RecordSchema.dated("bytes16", "bytes64")
    g = torch.Generator(device="cuda")
    lines = []
    for mix in args.mixes.split(","):
        g.manual_seed(100 + len(mix))
        lens = lengths(mix, n, g)
        voffs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        voffs[1:] = torch.cumsum(lens, 0)
        total_v = int(voffs[-1])
        cols = {"keys": torch.randint(0, 256, (n, 16), dtype=torch.uint8, device="cuda", generator=g),
                "phys": torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g),
                "logical": torch.randint(0, 1 << 31, (n,), dtype=torch.int32, device="cuda", generator=g),
                "node": torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g),
                "tags": torch.zeros(n, dtype=torch.uint8, device="cuda"),
                "values": torch.randint(0, 256, ((total_v + 3) // 4 * 4,), dtype=torch.uint8, device="cuda", generator=g),
                "value_offsets": voffs}
        enc, eoffs = canonical_bytes(cols, lens, voffs)
        fps_v = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        bs_v = torch.empty(((n + 255) // 256, 32), dtype=torch.uint8, device="cuda")
        run_var = lambda: lift_records(var_schema, cols, fps=fps_v, bsums=bs_v)  # noqa: E731
        run_enc = lambda: lift_encoded(enc, eoffs)  # noqa: E731
        run_var()
        fe, be = run_enc()
        torch.cuda.synchronize()
        if not (torch.equal(fps_v, fe) and torch.equal(bs_v, be)):
            raise SystemExit(f"mix {mix}: the two routes' outputs differ")
        del fe, be
        routes = {"var": run_var, "encoded": run_enc}
        if mix == "i":
            fcols = {k: cols[k] for k in ("keys", "phys", "logical", "node", "tags")}
            fcols["values"] = cols["values"][:n * 64].view(n, 64)
            ff, _ = lift_records(fixed_schema, fcols)
            torch.cuda.synchronize()
            if not torch.equal(ff, fps_v):
                raise SystemExit("mix i: the fixed-width schema kernel's output differs")
            del ff
            fps_f = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
            bs_f = torch.empty_like(bs_v)
            routes["fixed_schema"] = lambda: lift_records(fixed_schema, fcols, fps=fps_f, bsums=bs_f)  # noqa: E731
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
        moved = {"var": n * (16 + 20 + 1 + 8 + 32) + total_v, "encoded": n * (P + 8 + 32) + total_v,
                 "fixed_schema": n * (16 + 20 + 1 + 64 + 32)}
        line = {"probe": "var_lift", "mix": mix, "records": n, "value_bytes": total_v, "reps": args.reps}
        for k in routes:
            t = st[k]["median_ms"] / 1e3
            line[k] = dict(st[k], bytes_moved=moved[k], gib_per_s=moved[k] / t / 2**30, records_per_s=n / t)
        base = st["encoded"]
        spread = (base["p90_ms"] - base["p10_ms"]) / base["median_ms"]
        line["encoded_spread"] = spread
        line["var_over_encoded"] = st["var"]["median_ms"] / base["median_ms"]
        line["var_within_spread"] = st["var"]["median_ms"] <= base["median_ms"] * (1 + spread)
        if mix == "i":
            line["var_over_fixed_schema"] = st["var"]["median_ms"] / st["fixed_schema"]["median_ms"]
        print(json.dumps(line), flush=True)
        lines.append(line)
        del cols, enc, eoffs, fps_v, bs_v
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
