"""Time the ragged snapshot reload (RH_FORM_RAGGED, csrc/snap_ragged.hip): a str31 -> var file
reloaded into a dated and a projection store from device-resident bytes.

File shape: key lengths uniform in 1..31, value lengths uniform in 0..200, 10 % tombstones, file
order sorted by key (rows that repeat a key are dropped, so a file holds a little under --records
entries; the line records the count).  Per size (--records, comma separated) one JSON line:
  reload ms into both stores (median of --reps after a warm-up), the locate / lift split of
  rh_debug_last_reload_us, and the locate's segments, rounds and rewalked segments.
Two reference lines per size, same entry count, a b32v_b64 file (Vec<u8> 32-byte keys, 64-byte
values) both routes can read: its flag-clear reload, and its flag-set reload -- the price of the
byte-granular locate.  One more line per run: the first size's file with one value of 1 MiB of
zero bytes (every position in it parses as an entry), which shows the cost of the fix-up rounds.
The segment size is the library's (RSOS_HIP_RAGGED_SEG overrides it for a sweep).
Lines go to --out (default profiles/ragged_snapshot_probe.jsonl).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("RSOS_HIP_TREE") or
                os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "reconcile-rs_amd"))
import torch  # noqa: E402
from rsos_hip import GpuFingerprintStore, RecordSchema, _abi as A  # noqa: E402
from rsos_hip.snapshot import load_snapshot, ragged_stats  # noqa: E402
from rsos_hip.synth import make_records, make_snapshot  # noqa: E402

W = 32


def sorted_unique_keys(n, g):
    """Up to n distinct strings of 1..31 bytes in Ord order, as padded rows and lengths."""
    klen = torch.randint(1, W, (n,), dtype=torch.int64, device="cuda", generator=g)
    rows = torch.randint(0, 256, (n, W), dtype=torch.uint8, device="cuda", generator=g)
    rows *= (torch.arange(W, device="cuda")[None, :] < klen[:, None]).to(torch.uint8)
    rows[:, W - 1] = klen.to(torch.uint8)
    # memcmp order of the rows = Ord of the strings: four big-endian words, least significant first
    words = rows.view(n, 4, 8).flip(2).contiguous().view(torch.int64).view(n, 4) ^ (-1 << 63)
    order = torch.arange(n, device="cuda")
    for w in (3, 2, 1, 0):
        order = order[torch.sort(words[order, w], stable=True)[1]]
    rows, words = rows[order], words[order]
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[1:] = (words[1:] != words[:-1]).any(1)
    rows = rows[keep]
    return rows, rows[:, W - 1].to(torch.int64)


def build_file(n, seed, zero_value=0, chunk=1 << 19):
    """The file's bytes on the device and its entry count."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rows, klen = sorted_unique_keys(n, g)
    n = rows.shape[0]
    tomb = torch.rand(n, device="cuda", generator=g) < 0.1
    vlen = torch.randint(0, 201, (n,), dtype=torch.int64, device="cuda", generator=g)
    if zero_value:
        tomb[n // 2] = False
        vlen[n // 2] = zero_value
    vlen = torch.where(tomb, torch.zeros_like(vlen), vlen)
    elen = 8 + klen + 24 + torch.where(tomb, torch.zeros_like(vlen), 8 + vlen)
    offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    offs[1:] = torch.cumsum(elen, 0)
    offs += 16
    end = int(offs[-1])
    blob = torch.randint(0, 256, (end + 16,), dtype=torch.uint8, device="cuda", generator=g)  # the values' bytes
    head = torch.tensor(list(b"RCNL") + [1, 0, 0, 0], dtype=torch.uint8, device="cuda")
    blob[:8] = head
    blob[8:16] = torch.tensor([n], dtype=torch.int64, device="cuda").view(torch.uint8)
    blob[end:] = 0  # no members, no acks
    phys = torch.randint(1 << 40, 1 << 41, (n,), dtype=torch.int64, device="cuda", generator=g)
    logical = torch.randint(0, 1 << 31, (n,), dtype=torch.int32, device="cuda", generator=g)
    node = torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g)
    col = torch.arange(8 + (W - 1) + 24 + 8, dtype=torch.int64, device="cuda")
    is_key, is_tail, is_m = (col >= 8) & (col < 8 + W - 1), col >= 8 + W - 1, col >= 8 + W - 1 + 24
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        kl = klen[a:b, None]
        pre = torch.cat([klen[a:b].view(torch.uint8).view(-1, 8), rows[a:b, :W - 1],
                         phys[a:b].view(torch.uint8).view(-1, 8), logical[a:b].view(torch.uint8).view(-1, 4),
                         node[a:b].view(torch.uint8).view(-1, 8),
                         tomb[a:b].to(torch.int32).view(torch.uint8).view(-1, 4),
                         vlen[a:b].view(torch.uint8).view(-1, 8)], dim=1)
        keep = (~is_key[None, :] | (col[None, :] - 8 < kl)) & (~is_m[None, :] | ~tomb[a:b, None])
        pos = torch.where(is_tail[None, :], col[None, :] - (W - 1) + kl, col[None, :])
        blob[(offs[a:b, None] + pos)[keep]] = pre[keep]
    if zero_value:
        z = int(offs[n // 2 + 1])
        blob[z - zero_value:z] = 0
    return blob, n


def time_reload(blob, sd, sp, form, ragged, reps):
    dated, proj = GpuFingerprintStore(sd), GpuFingerprintStore(sp)
    A.lib().rh_debug_reload_timing(1)
    ms, split = [], []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = load_snapshot(blob, dated, proj, form, ragged=ragged)
        torch.cuda.synchronize()
        if r:  # the first reload allocates
            ms.append(1e3 * (time.perf_counter() - t0))
            lo, li = C.c_double(), C.c_double()
            A.lib().rh_debug_last_reload_us(C.byref(lo), C.byref(li))
            split.append((lo.value / 1e3, li.value / 1e3))
    A.lib().rh_debug_reload_timing(0)
    ms.sort()
    split.sort()
    out = {"reload_ms": ms[len(ms) // 2], "reload_min_ms": ms[0], "reload_max_ms": ms[-1],
           "locate_ms": split[len(split) // 2][0], "lift_ms": split[len(split) // 2][1],
           "entries": info.entries, "keys": info.keys, "tombstones": info.tombstones, "file_bytes": blob.numel()}
    if ragged:
        out.update(ragged_stats())
    dated.close(), proj.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "ragged_snapshot_probe.jsonl"))
    args = ap.parse_args()
    sizes = [int(x) for x in args.records.split(",")]
    sd, sp = RecordSchema.dated("str31", "var"), RecordSchema.projection("str31", "var")
    fd, fp = RecordSchema.dated("bytes32", "bytes64"), RecordSchema.projection("bytes32", "bytes64")
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
    for n in sizes:
        blob, m = build_file(n, 7)
        rag = time_reload(blob, sd, sp, "vec", True, args.reps)
        emit(dict({"probe": "ragged_snapshot", "file": "str31_var", "route": "ragged", "records": n}, **rag))
        del blob
        torch.cuda.empty_cache()
        fixed = make_snapshot(make_records(fd, m, seed=5, tombstone_fraction=0.1), fd, "vec")
        grid = time_reload(fixed, fd, fp, "vec", False, args.reps)
        emit(dict({"probe": "ragged_snapshot", "file": "b32v_b64", "route": "grid", "records": n}, **grid))
        both = time_reload(fixed, fd, fp, "vec", True, args.reps)
        emit(dict({"probe": "ragged_snapshot", "file": "b32v_b64", "route": "ragged", "records": n,
                   "ragged_over_grid": both["reload_ms"] / grid["reload_ms"],
                   "str31_var_over_grid": rag["reload_ms"] / grid["reload_ms"]}, **both))
        del fixed
        torch.cuda.empty_cache()
    blob, m = build_file(sizes[0], 7, zero_value=1 << 20)
    z = time_reload(blob, sd, sp, "vec", True, args.reps)
    emit(dict({"probe": "ragged_snapshot", "file": "str31_var + one 1 MiB zero value", "route": "ragged",
               "records": sizes[0]}, **z))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
