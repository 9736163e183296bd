"""Time the snapshot encode (rh_snapshot_encode_device, csrc/snap_encode.hip) beside the ragged
decode of the same file.

The file is scripts/ragged_snapshot_probe.py's String -> String file (str31 keys of 1..31 bytes,
values of 0..200 bytes, 10 % tombstones; --records 10000000 gives about 9.4 M entries).  It is
decoded to device columns once; the columns are encoded back and the result compared on the device
with the file's first entries_end bytes.  Then the two calls are timed in one process, alternating,
with device events around each call, after --warmup rounds, --reps times each (at least 20).
One JSON line per size: the median and min-max of each call, the encode's bytes/s counted as column
bytes read plus file bytes written, and that rate as a share of the copy rate of
profiles/r03s2_copy_rate.txt (one row per lane, read + write).
Lines go to --out (default profiles/snapshot_encode_probe.jsonl).
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("RSOS_HIP_TREE") or os.path.join(HERE, "..", "reconcile-rs_amd"))
sys.path.insert(0, HERE)
import torch  # noqa: E402
from rsos_hip import RecordSchema, _abi as A  # noqa: E402
from rsos_hip.snapshot import _encode_columns, decode_entries_device  # noqa: E402
from ragged_snapshot_probe import build_file  # noqa: E402


def copy_rate_tb_s():
    with open(os.path.join(HERE, "..", "profiles", "r03s2_copy_rate.txt")) as f:
        rows = [json.loads(line) for line in f if line.strip()]
    return next(r["tb_s"] for r in rows if r["kernel"] == "rows1")


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def probe(n, reps, warmup):
    sd = RecordSchema.dated("str31", "var")
    blob, m = build_file(n, 7)
    cols, info = decode_entries_device(sd, blob, "vec", ragged=True)
    end = info.entries_end
    heap, offs = cols["values"]
    heap = torch.cat([heap, torch.zeros(-heap.numel() % 4, dtype=torch.uint8, device="cuda")])  # whole words
    cols["values"] = (heap, offs)
    c, rows, _, held = _encode_columns(sd, cols)
    out = torch.zeros(end + 64, dtype=torch.uint8, device="cuda")
    s = sd.c()
    form = A.FORM_VEC | A.FORM_RAGGED
    L = A.lib()
    # the decode's outputs, allocated once
    dk = {k: torch.empty_like(cols[k]) for k in ("keys", "phys", "logical", "node", "tags")}
    dheap, doffs = torch.empty((blob.numel() + 3) // 4 * 4, dtype=torch.uint8, device="cuda"), torch.empty_like(offs)
    dvar = A.VarValues(dheap.data_ptr(), doffs.data_ptr(), dheap.numel())
    dc = A.Columns(*[dk[k].data_ptr() for k in ("keys", "phys", "logical", "node", "tags")], C.addressof(dvar))
    einfo, dinfo = A.SnapshotInfo(), A.SnapshotInfo()

    def encode():
        A.check(L.rh_snapshot_encode_device(C.byref(s), form, C.byref(c), rows, out.data_ptr(), end, C.byref(einfo),
                                            None), "rh_snapshot_encode_device")

    def decode():
        A.check(L.rh_snapshot_decode_device(C.byref(s), form, blob.data_ptr(), blob.numel(), C.byref(dc), rows,
                                            C.byref(dinfo), None), "rh_snapshot_decode_device")
    encode()
    torch.cuda.synchronize()
    same = bool(torch.equal(out[:end], blob[:end])) and not bool(out[end:].any())
    assert same, "the encoded bytes differ from the file"
    assert (einfo.entries, einfo.tombstones, einfo.entries_end) == (m, info.tombstones, end)
    null = torch.cuda.default_stream()
    times = {"encode": [], "decode": []}
    for r in range(warmup + reps):
        for name, fn in (("encode", encode), ("decode", decode)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(null)
            fn()
            b.record(null)
            b.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b))
    col_bytes = rows * (32 + 8 + 4 + 8 + 1) + 8 * (rows + 1) + int(offs[rows])
    enc, dec = stats(times["encode"]), stats(times["decode"])
    tb_s = (col_bytes + end) / (enc["median_ms"] * 1e-3) / 1e12
    del held
    return {"probe": "snapshot_encode", "file": "str31_var", "records": n, "entries": m, "file_bytes": end,
            "column_bytes": col_bytes, "reps": reps, "bit_exact": same,
            "encode_ms": enc["median_ms"], "encode_min_ms": enc["min_ms"], "encode_max_ms": enc["max_ms"],
            "decode_ms": dec["median_ms"], "decode_min_ms": dec["min_ms"], "decode_max_ms": dec["max_ms"],
            "encode_over_decode": enc["median_ms"] / dec["median_ms"],
            "encode_tb_s": tb_s, "copy_rate_tb_s": copy_rate_tb_s(), "share_of_copy_rate": tb_s / copy_rate_tb_s()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="10000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "snapshot_encode_probe.jsonl"))
    args = ap.parse_args()
    lines = []
    for n in (int(x) for x in args.records.split(",")):
        line = probe(n, max(args.reps, 20), args.warmup)
        print(json.dumps(line), flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
