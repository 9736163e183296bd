#!/usr/bin/env python3
"""The sharded store with variable-length values, measured in one process (one JSON line per figure;
every time is the min and the max over the repeats, after a warm-up call of the same shape):

  route   the ragged route alone (rsos_hip.device.route_columns_var) over a String -> String map of the
          shape scripts/ragged_snapshot_probe.py builds (str31 keys, values of 0..200 bytes, DATED with
          tags), as bytes read + written per second; the fixed-width route (route_columns) over a
          b16 -> b64 DATED map of the same row count; and, in the same run, the device copy rate of
          microbench/copy_rate.hip's shape (a 16-byte and a 32-byte column copied to two others)
  load    ShardedStore.load_bulk_device of the String -> String map into 4 and 8 shards on one device,
          beside one rh_store loading the same columns
  apply   ShardedStore.apply_device of `batch` rows into those maps, beside one store

    python scripts/sstore_var_probe.py [--records 10000000] [--batch 1000000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reconcile-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    import numpy as np
    import torch
    from ragged_snapshot_probe import sorted_unique_keys
    from rsos_hip import GpuFingerprintStore, RecordSchema
    from rsos_hip.device import route_columns, route_columns_var
    from rsos_hip.sharded import ShardedStore
    from rsos_hip.synth import make_records
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sch = RecordSchema.dated("str31", "var")
    out = open(a.out, "w") if a.out else None

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(fn, reps=a.reps):
        fn()  # warm: code objects, scratch, the routed copy
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return min(ms), max(ms)

    def string_map(n, seed, sort=True):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        rows, _ = sorted_unique_keys(n, g)
        n = rows.shape[0]
        if not sort:
            rows = rows[torch.randperm(n, device="cuda", generator=g)]
        vlen = torch.randint(0, 201, (n,), dtype=torch.int64, device="cuda", generator=g)
        offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        offs[1:] = torch.cumsum(vlen, 0)
        heap = torch.randint(0, 256, ((int(offs[-1]) + 3) // 4 * 4,), dtype=torch.uint8, device="cuda", generator=g)
        return {"keys": rows.contiguous(),
                "phys": torch.randint(1 << 40, 1 << 41, (n,), dtype=torch.int64, device="cuda", generator=g),
                "logical": torch.randint(0, 1 << 31, (n,), dtype=torch.int32, device="cuda", generator=g),
                "node": torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g),
                "tags": (torch.rand(n, device="cuda", generator=g) < 0.1).to(torch.uint8),
                "values": heap, "value_offsets": offs}

    cols = string_map(a.records, 7)
    n, heap_bytes = cols["keys"].shape[0], int(cols["value_offsets"][-1])
    fixed_row = 32 + 8 + 4 + 8 + 1
    emit(what="shape", records=n, batch=a.batch, schema="str31 -> var DATED + tags", heap_bytes=heap_bytes,
         mean_value=heap_bytes / n)

    # ---- the copy rate of this machine, this run --------------------------------------------------
    rows = 100_000_000
    k, f = torch.empty((rows, 16), dtype=torch.uint8, device="cuda"), torch.empty((rows, 32), dtype=torch.uint8, device="cuda")
    ko, fo = torch.empty_like(k), torch.empty_like(f)
    lo, hi = timed(lambda: (ko.copy_(k), fo.copy_(f)))
    copy_tb_s = 2 * rows * 48 / lo / 1e9
    emit(what="copy", shape="16 B + 32 B columns of 1e8 rows to two others (two device copies)", ms_min=lo, ms_max=hi,
         tb_s_best=copy_tb_s, tb_s_worst=2 * rows * 48 / hi / 1e9)
    del k, f, ko, fo

    # ---- the routes alone ------------------------------------------------------------------------
    one = GpuFingerprintStore(sch)
    maps = {g: ShardedStore(sch, [0] * g, var_values=True) for g in (4, 8)}
    load_ms = {"one": timed(lambda: one.load_bulk_device(cols), 2)}
    for g, sh in maps.items():
        load_ms[g] = timed(lambda: sh.load_bulk_device(cols), 2)
    splitters = {g: np.stack([np.frombuffer(sh._key_bytes(s), np.uint8) for s in sh.splitters]) for g, sh in maps.items()}
    for g in (4, 8):
        cap = n + 16 * g
        dst = {c: torch.empty((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device="cuda")
               for c, t in cols.items() if c not in ("values", "value_offsets")}
        dst["values"] = torch.empty_like(cols["values"])
        dst["value_offsets"] = torch.empty(cap + 1, dtype=torch.int64, device="cuda")
        lo, hi = timed(lambda: route_columns_var(sch, splitters[g], g, cols, out=dst, cap_rows=cap))
        # every fixed column read and written, the keys read twice, an offset read and written per row, the heap
        moved = n * (2 * fixed_row + 32 + 16) + 2 * heap_bytes
        emit(what="route", kind="ragged (str31 -> var)", rows=n, shards=g, ms_min=lo, ms_max=hi, bytes_moved=moved,
             tb_s_best=moved / lo / 1e9, tb_s_worst=moved / hi / 1e9, of_copy_rate_best=moved / lo / 1e9 / copy_tb_s,
             of_copy_rate_worst=moved / hi / 1e9 / copy_tb_s)
        del dst
    fsch = RecordSchema.dated("bytes16", "bytes64")
    fcols = make_records(fsch, n, seed=7, device="cuda:0", tombstone_fraction=0.05)
    frow = sum(t.nbytes for t in fcols.values()) / n
    for g in (4, 8):
        cap = n + 16 * g
        # splitters at equal steps of the first key byte (random keys: shards of nearly equal counts)
        fsp = np.ascontiguousarray(((np.arange(1, g) * 256) // g).astype(np.uint8)[:, None].repeat(16, axis=1))
        dst = {c: torch.empty((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device="cuda") for c, t in fcols.items()}
        lo, hi = timed(lambda: route_columns(fsch, fsp, g, fcols, out=dst, cap_rows=cap))
        moved = n * (2 * frow + 16)
        emit(what="route", kind="fixed (b16 -> b64)", rows=n, shards=g, ms_min=lo, ms_max=hi, bytes_moved=moved,
             tb_s_best=moved / lo / 1e9, tb_s_worst=moved / hi / 1e9, of_copy_rate_best=moved / lo / 1e9 / copy_tb_s,
             of_copy_rate_worst=moved / hi / 1e9 / copy_tb_s)
        del dst
    del fcols

    # ---- load and apply beside one store -----------------------------------------------------------
    emit(what="load", route="one rh_store, device columns", ms_min=load_ms["one"][0], ms_max=load_ms["one"][1])
    for g in (4, 8):
        emit(what="load", route="sharded, device columns", shards=g, ms_min=load_ms[g][0], ms_max=load_ms[g][1])
    batches = [string_map(a.batch, 100 + i, sort=False) for i in range(a.reps + 1)]
    for name, st in [("one rh_store, device columns", one)] + [("sharded, device columns", sh) for sh in maps.values()]:
        st.apply_device(batches[0])  # warm
        ms = []
        for b in batches[1:]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.apply_device(b)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        emit(what="apply", route=name, shards=len(getattr(st, "shards", [None])), rows=int(batches[1]["keys"].shape[0]),
             ms_min=min(ms), ms_max=max(ms))
    roots = {one.aggregate()} | {sh.aggregate() for sh in maps.values()}
    emit(what="check", same_root_everywhere=len(roots) == 1, size=one.size())
    for st in [one] + list(maps.values()):
        st.close()


if __name__ == "__main__":
    main()
