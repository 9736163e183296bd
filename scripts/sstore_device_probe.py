#!/usr/bin/env python3
"""The sharded store's device-column write side, measured in one process (one JSON line per figure):

  load    n b16 -> b64 DATED records already in HBM into 4 and 8 shards on one device
          (ShardedStore.load_bulk_device), beside one rh_store loading the same columns and beside
          the host route (rh_sstore_load of the same rows from host memory)
  apply   batches of `batch` rows (ShardedStore.apply_device) into those maps, beside one store's
          apply_device and the host route (rh_sstore_apply)
  route   the partition alone (rsos_hip.device.route_columns) for `batch` and n rows, as a fraction of
          the one-row-per-lane copy rate measured for this machine (profiles/r03s2_copy_rate.txt, rows1)

    python scripts/sstore_device_probe.py [--records 100000000] [--batch 1000000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reconcile-rs_amd"))

COPY_RATE_TB_S = 5.959  # profiles/r03s2_copy_rate.txt, "rows1"


def main():
    import numpy as np
    import torch
    from rsos_hip import GpuFingerprintStore, RecordSchema
    from rsos_hip.device import route_columns
    from rsos_hip.sharded import ShardedStore
    from rsos_hip.synth import make_records, to_host
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--host-route", type=int, default=1, help="0 to skip the host-route legs")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sch = RecordSchema.dated("bytes16", "bytes64")
    n, m = a.records, a.batch
    out = open(a.out, "w") if a.out else None

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(fn, reps=1):
        best = None
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best * 1e3

    cols = make_records(sch, n, seed=7, device="cuda:0", tombstone_fraction=0.05)
    row_bytes = sum(t.nbytes for t in cols.values()) / n
    emit(what="shape", records=n, batch=m, schema="b16->b64 DATED + tags", row_bytes=row_bytes)
    one = GpuFingerprintStore(sch)
    maps = {g: ShardedStore(sch, [0] * g) for g in (4, 8)}
    emit(what="load", route="one rh_store, device columns", ms=timed(lambda: one.load_bulk_device(cols), 2))
    for g, sh in maps.items():
        emit(what="load", route="sharded, device columns", shards=g, ms=timed(lambda: sh.load_bulk_device(cols), 2))
    hmap = None
    if a.host_route:
        hcols = to_host(cols)
        hmap = ShardedStore(sch, [0] * 4)
        emit(what="load", route="sharded, host columns (rh_sstore_load)", shards=4, ms=timed(lambda: hmap.load_bulk(hcols)))
        del hcols
    # update batches: random keys over the resident key range (nearly all new)
    for st in [one, hmap] + list(maps.values()):
        if st is not None:
            st.reserve(n + a.batches * m, m)
    batches = [make_records(sch, m, seed=100 + i, device="cuda:0", tombstone_fraction=0.05, random_keys=True)
               for i in range(a.batches + 1)]
    for name, st in [("one rh_store, device columns", one)] + [("sharded, device columns", sh) for sh in maps.values()]:
        st.apply_device(batches[0])  # warm: buffers, the routed copy
        ms = [timed(lambda b=b: st.apply_device(b)) for b in batches[1:]]
        emit(what="apply", route=name, shards=len(getattr(st, "shards", [None])), rows=m, ms_each=[round(x, 3) for x in ms],
             ms_median=float(np.median(ms)))
    if hmap is not None:
        hb = [to_host(b) for b in batches]
        ops = np.zeros(m, np.uint8)
        hmap.apply(hb[0], ops)
        ms = [timed(lambda b=b: hmap.apply(b, ops)) for b in hb[1:]]
        emit(what="apply", route="sharded, host columns (rh_sstore_apply)", shards=4, rows=m,
             ms_each=[round(x, 3) for x in ms], ms_median=float(np.median(ms)))
        hmap.close()
    roots = {one.aggregate()} | {sh.aggregate() for sh in maps.values()}
    emit(what="check", same_root_everywhere=len(roots) == 1, size=one.size())
    # the partition alone
    one.close()
    splitters = {g: np.stack([np.frombuffer(sh._key_bytes(k), np.uint8) for k in sh.splitters]) for g, sh in maps.items()}
    for sh in maps.values():
        sh.close()
    for rows, src in ((m, batches[1]), (n, cols)):
        for g in (4, 8):
            cap = rows + 16 * g
            dst = {c: torch.empty((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for c, t in src.items()}
            ms = timed(lambda: route_columns(sch, splitters[g], g, src, out=dst, cap_rows=cap), 3)
            moved = rows * (2 * row_bytes + 16)  # every column read and written, the keys read twice
            emit(what="route", rows=rows, shards=g, ms=ms, tb_s=moved / ms / 1e9,
                 of_copy_rate=moved / ms / 1e9 / COPY_RATE_TB_S)
            del dst


if __name__ == "__main__":
    main()
