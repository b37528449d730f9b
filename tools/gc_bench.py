"""Garbage collection of dropped segments (hmse_amd.gc) against a fresh ingest of the same remainder.
    python tools/gc_bench.py [store MiB (1024)] [corpus (wikipedia)]
Ingests the corpus into a one-shard store (default config: 4 MiB segments) and its band-table sidecar, then collects two cases —
10 % of the segments dropped, spread out (every 10th), and the oldest 25 % dropped (retention) — each with and without the sidecar.
Every run is checked by identity (manifest bytes == fresh ingest of the remainder, packed) and timed per phase (a device sync
between phases): plan, decode, minhash, lsh, reencode, gather, pack (build_manifest), sidecar (hmse_band_tables_write); the gather
KERNEL's GB/s (hmse_profile event pair around the launch) counts its bytes read + written.
The fresh ingest is timed the same way (ingest_shard + build_manifest).  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hmse_amd import IngestConfig, _lib, bandtable, corpus, gc, ingest, manifest, ops

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E, 8 TB/s


def fresh(data_np, r_so, cfg, dev):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ingest.ingest_shard(torch.from_numpy(data_np).to(dev), cfg, seg_off=torch.from_numpy(r_so).to(dev))
    m = manifest.build_manifest(res)
    torch.cuda.synchronize()
    return m, (time.perf_counter() - t0) * 1e3


def main():
    mib = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    name = sys.argv[2] if len(sys.argv) > 2 else "wikipedia"
    dev = torch.device("cuda:0")
    cfg = IngestConfig()
    data = corpus.load(name, mib << 20, seed=42)[0]
    res = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    store = manifest.build_manifest(res)
    side = bandtable.write_band_tables(res.band_keys.cpu().numpy(), cfg.band_bits, signatures=res.sig.cpu().numpy())
    del res
    so = gc.store_seg_off(store, cfg)
    n_seg = len(so) - 1
    cases = {"spread_10pct": list(range(0, n_seg, 10)), "oldest_25pct": list(range(n_seg // 4))}
    gc.drop_segments(store, cases["spread_10pct"], cfg, dev, band_tables=side)          # warm-up (kernel loads, allocator)
    out = {"store_mib": mib, "corpus": name, "segments": n_seg, "chunks": int(len(store.chunk_map)), "stored": int(len(store.index)),
           "hbm_peak_gbs": HBM_PEAK_GBS, "cases": {}}
    for cname, drop in cases.items():
        keep = [i for i in range(n_seg) if i not in set(drop)]
        r = np.concatenate([data[so[i]: so[i + 1]] for i in keep])
        r_so = np.concatenate([[0], np.cumsum([so[i + 1] - so[i] for i in keep])]).astype(np.int64)
        want, t_fresh = fresh(r, r_so, cfg, dev)
        wb = want.to_bytes()
        row = {"dropped_segments": len(drop), "remainder_mib": round(r.size / 2**20, 1), "fresh_ingest_ms": round(t_fresh, 1)}
        for with_side in (True, False):
            tm = {}
            lib = _lib.hip_lib()
            kms, launches = C.c_double(), C.c_uint64()
            lib.hmse_profile_enable(1)
            lib.hmse_profile_read(ops.STAGE_RECORD_GATHER, C.byref(kms), C.byref(launches), 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m, _, st = gc.drop_segments(store, drop, cfg, dev, band_tables=side if with_side else None, timings=tm)
            total = (time.perf_counter() - t0) * 1e3
            lib.hmse_profile_read(ops.STAGE_RECORD_GATHER, C.byref(kms), C.byref(launches), 1)
            lib.hmse_profile_enable(0)
            ok = m.to_bytes() == wb
            gb = tm.pop("gather_bytes", 0)
            k_ms = max(kms.value, 1e-6)
            row["sidecar" if with_side else "no_sidecar"] = {
                "identical": ok, "total_ms": round(total, 1), "vs_fresh": round(total / t_fresh, 3),
                "phases_ms": {k: round(v, 2) for k, v in tm.items()},
                "gather_kernel_ms": round(k_ms, 3), "gather_bytes": gb, "gather_gbs": round(gb / k_ms / 1e6, 1),
                "gather_pct_of_peak": round(100 * gb / k_ms / 1e6 / HBM_PEAK_GBS, 1),
                "stats": st}
        out["cases"][cname] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
