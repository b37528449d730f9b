"""Garbage collection of a SHARDED store (hmse_amd.gc, N > 1 shards) against a fresh sharded ingest of the same remainder.
    python tools/gc_sharded_bench.py [store MiB (1024)] [shards (4)] [corpus (wikipedia)] [--shard-local]
Ingests the corpus into an N-shard store with ingest_shards_local (default config: 4 MiB segments; global L4 unless --shard-local)
and its per-shard band-table sidecars, then collects the two cases of tools/gc_bench.py — 10 % of the segments dropped, spread out
(every 10th global segment), and the oldest 25 % dropped — with the sidecars.  Every run is checked by identity (store bytes and
sidecars == fresh sharded ingest of the remainder) and timed per phase (a device sync between phases): plan, lsh, decode, reencode,
gather, pack (build_manifest of every shard + merge_manifests), sidecar (the N sidecars, hmse_band_tables_write).
The fresh ingest is timed the same way (ingest_shards_local + build_manifest + merge_manifests).
Also times the sidecars of the collected store both ways: bandtable.write_band_tables (numpy, from host copies of the keys and
signatures, the copies included) and the kernel (hmse_band_tables_write, device events; GB/s of bytes written).
Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hmse_amd import IngestConfig, bandtable, corpus, gc, ingest, manifest, ops


def sharded(parts, sos, cfg, dev, global_l4):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rs = ingest.ingest_shards_local([torch.from_numpy(p).to(dev) for p in parts], cfg, global_l4=global_l4,
                                    seg_offs=None if sos is None else [torch.from_numpy(s).to(dev) for s in sos])
    store = manifest.merge_manifests([manifest.build_manifest(r, i, len(rs)) for i, r in enumerate(rs)])
    torch.cuda.synchronize()
    return store, rs, (time.perf_counter() - t0) * 1e3


def sidecar_times(keys, sigs, cfg):
    """(numpy ms incl. host copies, kernel ms by device events, bytes written) over the N sidecars."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = [bandtable.write_band_tables(k.cpu().numpy(), cfg.band_bits, signatures=s.cpu().numpy()) for k, s in zip(keys, sigs)]
    t_np = (time.perf_counter() - t0) * 1e3
    for k, s in zip(keys, sigs):                                  # warm-up
        ops.band_tables_write(k, s, cfg.band_bits)
    ms, nbytes = 0.0, 0
    for k, s, w in zip(keys, sigs, want):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ops.band_tables_write(k, s, cfg.band_bits)          # (includes its one host sync: the size)
        e1.record()
        torch.cuda.synchronize()
        ms += e0.elapsed_time(e1)
        nbytes += out.numel()
        assert out.cpu().numpy().tobytes() == w
    return t_np, ms, nbytes


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    global_l4 = "--shard-local" not in sys.argv
    mib = int(args[0]) if len(args) > 0 else 1024
    n = int(args[1]) if len(args) > 1 else 4
    name = args[2] if len(args) > 2 else "wikipedia"
    dev = torch.device("cuda:0")
    cfg = IngestConfig()
    data = corpus.load(name, mib << 20, seed=42)[0]
    per = -(-(data.size // n) // cfg.seg_size) * cfg.seg_size   # shard cuts on segment boundaries
    parts = [data[i * per: min(data.size, (i + 1) * per)] for i in range(n)]
    store, rs, _ = sharded(parts, None, cfg, dev, global_l4)
    sides = [bandtable.write_band_tables(r.band_keys.cpu().numpy(), cfg.band_bits, signatures=r.sig.cpu().numpy()) for r in rs]
    del rs
    sos, _, seg_base = gc.shard_segments(store, cfg)
    n_seg = int(seg_base[-1])
    cases = {"spread_10pct": list(range(0, n_seg, 10)), "oldest_25pct": list(range(n_seg // 4))}
    gc.drop_segments(store, cases["spread_10pct"], cfg, dev, band_tables=sides, global_l4=global_l4)      # warm-up
    out = {"store_mib": mib, "shards": n, "global_l4": global_l4, "corpus": name, "segments": n_seg,
           "chunks": int(sum(len(m.chunk_map) for m in store.shards)), "stored": int(sum(len(m.index) for m in store.shards)),
           "cross_shard_pointers": int(sum(((m.chunk_map["kind"] == 1) & (m.chunk_map["shard"] != m.shard)).sum() for m in store.shards)),
           "remote_dictionaries": int(sum(m.n_remote() for m in store.shards)), "cases": {}}
    for cname, drop in cases.items():
        per_shard = gc.split_segments(seg_base, drop)
        rem, r_sos = [], []
        for p, so, d in zip(parts, sos, per_shard):
            keep = [i for i in range(len(so) - 1) if i not in set(d)]
            rem.append(np.concatenate([p[so[i]: so[i + 1]] for i in keep]) if keep else p[:0])
            r_sos.append(np.concatenate([[0], np.cumsum([so[i + 1] - so[i] for i in keep])]).astype(np.int64) if keep else np.zeros(2, np.int64))
        want, rs, t_fresh = sharded(rem, r_sos, cfg, dev, global_l4)
        want_sides = [bandtable.write_band_tables(r.band_keys.cpu().numpy(), cfg.band_bits, signatures=r.sig.cpu().numpy()) for r in rs]
        t_np, k_ms, k_bytes = sidecar_times([r.band_keys for r in rs], [r.sig for r in rs], cfg)
        del rs
        tm = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m, got_sides, st = gc.drop_segments(store, drop, cfg, dev, band_tables=sides, global_l4=global_l4, timings=tm)
        total = (time.perf_counter() - t0) * 1e3
        tm.pop("gather_bytes", None)
        out["cases"][cname] = {
            "dropped_segments": len(drop), "remainder_mib": round(sum(r.size for r in rem) / 2**20, 1), "fresh_ingest_ms": round(t_fresh, 1),
            "identical": m.to_bytes() == want.to_bytes() and got_sides == want_sides, "total_ms": round(total, 1),
            "vs_fresh": round(total / t_fresh, 3), "phases_ms": {k: round(v, 2) for k, v in tm.items()},
            "sidecar_numpy_ms": round(t_np, 1), "sidecar_kernel_ms": round(k_ms, 3), "sidecar_bytes": k_bytes,
            "sidecar_kernel_gbs": round(k_bytes / max(k_ms, 1e-6) / 1e6, 1),
            "stats": {k: v for k, v in st.items() if k != "per_shard"}, "per_shard": st["per_shard"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
