"""Scrub, salvage and repair (hmse_amd.scrub) of an ingested wiki-synth store.
    python tools/scrub_bench.py [--bytes N (1 GiB)] [--seed 42] [--damaged 1000] [--out runs/scrub_<size>.json]
Ingests wiki-synth(seed) with the default configuration (ingest_shard) into a one-shard store, then times, each with a device sync
around it (best of 3 after a warm-up): read_store(verify=True); scrub of the clean store; scrub of a copy with `--damaged` records
each hit by one flipped byte; salvage of that copy; repair of it from a replica whose damage is disjoint.  hmse_scrub_records and
hmse_scrub_attribute are timed by the library's device events (hmse_profile_enable) over the clean scrubs.  Where the time goes: one
more clean scrub with per-phase timings (scrub(timings=...), a device sync between phases), and read_store's steps run one by one
with the same syncs (read_store_phases).  Writes one JSON file and prints it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hmse_amd import IngestConfig, _lib, corpus, gc, ingest, manifest, ops, read, scrub


def timed(fn, reps=3):
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return out, best


def read_store_phases(store, dev) -> dict:
    """read.read_store(verify=True)'s steps (StoreReader.read_all), in its order, timed one by one."""
    out = {}
    clock = gc._Clock(out)
    rd = read.StoreReader(store, dev)
    clock.lap("open")                                              # headers parsed, blob uploaded
    raw, raw_off = rd.decode(verify=False)
    clock.lap("inflate")
    cuts = read.to_device(rd.cuts, torch.int64, dev)
    data = ops.read_assemble(cuts, read.to_device(rd.slot, torch.int64, dev), raw_off, raw)
    clock.lap("assemble")
    read.verify_digests(data, cuts, read.to_device(rd.sha[rd.slot], torch.uint8, dev))
    clock.lap("sha256_verify")
    return out


def damage(store, recs, rng):
    p = scrub.plan(store)
    out = manifest.Store([manifest.Manifest(m.lba_unit, m.index, m.chunk_map, m.pointers, m.blob.copy(), m.shard, m.n_shards, m.chunk_base,
                                            m.remote_bases, m.pieces) for m in store.shards])
    for g in recs:
        s = int(p.rec_shard[g]); o = int(p.rec_off[g] - p.shard_blob[s]); L = int(p.rec_len[g])
        h = 8 if p.kind[g] == 2 else 0
        out.shards[s].blob[o + h + int(rng.integers(0, max(L - h, 1)))] ^= 0xFF
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--damaged", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = IngestConfig()
    data = corpus.wiki_synth(a.bytes, seed=a.seed)
    r = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    store = manifest.Store([manifest.build_manifest(r)])
    del r
    torch.cuda.empty_cache()
    n_rec = len(store.shards[0].index)
    res = {"bytes": a.bytes, "records": n_rec, "chunks": len(store.shards[0].chunk_map), "blob_bytes": int(store.shards[0].blob.size)}
    read.read_store(store, dev)                                    # warm-up
    _, res["read_store_verify_ms"] = timed(lambda: read.read_store(store, dev, verify=True))
    res["read_store_phases_ms"] = read_store_phases(store, dev)
    lib = _lib.hip_lib()
    lib.hmse_profile_read(ops.STAGE_SCRUB_RECORDS, None, None, 1); lib.hmse_profile_read(ops.STAGE_SCRUB_ATTRIBUTE, None, None, 1)
    scrub.scrub(store, dev)
    lib.hmse_profile_enable(1)
    rep, res["scrub_clean_ms"] = timed(lambda: scrub.scrub(store, dev))
    lib.hmse_profile_enable(0)
    import ctypes as C
    for name, st in (("scrub_records_kernel_ms", ops.STAGE_SCRUB_RECORDS), ("scrub_attribute_kernels_ms", ops.STAGE_SCRUB_ATTRIBUTE)):
        ms, n = C.c_double(0), C.c_uint64(0)
        lib.hmse_profile_read(st, C.byref(ms), C.byref(n), 1)
        res[name] = ms.value / max(n.value, 1)
    assert rep.clean
    res["scrub_phases_ms"] = {}
    scrub.scrub(store, dev, timings=res["scrub_phases_ms"])
    rng = np.random.default_rng(a.seed)
    big = np.nonzero(scrub.plan(store).rec_len > 16)[0]
    pick = rng.choice(big, 2 * a.damaged, replace=False)
    bad_a, bad_b = damage(store, pick[: a.damaged], rng), damage(store, pick[a.damaged:], rng)
    rep_a, res["scrub_damaged_ms"] = timed(lambda: scrub.scrub(bad_a, dev))
    res["damaged_roots"] = len(rep_a.roots)
    res["damaged_ranges"] = len(rep_a.ranges)
    res["damaged_bytes"] = int(rep_a.ranges[:, 1].sum()) if len(rep_a.ranges) else 0
    _, res["salvage_ms"] = timed(lambda: scrub.salvage(bad_a, dev))
    (fixed, rep_f), res["repair_replica_ms"] = timed(lambda: scrub.repair(bad_a, dev, replicas=[bad_b]))
    res["repair_identical"] = fixed.to_bytes() == store.to_bytes()
    res["scrub_over_read_store"] = res["scrub_clean_ms"] / res["read_store_verify_ms"]
    res["new_passes_share_of_scrub"] = (res["scrub_records_kernel_ms"] + res["scrub_attribute_kernels_ms"]) / res["scrub_clean_ms"]
    out = a.out or os.path.join("runs", f"scrub_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
