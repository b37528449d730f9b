"""Import (hmse_amd.gunzip.from_gzip) of three gzip files of one wiki-synth corpus.
    python tools/gunzip_bench.py [--bytes N (256 MiB)] [--seed 42] [--reps 5] [--out runs/gunzip_<size>.json]
Ingests wiki-synth(seed) with the default configuration into a one-shard store and builds, once:
  bgzf       the store's BGZF export (export.to_gzip(bgzf=True)): every member says how long it is — measured, not walked
  gzip       the store's plain multi-member export: one member per chunk, each walked for its length and then decoded
  level6     zlib level 6 of the same corpus in members of 64 KiB: few, long members — a member is serial inside one wavefront
For each, with a device sync around it (median, min and max of --reps after one warm-up): from_gzip's wall time and GiB/s of DECODED
bytes with the data already in HBM, and inside the same calls the time spent in its phases — candidates / measure / inflate / crc by a
synchronised host clock around ops.gzip_candidates, ops.gzip_measure, ops.l1_inflate and ops.crc32, chain = the rest (torch ops and the
read-backs).  Beside it: single-thread zlib (a chain of decompressobj(wbits=31), tests/gunzip_ref.py) over the same bytes on this
machine's CPU, once, and read.read_store of the store for scale.  Checks every import against the corpus before it times anything.
Writes one JSON file and prints it."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import gunzip_ref as ref
from hmse_amd import IngestConfig, corpus, export, gunzip, ingest, manifest, ops, read

GIB = float(1 << 30)
PHASES = {"candidates": "gzip_candidates", "measure": "gzip_measure", "inflate": "l1_inflate", "crc": "crc32"}


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def timed(fn, reps):
    fn()                                                            # warm-up
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, stats(ms)


def phased(data, dev, reps):
    """from_gzip with a synchronised clock around its four device phases -> per phase and in total, ms per repetition"""
    spent = {k: 0.0 for k in PHASES}
    real = {k: getattr(ops, fn) for k, fn in PHASES.items()}

    def wrap(k):
        def f(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = real[k](*a, **kw)
            torch.cuda.synchronize()
            spent[k] += (time.perf_counter() - t0) * 1e3
            return out
        return f
    rows = []
    try:
        for k, fn in PHASES.items():
            setattr(ops, fn, wrap(k))
        gunzip.from_gzip(data, dev)                                 # warm-up
        for _ in range(reps):
            for k in spent:
                spent[k] = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gunzip.from_gzip(data, dev)
            torch.cuda.synchronize()
            total = (time.perf_counter() - t0) * 1e3
            rows.append({**spent, "chain": total - sum(spent.values()), "total": total})
    finally:
        for k, fn in PHASES.items():
            setattr(ops, fn, real[k])
    return {k: stats([r[k] for r in rows]) for k in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    data = corpus.wiki_synth(a.bytes, seed=a.seed)
    whole = data.tobytes()
    want = torch.from_numpy(data).to(dev)
    cfg = IngestConfig()
    r = ingest.ingest_shard(want, cfg)
    store = manifest.Store([manifest.build_manifest(r)])
    del r
    torch.cuda.empty_cache()
    files = {"bgzf": export.to_gzip(store, dev, cfg, bgzf=True).data, "gzip": export.to_gzip(store, dev, cfg).data}
    step = 64 << 10
    with ThreadPoolExecutor(16) as pool:
        parts = list(pool.map(lambda o: ref.member(whole[o: o + step], 6), range(0, len(whole), step)))
    files["level6"] = torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).to(dev)
    del parts
    res = {"bytes": a.bytes, "note": "one run; host clocks around device synchronises; the data is in HBM before the clock starts"}
    _, res["read_store"] = timed(lambda: read.read_store(store, dev), a.reps)
    res["read_store"]["corpus_gibs"] = a.bytes / GIB / (res["read_store"]["median_ms"] * 1e-3)
    for name, d in files.items():
        imp = gunzip.from_gzip(d, dev)
        assert torch.equal(imp.raw, want) and imp.crc32 == zlib.crc32(whole), name
        row = {"file_bytes": int(d.numel()), "members": imp.n_members, "candidates": imp.n_candidates, "bgzf_members": imp.n_bgzf}
        del imp
        _, row["from_gzip"] = timed(lambda: gunzip.from_gzip(d, dev), a.reps)
        _, row["from_gzip_unverified"] = timed(lambda: gunzip.from_gzip(d, dev, verify=False), a.reps)
        for k in ("from_gzip", "from_gzip_unverified"):
            row[k]["raw_gibs"] = a.bytes / GIB / (row[k]["median_ms"] * 1e-3)
        row["phases_ms"] = phased(d, dev, a.reps)
        blob = d.cpu().numpy().tobytes()
        t0 = time.perf_counter()
        members = ref.chain(blob)
        t = time.perf_counter() - t0
        assert len(members) == row["members"] and sum(len(m[2]) for m in members) == a.bytes
        row["zlib_one_thread"] = {"s": t, "raw_gibs": a.bytes / GIB / t, "runs": 1}
        del members, blob
        res[name] = row
        print(name, json.dumps(row), flush=True)
    out = a.out or os.path.join("runs", f"gunzip_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
