"""Exact search (hmse_amd.find) over an ingested wiki-synth store.
    python tools/find_bench.py [--bytes N (1 GiB)] [--seed 42] [--reps 5] [--out runs/find_<size>.json]
Ingests wiki-synth(seed) with the default configuration (ingest_shard) into a one-shard store, then measures, each with a device sync
around it (median, min and max of --reps after one warm-up):
  open        StoreFinder(store): every record decoded once (and verified);
  count/find  for P in 1, 8, 32 patterns of m in 4, 16, 256 bytes, each with RARE patterns (slices of the corpus at random offsets) and
              FREQUENT ones (the most common m-byte strings of a sample of the corpus; m = 256: repeats of the rare ones);
  scan kernel find_scan_kernel alone, by the library's device events (hmse_profile_read(30), reset first: the slot is shared with the
              DELTA encode kernels of the ingest): decoded unique bytes / kernel time, and its share of the achievable HBM read rate
              (6.3 TB/s, MI355X);
  l2 hash     l2_hash_kernel (the project's other one-read-per-byte kernel) over the same decoded bytes, in the same process
              (hmse_profile_read(2) around ops.l2_cdc);
  today       read_store -> .cpu() -> a bytes.find loop per pattern, the same patterns (P = 8, m = 16, rare), once.
Writes one JSON file and prints it."""
import argparse
import collections
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hmse_amd import IngestConfig, _lib, corpus, find, ingest, manifest, ops, read

HBM_READ_BPS = 6.3e12      # achievable HBM read rate of an MI355X (8 TB/s peak)


def timed(fn, reps):
    fn()                                                            # warm-up
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def kernel_ms(lib, slot):
    ms, n = C.c_double(0), C.c_uint64(0)
    lib.hmse_profile_read(slot, C.byref(ms), C.byref(n), 1)
    return ms.value, int(n.value)


def patterns(data: np.ndarray, p: int, m: int, frequent: bool, rng) -> list:
    b = data[: 8 << 20].tobytes()
    if frequent and m < 256:
        top = collections.Counter(b[o: o + m] for o in range(0, len(b) - m, 7)).most_common(p)
        return [w for w, _ in top]
    offs = rng.integers(0, data.size - m, 4 if frequent else p)
    pats = [data[o: o + m].tobytes() for o in offs]
    return (pats * p)[:p]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = IngestConfig()
    data = corpus.wiki_synth(a.bytes, seed=a.seed)
    r = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    store = manifest.Store([manifest.build_manifest(r)])
    del r
    torch.cuda.empty_cache()
    lib = _lib.hip_lib()
    fd, t_open = timed(lambda: find.StoreFinder(store, dev), max(1, a.reps // 2))
    unique = int(fd.raw.numel())
    res = {"bytes": a.bytes, "decoded_unique_bytes": unique, "records": fd.n_records, "chunks": int(fd.slot.numel()),
           "resident_bytes": fd.resident_bytes, "open": t_open, "hbm_read_bps_achievable": HBM_READ_BPS, "cases": []}
    rng = np.random.default_rng(a.seed)
    for p in (1, 8, 32):
        for m in (4, 16, 256):
            for frequent in (False, True):
                pats = patterns(data, p, m, frequent, rng)
                case = {"P": p, "m": m, "patterns": "frequent" if frequent else "rare"}
                counts, case["count"] = timed(lambda: fd.count(pats), a.reps)
                case["occurrences"] = int(counts.sum())
                if case["occurrences"] <= 1 << 26:
                    _, case["find"] = timed(lambda: fd.find(pats, max_hits=1 << 26), a.reps)
                # the scan kernel alone (count-only launches: the filter and the verify, no hit list)
                flat, off = find.pack_patterns(pats)
                pat = torch.from_numpy(flat.copy()).to(dev)
                kernel_ms(lib, ops.STAGE_FIND_SCAN)
                lib.hmse_profile_enable(1)
                for _ in range(a.reps):
                    ops.find_scan(fd.raw, fd.raw_off, fd.mult, pat, off, hits_cap=0)
                lib.hmse_profile_enable(0)
                ms, n = kernel_ms(lib, ops.STAGE_FIND_SCAN)
                case["scan_kernel_ms"] = ms / max(n, 1)
                case["scan_bytes_per_s"] = unique / (case["scan_kernel_ms"] * 1e-3)
                case["scan_share_of_hbm_read"] = case["scan_bytes_per_s"] / HBM_READ_BPS
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
    # l2_hash_kernel over the same bytes
    ops.l2_cdc(fd.raw, cfg)
    kernel_ms(lib, ops.STAGE_L2)
    lib.hmse_profile_enable(1)
    for _ in range(a.reps):
        ops.l2_cdc(fd.raw, cfg)
    lib.hmse_profile_enable(0)
    ms, n = kernel_ms(lib, ops.STAGE_L2)
    res["l2_hash_kernel_ms"] = ms / max(n, 1)
    res["l2_hash_ps_per_byte"] = res["l2_hash_kernel_ms"] * 1e9 / unique
    one = [c for c in res["cases"] if c["P"] == 1 and c["patterns"] == "rare"]
    res["scan_p1_ps_per_byte"] = {str(c["m"]): c["scan_kernel_ms"] * 1e9 / unique for c in one}
    # what a user does today
    pats = patterns(data, 8, 16, False, np.random.default_rng(a.seed))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = read.read_store(store, dev).cpu().numpy().tobytes()
    t1 = time.perf_counter()
    n_found = 0
    for q in pats:
        o = host.find(q)
        while o >= 0:
            n_found += 1
            o = host.find(q, o + 1)
    t2 = time.perf_counter()
    res["today"] = {"P": 8, "m": 16, "read_store_to_host_ms": (t1 - t0) * 1e3, "bytes_find_loop_ms": (t2 - t1) * 1e3, "occurrences": n_found}
    assert n_found == int(fd.count(pats).sum())
    out = a.out or os.path.join("runs", f"find_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
