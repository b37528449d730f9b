"""Dictionary search (hmse_amd.find.PatternSet, StoreFinder.count_set / find_set) over an ingested wiki-synth store.
    python tools/findset_bench.py [--bytes N (1 GiB)] [--seed 42] [--reps 5] [--sizes 32,1024,32768,262144] [--out runs/findset_<size>.json]
Ingests wiki-synth(seed) with the default configuration into a one-shard store and opens a StoreFinder.  For every dictionary size P —
word n-grams of 8..64 bytes, half cut out of the corpus at word starts, half absent (the same bytes with one byte replaced by '#') —
it measures, each with a device sync around it (median, min and max of --reps after one warm-up):
  build        the host time of PatternSet(patterns, device) (once);
  count_set    one scan and one seam pass for the whole dictionary;  find_set: the same plus the hit lists, place and the sorts;
  scan kernel  findset_scan_kernel alone, by the library's device events (hmse_profile_read(30), reset first: the slot is shared with
               hmse_find_scan and the DELTA encode kernels): decoded unique bytes / kernel time, and its share of the HBM read rate
               bench.py's roofline uses;
  filter       the share of the positions of a 16 MiB sample of the decoded records whose window passes the bitmap (torch restatement);
  grouped      StoreFinder.count on the same patterns (ceil(P / 32) scan + seam passes) for P <= 1024, measured; for larger P its
               time per group at P = 1024 times ceil(P / 32), marked "extrapolated".
Writes one JSON file and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hmse_amd import IngestConfig, _lib, corpus, find, ingest, manifest, ops

HBM_READ_BPS = 6.3e12      # achievable HBM read rate of an MI355X (8 TB/s peak): bench.py's roofline figure


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


def dictionary(data: np.ndarray, p: int, rng) -> list:
    """p distinct-looking word n-grams of 8..64 bytes: even ones from the corpus (starting behind a blank), odd ones absent."""
    b = data[: min(data.size, 256 << 20)].tobytes()
    out = []
    while len(out) < p:
        o = b.find(b" ", int(rng.integers(0, len(b) - 200))) + 1
        m = int(rng.integers(8, 65))
        w = b[o: o + m]
        if len(w) < m:
            continue
        if len(out) % 2:
            k = int(rng.integers(0, m))
            w = w[:k] + b"#" + w[k + 1:]
        out.append(w)
    return out


def filter_pass_rate(fd, ps, sample=16 << 20) -> float:
    raw = fd.raw[: min(int(fd.raw.numel()), sample)].to(torch.int64)
    key = raw[:-3] | (raw[1:-2] << 8) | (raw[2:-1] << 16) | (raw[3:] << 24)
    bit = ((key * ops.FINDSET_HASH) & 0xFFFFFFFF) >> (32 - ops.FINDSET_BITMAP_BITS)
    bm = ps.set.bitmap.to(torch.int64) & 0xFFFFFFFF
    return float((((bm[bit >> 5] >> (bit & 31)) & 1).sum() / bit.numel()).item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="32,1024,32768,262144")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    data = corpus.wiki_synth(a.bytes, seed=a.seed)
    r = ingest.ingest_shard(torch.from_numpy(data).to(dev), IngestConfig())
    store = manifest.Store([manifest.build_manifest(r)])
    del r
    torch.cuda.empty_cache()
    lib = _lib.hip_lib()
    fd = find.StoreFinder(store, dev)
    unique = int(fd.raw.numel())
    res = {"bytes": a.bytes, "decoded_unique_bytes": unique, "records": fd.n_records, "chunks": int(fd.slot.numel()),
           "hbm_read_bps_achievable": HBM_READ_BPS, "cases": []}
    rng = np.random.default_rng(a.seed)
    per_group_ms = None
    for p in [int(v) for v in a.sizes.split(",")]:
        pats = dictionary(data, p, rng)
        t0 = time.perf_counter()
        ps = find.PatternSet(pats, False, dev)
        torch.cuda.synchronize()
        case = {"P": p, "unique": ps.n_unique, "entries": ps.n_entries, "dir_bits": ps.dir_bits, "set_resident_bytes": ps.resident_bytes,
                "build_host_ms": (time.perf_counter() - t0) * 1e3, "filter_pass_rate": filter_pass_rate(fd, ps)}
        counts, case["count_set"] = timed(lambda: fd.count_set(ps), a.reps)
        case["occurrences"] = int(counts.sum())
        if case["occurrences"] <= 1 << 26:
            _, case["find_set"] = timed(lambda: fd.find_set(ps, max_hits=1 << 26), a.reps)
        kernel_ms(lib, ops.STAGE_FIND_SCAN)
        lib.hmse_profile_enable(1)
        for _ in range(a.reps):
            ops.findset_scan(fd.raw, fd.raw_off, fd.mult, ps.set, hits_cap=0)
        lib.hmse_profile_enable(0)
        ms, n = kernel_ms(lib, ops.STAGE_FIND_SCAN)
        case["scan_kernel_ms"] = ms / max(n, 1)
        case["scan_bytes_per_s"] = unique / (case["scan_kernel_ms"] * 1e-3)
        case["scan_share_of_hbm_read"] = case["scan_bytes_per_s"] / HBM_READ_BPS
        groups = -(-p // find.GROUP)
        if p <= 1024:
            old, case["grouped_count"] = timed(lambda: fd.count(pats), max(1, a.reps // 2 if p > 32 else a.reps))
            assert torch.equal(old, counts), "count_set and the grouped count disagree"
            case["grouped_count"]["how"] = "measured"
            per_group_ms = case["grouped_count"]["median_ms"] / groups
        elif per_group_ms is not None:
            case["grouped_count"] = {"median_ms": per_group_ms * groups, "how": f"extrapolated: {per_group_ms:.3f} ms per group x {groups} groups"}
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    out = a.out or os.path.join("runs", f"findset_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
