"""Approximate search (hmse_amd.find count_approx / find_approx) over an ingested wiki-synth store.
    python tools/approx_bench.py [--bytes N (256 MiB)] [--seed 42] [--reps 5] [--out runs/approx_<size>.json]
Ingests wiki-synth(seed) with the default configuration (ingest_shard) into a one-shard store, then measures, each with a device sync
around it (median, min and max of --reps after one warm-up), for m in 8, 16, 64, k in 0, 2, 8 (where k < m) and P in 1, 8 patterns per
launch (slices of the corpus at random offsets):
  count_approx / find_approx   wall time and decoded unique GiB/s;
  count / find                 the exact search over the same patterns, in the same run (hmse_amd/csrc/find.hip is what it was);
  scan kernel                  approx_scan_kernel alone, by the library's device events (hmse_profile_read(30), reset first: the slot is
                               shared), count-only launches: decoded unique bytes / kernel time, ps per byte and pattern, and — given
                               --insts, the static VALU instructions per byte and pattern read off the disassembly — the fraction of
                               the VALU issue bound (256 CUs x 4 SIMDs x 16 lanes per clock at --mhz) that count implies.  One
                               figure for every case, and an assumed clock: the share is good to about +-5 %.
Writes one JSON file and prints it."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hmse_amd import IngestConfig, _lib, corpus, find, ingest, manifest, ops

GIB = float(1 << 30)
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc", "approx.hip")).read()
S = int(re.search(r"constexpr int AX_STRIP = (\d+);", _SRC).group(1))      # the scan's strip: bytes per lane and tile


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--insts", type=float, default=0.0, help="static VALU instructions per byte and pattern of the scan's strip loop")
    ap.add_argument("--mhz", type=float, default=2400.0)
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
    lanes_per_s = 256 * 4 * 16 * a.mhz * 1e6
    res = {"bytes": a.bytes, "decoded_unique_bytes": unique, "records": fd.n_records, "chunks": int(fd.slot.numel()), "insts_per_byte_pattern": a.insts,
           "valu_lane_ops_per_s": lanes_per_s, "cases": []}
    rng = np.random.default_rng(a.seed)
    gibs = lambda t: unique / GIB / (t["median_ms"] * 1e-3)
    for p in (1, 8):
        for m in (8, 16, 64):
            pats = [data[o: o + m].tobytes() for o in rng.integers(0, data.size - m, p)]
            _, t_count = timed(lambda: fd.count(pats), a.reps)
            _, t_find = timed(lambda: fd.find(pats, max_hits=1 << 26), a.reps)
            for k in (0, 2, 8):
                if k >= m:
                    continue
                case = {"P": p, "m": m, "k": k, "exact_count": t_count, "exact_find": t_find, "exact_count_gibs": gibs(t_count), "exact_find_gibs": gibs(t_find)}
                counts, case["count_approx"] = timed(lambda: fd.count_approx(pats, k), a.reps)
                case["occurrences"] = int(counts.sum())
                case["count_approx_gibs"] = gibs(case["count_approx"])
                if case["occurrences"] <= 1 << 24:
                    _, case["find_approx"] = timed(lambda: fd.find_approx(pats, k, max_hits=1 << 24), a.reps)
                    case["find_approx_gibs"] = gibs(case["find_approx"])
                flat, off = find.pack_patterns(pats)
                pat = torch.from_numpy(flat.copy()).to(dev)
                kernel_ms(lib, ops.STAGE_FIND_SCAN)
                lib.hmse_profile_enable(1)
                for _ in range(a.reps):
                    ops.approx_scan(fd.raw, fd.raw_off, fd.mult, pat, off, [k] * p, hits_cap=0)
                lib.hmse_profile_enable(0)
                ms, n = kernel_ms(lib, ops.STAGE_FIND_SCAN)
                case["scan_kernel_ms"] = ms / max(n, 1)
                case["scan_gibs"] = unique / GIB / (case["scan_kernel_ms"] * 1e-3)
                case["scan_ps_per_byte_pattern"] = case["scan_kernel_ms"] * 1e9 / unique / p
                if a.insts:
                    # every strip byte costs (S + warm-up) / S column steps of a.insts instructions each, 64 lanes per instruction
                    steps = (S + 4 * ((m + k + 2) // 4)) / S
                    bound_s = unique * p * a.insts * steps / lanes_per_s
                    case["valu_issue_bound_ms"] = bound_s * 1e3
                    case["share_of_valu_issue_bound"] = bound_s / (case["scan_kernel_ms"] * 1e-3)
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
    out = a.out or os.path.join("runs", f"approx_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
