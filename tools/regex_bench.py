"""Regular-expression search (hmse_amd.regex, StoreFinder.find_regex) over an ingested wiki-synth store.
    python tools/regex_bench.py [--bytes N (256 MiB)] [--seed 42] [--reps 5] [--out runs/regex_<size>.json]
Ingests wiki-synth(seed), with dates written over it at seeded places, into a one-shard store, then measures, each with a device sync
around it (median, min and max of --reps after one warm-up):
  open        StoreFinder(store): every record decoded once (and verified);
  count/find  count_regex / find_regex for a pure literal, a rare structured pattern (a date), a frequent one ([a-z]+) and the worst
              case ([^\\n]*x: every start walks to the end of its line or 256 bytes);
  scan kernel regex_scan_kernel alone, by the library's device events (hmse_profile_read(30), reset first: the slot is shared):
              decoded unique bytes / kernel time, and its share of the achievable HBM read rate (6.3 TB/s, MI355X);
  literal     StoreFinder.count / find and find_scan_kernel with the same literal on the same store — the ratio a reader looks for first;
  today       read_store -> .cpu() -> re.finditer with a lookahead (every start) per pattern, once.
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

from hmse_amd import IngestConfig, _lib, corpus, find, ingest, manifest, ops, read
from hmse_amd.regex import Regex

HBM_READ_BPS = 6.3e12      # achievable HBM read rate of an MI355X (8 TB/s peak)
LITERAL = b"hzms arelep"
CASES = [("literal", LITERAL), ("date", rb"\d{4}-\d\d-\d\d"), ("frequent", rb"[a-z]+"), ("worst", rb"[^\n]*x")]


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


def scan_alone(lib, call, reps, unique):
    kernel_ms(lib, ops.STAGE_FIND_SCAN)                              # reset: the slot is shared
    kernel_ms(lib, ops.STAGE_FIND_PLACE)
    lib.hmse_profile_enable(1)
    for _ in range(reps):
        call()
    lib.hmse_profile_enable(0)
    ms, n = kernel_ms(lib, ops.STAGE_FIND_SCAN)
    k = ms / max(n, 1)
    return {"scan_kernel_ms": k, "scan_bytes_per_s": unique / (k * 1e-3), "scan_share_of_hbm_read": unique / (k * 1e-3) / HBM_READ_BPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = IngestConfig()
    data = corpus.wiki_synth(a.bytes, seed=a.seed)
    rng = np.random.default_rng(a.seed)
    for o in rng.integers(0, data.size - 16, max(a.bytes >> 16, 8)):   # a date every 64 KiB on average
        data[o: o + 10] = np.frombuffer(b"%04d-%02d-%02d" % (1900 + o % 200, 1 + o % 12, 1 + o % 28), np.uint8)
    r = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    store = manifest.Store([manifest.build_manifest(r)])
    del r
    torch.cuda.empty_cache()
    lib = _lib.hip_lib()
    fd, t_open = timed(lambda: find.StoreFinder(store, dev), max(1, a.reps // 2))
    unique = int(fd.raw.numel())
    res = {"bytes": a.bytes, "decoded_unique_bytes": unique, "records": fd.n_records, "chunks": int(fd.slot.numel()),
           "resident_bytes": fd.resident_bytes, "open": t_open, "hbm_read_bps_achievable": HBM_READ_BPS, "cases": []}
    for name, pat in CASES:
        rx = Regex(pat, device=dev)
        case = {"case": name, "pattern": pat.decode("latin-1"), "n_states": rx.n_states, "n_classes": rx.n_classes, "reach": rx.reach}
        counts, case["count_regex"] = timed(lambda: fd.count_regex(rx), a.reps)
        case["occurrences"] = int(counts.sum())
        if case["occurrences"] <= 1 << 26:
            _, case["find_regex"] = timed(lambda: fd.find_regex(rx, max_hits=1 << 26), a.reps)
        case.update(scan_alone(lib, lambda: ops.regex_scan(fd.raw, fd.raw_off, fd.mult, rx.rx, hits_cap=0), a.reps, unique))
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    # the same literal through the literal kernels, on the same store
    lit = {"pattern": LITERAL.decode()}
    counts, lit["count"] = timed(lambda: fd.count([LITERAL]), a.reps)
    _, lit["find"] = timed(lambda: fd.find([LITERAL]), a.reps)
    assert int(counts[0]) == res["cases"][0]["occurrences"]
    pat = torch.from_numpy(np.frombuffer(LITERAL, np.uint8).copy()).to(dev)
    lit.update(scan_alone(lib, lambda: ops.find_scan(fd.raw, fd.raw_off, fd.mult, pat, [0, len(LITERAL)], hits_cap=0), a.reps, unique))
    res["find_literal"] = lit
    res["literal_regex_over_find"] = {"count": res["cases"][0]["count_regex"]["median_ms"] / lit["count"]["median_ms"],
                                      "scan_kernel": res["cases"][0]["scan_kernel_ms"] / lit["scan_kernel_ms"]}
    # what a user does today
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = read.read_store(store, dev).cpu().numpy().tobytes()
    t1 = time.perf_counter()
    today = {"read_store_to_host_ms": (t1 - t0) * 1e3, "finditer_ms": {}}
    for name, pat in CASES[:2] + ([CASES[2]] if a.bytes <= 64 << 20 else []):
        t2 = time.perf_counter()
        n_found = sum(1 for _ in re.finditer(b"(?=" + pat + b")", host))
        today["finditer_ms"][name] = (time.perf_counter() - t2) * 1e3
        assert n_found == [c for c in res["cases"] if c["case"] == name][0]["occurrences"]
    res["today"] = today
    out = a.out or os.path.join("runs", f"regex_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
