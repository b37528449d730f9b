"""Regular-expression search with assertions (hmse_amd.regex.Regex(assertions=True), hmse_regexa_scan / hmse_regexa_seams) over an
ingested wiki-synth store.
    python tools/regexa_bench.py [--bytes N (256 MiB)] [--seed 42] [--reps 5] [--out runs/regexa_<size>.json]
Ingests wiki-synth(seed), with log lines and dates written over it at seeded places, into a one-shard store, then measures, each with a
device sync around it (median, min and max of --reps after one warm-up):
  cost        assertion-free patterns compiled BOTH ways on the same store: count_regex through the plain entry points (hmse_regex_*:
              the reference, existing code) and through the asserting ones, and each scan and seams kernel alone by the library's device
              events (hmse_profile_read(30) / (31), reset first: the slots are shared).  The asserting scan does one more table step per
              walk and a wider filter lookup; its seams launch reach + 1 threads per chunk instead of reach - 1;
  use         `^...`, `...$` and `\\b...\\b` patterns through count_regex / find_regex, against what a user does without them:
              read_store -> .cpu() -> re.finditer(..., re.M) on the host (the counts must agree).
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

COST = [("literal", b"hzms arelep"), ("date", rb"\d{4}-\d\d-\d\d"), ("frequent", rb"[a-z]+"), ("worst", rb"[^\n]*x")]
USE = [("line_start", rb"^ERROR"), ("line_end", rb"id=\d+$"), ("word", rb"\berror\b"), ("date_word", rb"\b\d{4}-\d\d-\d\d\b")]
PLANTS = [b"\nERROR code id=7\n", b" ERROR id=12 ", b" error ", b"xerrors", b" 2024-01-31 ", b"12024-01-312"]


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


def kernel_alone(lib, call, slot, reps):
    kernel_ms(lib, ops.STAGE_FIND_SCAN)                              # reset: the slots are shared
    kernel_ms(lib, ops.STAGE_FIND_PLACE)
    lib.hmse_profile_enable(1)
    for _ in range(reps):
        call()
    lib.hmse_profile_enable(0)
    ms, n = kernel_ms(lib, slot)
    return ms / max(n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    data = corpus.wiki_synth(a.bytes, seed=a.seed)
    rng = np.random.default_rng(a.seed)
    for o in rng.integers(0, data.size - 32, max(a.bytes >> 14, 8)):   # a plant every 16 KiB on average
        s = PLANTS[int(o) % len(PLANTS)]
        data[o: o + len(s)] = np.frombuffer(s, np.uint8)
    r = ingest.ingest_shard(torch.from_numpy(data).to(dev), IngestConfig())
    store = manifest.Store([manifest.build_manifest(r)])
    del r
    torch.cuda.empty_cache()
    lib = _lib.hip_lib()
    fd = find.StoreFinder(store, dev)
    unique = int(fd.raw.numel())
    res = {"bytes": a.bytes, "decoded_unique_bytes": unique, "records": fd.n_records, "chunks": int(fd.slot.numel()), "cost": [], "use": []}
    for name, pat in COST:
        case = {"case": name, "pattern": pat.decode("latin-1")}
        for form, rx in (("plain", Regex(pat, device=dev)), ("asserting", Regex(pat, device=dev, assertions=True))):
            scan, seams = (ops.regexa_scan, ops.regexa_seams) if rx.asserting else (ops.regex_scan, ops.regex_seams)
            counts, t = timed(lambda: fd.count_regex(rx), a.reps)
            case[form] = {"n_states": rx.n_states, "n_classes": rx.n_classes, "reach": rx.reach, "occurrences": int(counts.sum()), "count_regex": t,
                          "scan_kernel_ms": kernel_alone(lib, lambda: scan(fd.raw, fd.raw_off, fd.mult, rx.rx, hits_cap=0), ops.STAGE_FIND_SCAN, a.reps),
                          "seams_kernel_ms": kernel_alone(lib, lambda: seams(fd.raw, fd.raw_off, fd.cuts, fd.slot, rx.rx, hits_cap=0), ops.STAGE_FIND_PLACE, a.reps)}
        assert case["plain"]["occurrences"] == case["asserting"]["occurrences"]
        case["asserting_over_plain"] = {k: case["asserting"][k] / max(case["plain"][k], 1e-9) for k in ("scan_kernel_ms", "seams_kernel_ms")}
        case["asserting_over_plain"]["count_regex"] = case["asserting"]["count_regex"]["median_ms"] / case["plain"]["count_regex"]["median_ms"]
        res["cost"].append(case)
        print(json.dumps(case), flush=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = read.read_store(store, dev).cpu().numpy().tobytes()
    res["read_store_to_host_ms"] = (time.perf_counter() - t0) * 1e3
    for name, pat in USE:
        rx = Regex(pat, device=dev, assertions=True)
        case = {"case": name, "pattern": pat.decode("latin-1"), "n_states": rx.n_states, "n_classes": rx.n_classes, "reach": rx.reach}
        counts, case["count_regex"] = timed(lambda: fd.count_regex(rx), a.reps)
        case["occurrences"] = int(counts.sum())
        _, case["find_regex"] = timed(lambda: fd.find_regex(rx, max_hits=1 << 26), a.reps)
        t2 = time.perf_counter()
        n_found = sum(1 for _ in re.finditer(b"(?=" + pat + b")", host, re.M))
        case["host_finditer_ms"] = (time.perf_counter() - t2) * 1e3
        assert n_found == case["occurrences"], (name, n_found, case["occurrences"])
        case["host_detour_over_find_regex"] = (res["read_store_to_host_ms"] + case["host_finditer_ms"]) / case["find_regex"]["median_ms"]
        res["use"].append(case)
        print(json.dumps(case), flush=True)
    out = a.out or os.path.join("runs", f"regexa_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
