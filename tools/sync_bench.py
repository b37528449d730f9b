"""Replication (hmse_amd.sync) between two ingested wiki-synth stores.
    python tools/sync_bench.py [--bytes N (1 GiB)] [--replace 0.05] [--swaps 3] [--seed 42] [--reps 5] [--out runs/sync_<size>.json]
Store A: wiki-synth(seed), the default configuration (ingest_shard), one shard.  Store B: the same corpus with the share --replace of
its 4 MiB segments replaced by other text (wiki-synth(seed + 1)) and --swaps pairs of segments exchanged.  Measures, each with a device
sync around it (median, min and max of --reps after one warm-up):
  diff / make_patch / apply_patch     A -> B (apply with verify=False and, once, with verify=True);
  match kernel    sync_match_kernel alone, by the library's device events (hmse_profile_read(19), reset first: the slot is shared with a
                  DEFLATE dictionary-job class of the ingest): 2 x compared bytes / kernel time, and its share of the HBM rate bench.py's
                  roofline uses (8 TB/s);
  patch bytes     against len(B.to_bytes()): what travels instead of the whole store;
  numpy           the plain reference on the same inputs (tests/sync_ref.py: digest dictionary, bytes ==, slice assignment), once.
Writes one JSON file and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from hmse_amd import IngestConfig, _lib, corpus, ingest, manifest, ops, sync

HBM_PEAK_BPS = 8.0e12      # bench.py HBM_PEAK_GBPS


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--replace", type=float, default=0.05)
    ap.add_argument("--swaps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = IngestConfig()
    data_a = corpus.wiki_synth(a.bytes, seed=a.seed)
    n_seg = a.bytes // cfg.seg_size
    rng = np.random.default_rng(a.seed)
    data_b = data_a.copy()
    other = corpus.wiki_synth(a.bytes, seed=a.seed + 1)
    replaced = rng.choice(n_seg, max(1, int(round(a.replace * n_seg))), replace=False) if n_seg else np.zeros(0, np.int64)
    for s in replaced:
        data_b[s * cfg.seg_size:(s + 1) * cfg.seg_size] = other[s * cfg.seg_size:(s + 1) * cfg.seg_size]
    for _ in range(a.swaps if n_seg >= 2 else 0):
        i, j = rng.choice(n_seg, 2, replace=False)
        si, sj = slice(i * cfg.seg_size, (i + 1) * cfg.seg_size), slice(j * cfg.seg_size, (j + 1) * cfg.seg_size)
        data_b[si], data_b[sj] = data_b[sj].copy(), data_b[si].copy()
    del other

    def store(d):
        r = ingest.ingest_shard(torch.from_numpy(d).to(dev), cfg)
        m = manifest.build_manifest(r)
        del r
        torch.cuda.empty_cache()
        return m
    A, B = store(data_a), store(data_b)
    lib = _lib.hip_lib()
    res = {"bytes": a.bytes, "segments": int(n_seg), "segments_replaced": int(len(replaced)), "segment_pairs_swapped": a.swaps,
           "records_A": len(A.index), "records_B": len(B.index), "store_bytes_A": len(A.to_bytes()), "store_bytes_B": len(B.to_bytes()),
           "hbm_peak_bps": HBM_PEAK_BPS}
    d, res["diff"] = timed(lambda: sync.diff(A, B, dev), a.reps)
    res["diff_result"] = {"chunks": int(len(d.present)), "present": int(d.present.sum()), "new_ranges": int(len(d.new_ranges)), "shared_bytes": d.shared_bytes,
                          "new_bytes": d.new_bytes, "new_unique_bytes": d.new_unique_bytes, "unreferenced_records": int(len(d.unreferenced))}
    lib.hmse_profile_read(ops.STAGE_SYNC_MATCH, None, None, 1)
    lib.hmse_profile_enable(1)
    p, res["make_patch"] = timed(lambda: sync.make_patch(A, B, dev), a.reps)
    lib.hmse_profile_enable(0)
    ms, n = C.c_double(0), C.c_uint64(0)
    lib.hmse_profile_read(ops.STAGE_SYNC_MATCH, C.byref(ms), C.byref(n), 1)
    kernel_ms = ms.value / max(int(n.value), 1)
    in_a = {bytes(x) for x in np.ascontiguousarray(A.index["sha256"])}
    n_cand = sum(bytes(x) in in_a for x in np.ascontiguousarray(B.index["sha256"]))
    # compared bytes: the streams of the records whose candidate has the same length (an upper bound of what the kernel reads: it
    # leaves a record at the first 1 KiB trip that differs) — the copied ones in full
    res["match_kernel"] = {"launches": int(n.value), "ms": kernel_ms, "records": len(B.index), "candidates": n_cand, "copied_bytes": p.copied_bytes,
                           "bytes_read_at_least": 2 * p.copied_bytes,
                           "bytes_per_s": 2 * p.copied_bytes / (kernel_ms * 1e-3) if kernel_ms else None,
                           "share_of_hbm_peak": 2 * p.copied_bytes / (kernel_ms * 1e-3) / HBM_PEAK_BPS if kernel_ms else None}
    blob = p.to_bytes()
    res["patch"] = {"bytes": len(blob), "literal_bytes": p.literal_bytes, "copied_bytes": p.copied_bytes, "records_literal": int((p.src < 0).sum()),
                    "records_copied": int((p.src >= 0).sum()), "share_of_store_B": len(blob) / res["store_bytes_B"]}
    out_m, res["apply_patch_no_verify"] = timed(lambda: sync.apply_patch(A, p, dev, verify=False), a.reps)
    assert out_m.to_bytes() == B.to_bytes()
    _, res["apply_patch_verify"] = timed(lambda: sync.apply_patch(A, p, dev, verify=True), 1)
    # the plain reference on the same inputs
    import dataclasses
    import sync_ref as ref
    t0 = time.perf_counter()
    rd = ref.diff(A, B)
    t1 = time.perf_counter()
    rp = ref.plan(A, B)
    t2 = time.perf_counter()
    rb = ref.apply(A, dataclasses.replace(B, blob=np.zeros(0, np.uint8)), B.blob.size, rp["src"], rp["literals"], rp["delta_hdrs"])
    t3 = time.perf_counter()
    assert np.array_equal(rd["present"], d.present) and np.array_equal(rp["src"], p.src) and rb.to_bytes() == B.to_bytes()
    res["numpy_reference"] = {"diff_ms": (t1 - t0) * 1e3, "plan_ms": (t2 - t1) * 1e3, "apply_ms": (t3 - t2) * 1e3}
    out = a.out or os.path.join("runs", f"sync_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
