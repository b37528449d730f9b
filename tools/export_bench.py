"""Export (hmse_amd.export to_gzip / crc32) of an ingested wiki-synth store.
    python tools/export_bench.py [--bytes N (256 MiB)] [--seed 42] [--reps 5] [--out runs/export_<size>.json]
Ingests wiki-synth(seed) with the default configuration (ingest_shard) into a one-shard store, then measures, each with a device sync
around it (median, min and max of --reps after one warm-up):
  to_gzip (gzip and BGZF), export.crc32, read.read_store   wall time and GiB/s of CORPUS bytes, in the same run on the same store;
  the CRC kernel alone     crc32_kernel by the library's device events (hmse_profile_read(0)) over the decoded unique records, and over
                           the same number of bytes of one constant byte: GB/s of unique bytes;
  the member kernel alone  gzip_members_kernel by hmse_profile_read(1);
  re-encoding              ops.l1_deflate of the DELTA records without dictionaries, as to_gzip calls it: its share of to_gzip — the
                           known cost of gzip having no dictionaries;
  sizes                    output bytes against the store's blob bytes.
Checks the first export with Python's gzip against the corpus before it times anything.  Writes one JSON file and prints it."""
import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hmse_amd import KIND_DELTA, IngestConfig, _lib, corpus, export, ingest, manifest, ops, read

GIB = float(1 << 30)


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
    return ms.value / max(int(n.value), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    data = corpus.wiki_synth(a.bytes, seed=a.seed)
    cfg = IngestConfig()
    r = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    store = manifest.Store([manifest.build_manifest(r)])
    del r
    torch.cuda.empty_cache()
    lib = _lib.hip_lib()
    x = export.to_gzip(store, dev, cfg)
    assert x.crc32 == zlib.crc32(data.tobytes()) and gzip.decompress(x.tobytes()) == data.tobytes()
    rd = read.StoreReader(store, dev)
    raw, raw_off = rd.decode(verify=False)
    unique, blob = int(raw.numel()), int(sum(m.blob.size for m in store.shards))
    delta_ids = torch.from_numpy(np.nonzero(rd.kind == KIND_DELTA)[0].astype(np.int64)).to(dev)
    res = {"bytes": a.bytes, "decoded_unique_bytes": unique, "records": len(rd.kind), "chunks": len(rd.slot), "delta_records": int(delta_ids.numel()),
           "delta_raw_bytes": int(rd.raw_len[rd.kind == KIND_DELTA].sum()), "blob_bytes": blob, "gzip_bytes": int(x.data.numel())}
    del x
    gibs = lambda t: a.bytes / GIB / (t["median_ms"] * 1e-3)
    z, res["to_gzip_bgzf"] = timed(lambda: export.to_gzip(store, dev, cfg, bgzf=True), a.reps)
    res["bgzf_bytes"] = int(z.data.numel())
    del z
    for name, fn in (("to_gzip", lambda: export.to_gzip(store, dev, cfg)), ("to_gzip_unverified", lambda: export.to_gzip(store, dev, cfg, verify=False)),
                     ("crc32", lambda: export.crc32(store, dev)), ("read_store", lambda: read.read_store(store, dev))):
        _, res[name] = timed(fn, a.reps)
    for name in ("to_gzip", "to_gzip_bgzf", "to_gzip_unverified", "crc32", "read_store"):
        res[name]["corpus_gibs"] = gibs(res[name])
    _, res["reencode"] = timed(lambda: ops.l1_deflate(raw, raw_off, cfg, chunk_ids=delta_ids, base=None), a.reps)
    res["reencode_share_of_to_gzip"] = res["reencode"]["median_ms"] / res["to_gzip"]["median_ms"]
    _, res["decode"] = timed(lambda: rd.decode(verify=False), a.reps)
    res["output_over_blob"] = res["gzip_bytes"] / blob
    # the kernels alone, by the library's event pairs
    const = torch.full_like(raw, 0x65)
    for name, buf in (("random", raw), ("constant", const)):
        kernel_ms(lib, ops.STAGE_EXPORT_CRC)
        lib.hmse_profile_enable(1)
        for _ in range(a.reps):
            crc = ops.crc32(buf, raw_off)
        lib.hmse_profile_enable(0)
        ms = kernel_ms(lib, ops.STAGE_EXPORT_CRC)
        res["crc_kernel_" + name] = {"ms": ms, "unique_gb_per_s": unique / 1e9 / (ms * 1e-3)}
    kernel_ms(lib, ops.STAGE_EXPORT_MEMBERS)
    lib.hmse_profile_enable(1)
    for _ in range(a.reps):
        export.to_gzip(store, dev, cfg, verify=False)
    lib.hmse_profile_enable(0)
    ms = kernel_ms(lib, ops.STAGE_EXPORT_MEMBERS)
    res["members_kernel"] = {"ms": ms, "output_gb_per_s": res["gzip_bytes"] / 1e9 / (ms * 1e-3)}
    out = a.out or os.path.join("runs", f"export_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
