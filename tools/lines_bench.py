"""Lines of a hit (hmse_amd.find lines / text) over an ingested wiki-synth store.
    python tools/lines_bench.py [--bytes N (1 GiB)] [--seed 42] [--reps 5] [--out runs/lines_<size>.json]
Ingests wiki-synth(seed) with the default configuration (ingest_shard) into a one-shard store, opens a StoreFinder and measures, each
with a device sync around it (median, min and max of --reps after one warm-up), for a RARE pattern (a 16-byte slice of the corpus) and
a FREQUENT one (the common word of a sample whose count lies nearest to a million), at (before, after) = (0, 0) and (2, 2):
  lines       StoreFinder.lines(found): one hmse_lines_extent call and the torch sorts that group the extents;
  text        StoreFinder.text(lines): the prefix sum and one hmse_lines_gather call;
  kernels     lines_extent_kernel and lines_gather_kernel alone, by the library's device events (hmse_profile_read(31), reset first:
              the slot is shared with hmse_find_place, the seam kernels and the DELTA encode kernels);
  looked at   the bytes the extent kernel looks at per hit (from its answers: both walks, the delimiters that end them included);
  today       the same hits on the host: read_store -> .cpu() -> bytes.rfind / bytes.find per hit (and per line of context), once; its
              extents are asserted equal to the device's.
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


def profiled(lib, fn, reps):
    """Mean device time of the one kernel `fn` brackets in slot 31."""
    kernel_ms(lib, ops.STAGE_FIND_PLACE)
    lib.hmse_profile_enable(1)
    for _ in range(reps):
        fn()
    lib.hmse_profile_enable(0)
    ms, n = kernel_ms(lib, ops.STAGE_FIND_PLACE)
    return ms / max(n, 1)


def host_extents(host: bytes, offsets, before: int, after: int):
    """Today's path: bytes.rfind / bytes.find per hit and per line of context."""
    n, out_s, out_e = len(host), [], []
    for o in offsets:
        s = o
        for _ in range(before + 1):
            s = host.rfind(b"\n", 0, s)
            if s < 0:
                break
        e = o - 1
        for _ in range(after + 1):
            e = host.find(b"\n", e + 1)
            if e < 0:
                e = n
                break
        out_s.append(s + 1)
        out_e.append(e)
    return out_s, out_e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
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
    rng = np.random.default_rng(a.seed)
    o = int(rng.integers(0, data.size - 16))
    sample = data[: 4 << 20].tobytes()
    words = [w for w, _ in collections.Counter(sample.split()).most_common(200) if len(w) >= 3]
    counts = fd.count(words).tolist()
    frequent = words[min(range(len(words)), key=lambda i: abs(counts[i] - 1_000_000))]
    res = {"bytes": a.bytes, "decoded_unique_bytes": int(fd.raw.numel()), "chunks": int(fd.slot.numel()), "newlines_per_byte": sample.count(b"\n") / len(sample),
           "cases": []}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = read.read_store(store, dev).cpu().numpy().tobytes()
    res["today_read_store_to_host_ms"] = (time.perf_counter() - t0) * 1e3
    for name, pat in (("rare", data[o: o + 16].tobytes()), ("frequent", frequent)):
        found = fd.find([pat], max_hits=1 << 26)
        n = int(found.offsets.numel())
        for b, aft in ((0, 0), (2, 2)):
            case = {"pattern": name, "bytes_of_pattern": len(pat), "hits": n, "before": b, "after": aft}
            ln, case["lines"] = timed(lambda: fd.lines(found, before=b, after=aft), a.reps)
            (txt, off), case["text"] = timed(lambda: fd.text(ln, max_bytes=1 << 34), a.reps)
            case["extents"], case["text_bytes"], case["cut"] = int(ln.start.numel()), int(txt.numel()), int((ln.flags != 0).sum())
            case["extent_kernel_ms"] = profiled(lib, lambda: ops.lines_extent(fd.raw, fd.raw_off, fd.cuts, fd.slot, found.offsets, 0x0A, b, aft, 1 << 16), a.reps)
            case["gather_kernel_ms"] = profiled(lib, lambda: ops.lines_gather(fd.raw, fd.raw_off, fd.cuts, fd.slot, ln.start, ln.end, off, int(off[-1])), a.reps)
            s, e, f, _ = ops.lines_extent(fd.raw, fd.raw_off, fd.cuts, fd.slot, found.offsets, 0x0A, b, aft, 1 << 16)
            looked = (found.offsets - s) + ((s > 0) & ((f & 1) == 0)) + (e - found.offsets) + ((e < fd.n_bytes) & ((f & 2) == 0))
            case["bytes_looked_at_per_hit"] = float(looked.sum()) / max(n, 1)
            case["gather_bytes_per_s"] = case["text_bytes"] / max(case["gather_kernel_ms"] * 1e-3, 1e-12)
            offs = found.offsets.tolist()
            t0 = time.perf_counter()
            hs, he = host_extents(host, offs, b, aft)
            t1 = time.perf_counter()
            parts = [host[x:y] for x, y in sorted(set(zip(hs, he)))]
            case["today_rfind_find_loop_ms"], case["today_slices_ms"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
            assert case["cut"] or (hs == s.tolist() and he == e.tolist()), "the host path and the device disagree"
            assert case["cut"] or b"".join(parts) == txt.cpu().numpy().tobytes()
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    out = a.out or os.path.join("runs", f"lines_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
