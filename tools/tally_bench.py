"""Tally of search results (hmse_amd.find tally) over an ingested wiki-synth store.
    python tools/tally_bench.py [--bytes N (64 MiB)] [--seed 42] [--reps 3] [--out profiles/tally/tally_<size>.json]
Ingests wiki-synth(seed) with the default configuration (ingest_shard) into a one-shard store, opens a StoreFinder and measures, each
with a device sync around it (median, min and max of --reps after one warm-up), for a FREQUENT regex ([a-z]+: every lower-case word),
a RARE one (the == headings ==) and the LINES that grep finds for a common word:
  tally       StoreFinder.tally(ranges): per round one hmse_tally_keys and one hmse_tally_same call, and the torch sorts around them;
  kernels     tally_keys_kernel and tally_same_kernel alone on the same ranges, by the library's device events (hmse_profile_read(31),
              reset first: the slot is shared with the other search kernels), and their calls' wall time with a sync around each;
  sorts       the share of `tally` that is neither of the two calls: the torch plumbing (sorts, masks, bincount);
  rounds      key / compare rounds taken; ranges, distinct values, bytes covered;
  today       the same ranges on the host: text() -> .cpu() -> one bytes slice per occurrence into a collections.Counter, once; its
              counts are asserted equal to the device's, value by value.
Finding the ranges (find_regex, nonoverlapping, grep) is not part of either side.  Writes one JSON file and prints it."""
import argparse
import collections
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from hmse_amd import IngestConfig, _lib, corpus, find, ingest, manifest, ops
from hmse_amd.regex import Regex


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


def host_route(fd, start, end, ptr):
    """Today's path -> one Counter per group."""
    data, off = fd.text((start, end), max_bytes=1 << 36)
    host, off, ptr = data.cpu().numpy().tobytes(), off.tolist(), ptr.tolist()
    return [collections.Counter(host[off[i]: off[i + 1]] for i in range(ptr[j], ptr[j + 1])) for j in range(len(ptr) - 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=64 << 20)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=3)
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
    res = {"bytes": a.bytes, "decoded_unique_bytes": int(fd.raw.numel()), "chunks": int(fd.slot.numel()), "cases": []}
    tabs = (fd.raw, fd.raw_off, fd.cuts, fd.slot)
    ranges = []
    for name, pat in (("frequent", rb"[a-z]+"), ("rare", rb"== [^=\n]+ ==")):
        f = find.nonoverlapping(fd.find_regex(Regex(pat, device=dev), max_hits=1 << 28))
        ranges.append((name, pat.decode(), f.offsets, f.offsets + f.lengths, f.ptr))
    ln = fd.grep([b"the"], max_hits=1 << 28)
    ranges.append(("lines", "grep 'the'", ln.start, ln.end, ln.ptr))
    for name, what, start, end, ptr in ranges:
        n = int(start.numel())
        case = {"case": name, "what": what, "ranges": n, "bytes_covered": int((end - start).sum())}
        t, case["tally"] = timed(lambda: fd.tally((start, end, ptr)), a.reps)
        case["rounds"], case["distinct"] = t.rounds, int(t.distinct.sum())
        D = int(t.start.numel())
        s2, e2 = torch.cat([start, t.start]).contiguous(), torch.cat([end, t.end]).contiguous()      # every range against its value's representative
        rep = torch.cat([n + t.value_of, n + torch.arange(D, dtype=torch.int64, device=dev)]).contiguous()
        _, case["keys_call"] = timed(lambda: ops.tally_keys(*tabs, start, end), a.reps)
        _, case["same_call"] = timed(lambda: ops.tally_same(*tabs, s2, e2, rep), a.reps)
        case["keys_kernel_ms"] = profiled(lib, lambda: ops.tally_keys(*tabs, start, end), a.reps)
        case["same_kernel_ms"] = profiled(lib, lambda: ops.tally_same(*tabs, s2, e2, rep), a.reps)
        calls = case["rounds"] * (case["keys_call"]["median_ms"] + case["same_call"]["median_ms"])
        case["sorts_share"] = max(0.0, 1.0 - calls / max(case["tally"]["median_ms"], 1e-9))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        today = host_route(fd, start, end, ptr)
        case["today_text_cpu_counter_ms"] = (time.perf_counter() - t0) * 1e3
        case["today_over_tally"] = case["today_text_cpu_counter_ms"] / max(case["tally"]["median_ms"], 1e-9)
        # the device's values, value by value, against the host's
        vdata, voff = fd.text(t, max_bytes=1 << 36)
        vhost, voff, vptr, cnt = vdata.cpu().numpy().tobytes(), voff.tolist(), t.ptr.tolist(), t.count.tolist()
        for j, want in enumerate(today):
            got = {vhost[voff[i]: voff[i + 1]]: cnt[i] for i in range(vptr[j], vptr[j + 1])}
            assert got == dict(want) and vptr[j + 1] - vptr[j] == len(want), f"{name}: the host route and the device disagree in group {j}"
            assert cnt[vptr[j]: vptr[j + 1]] == sorted(cnt[vptr[j]: vptr[j + 1]], reverse=True)
        case["most_frequent"] = [(vhost[voff[i]: voff[i + 1]][:40].decode("latin-1"), cnt[i]) for i in range(min(3, D))]
        if name == "frequent":
            assert case["tally"]["median_ms"] < case["today_text_cpu_counter_ms"], "the device path is not faster than the host route"
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "tally", f"tally_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
