"""Order of search results (hmse_amd.find sort) over an ingested wiki-synth store.
    python tools/order_bench.py [--bytes N (64 MiB)] [--seed 42] [--reps 3] [--out profiles/order/order_<size>.json]
Ingests wiki-synth(seed) with the default configuration (ingest_shard) into a one-shard store, opens a StoreFinder and measures, each
with a device sync around it (median, min and max of --reps after one warm-up), for the three range sets of tools/tally_bench.py — a
FREQUENT regex ([a-z]+: every lower-case word), a RARE one (the == headings ==) and the LINES that grep finds for a common word:
  sort        StoreFinder.sort(ranges): per round one hmse_order_keys and at most one hmse_order_lcp call, and the torch sorts around them;
  no_skip     the same call with _skip=False (depth + 7 a round, no hmse_order_lcp, max_rounds = what the longest range needs), timed
              likewise; its result is asserted equal to sort's;
  kernels     order_keys_kernel and order_lcp_kernel summed over the rounds of one more run, by the library's device events
              (hmse_profile_read(31), reset before every call: the slot is shared with the other search kernels), the calls' wall time with
              a sync around each, and the ranges keyed and compared over all rounds;
  plumbing    the share of that run that is neither of the two calls: the torch sorts, masks and scatters;
  rounds      key / LCP rounds taken; ranges, distinct texts, bytes covered;
  today       the same ranges on the host: text() -> .cpu() -> sorted() over one bytes slice per range, once; its order is asserted equal
              to the device's, position by position.
Finding the ranges (find_regex, nonoverlapping, grep) is not part of either side.  Writes one JSON file and prints it."""
import argparse
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


def instrumented(lib, fd, start, end, group, G):
    """One run of find.order_ranges whose two calls are bracketed: device events of the one kernel each launches, wall time with a sync."""
    tabs = (fd.raw, fd.raw_off, fd.cuts, fd.slot)
    acc = {"keys_kernel_ms": 0.0, "lcp_kernel_ms": 0.0, "keys_call_ms": 0.0, "lcp_call_ms": 0.0, "ranges_keyed": 0, "ranges_compared": 0}

    def bracket(which, n, fn):
        kernel_ms(lib, ops.STAGE_FIND_PLACE)
        lib.hmse_profile_enable(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        acc[which + "_call_ms"] += (time.perf_counter() - t0) * 1e3
        lib.hmse_profile_enable(0)
        acc[which + "_kernel_ms"] += kernel_ms(lib, ops.STAGE_FIND_PLACE)[0]
        acc["ranges_keyed" if which == "keys" else "ranges_compared"] += n
        return out
    keys = lambda s, e, d: bracket("keys", s.numel(), lambda: ops.order_keys(*tabs, s, e, d))
    lcp = lambda s, e, rep, frm: bracket("lcp", s.numel(), lambda: ops.order_lcp(*tabs, s, e, rep, frm))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    find.order_ranges(start, end, group, G, keys, lcp)
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) * 1e3
    acc["run_ms"] = total
    acc["plumbing_share"] = max(0.0, 1.0 - (acc["keys_call_ms"] + acc["lcp_call_ms"]) / max(total, 1e-9))
    return acc


def host_route(fd, start, end, ptr):
    """Today's path -> the input indices in order, group after group."""
    data, off = fd.text((start, end), max_bytes=1 << 36)
    host, off, ptr, st = data.cpu().numpy().tobytes(), off.tolist(), ptr.tolist(), start.tolist()
    order = []
    for j in range(len(ptr) - 1):
        order += sorted(range(ptr[j], ptr[j + 1]), key=lambda i: (host[off[i]: off[i + 1]], st[i], i))
    return order


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
    ranges = []
    for name, pat in (("frequent", rb"[a-z]+"), ("rare", rb"== [^=\n]+ ==")):
        f = find.nonoverlapping(fd.find_regex(Regex(pat, device=dev), max_hits=1 << 28))
        ranges.append((name, pat.decode(), f.offsets, f.offsets + f.lengths, f.ptr))
    ln = fd.grep([b"the"], max_hits=1 << 28)
    ranges.append(("lines", "grep 'the'", ln.start, ln.end, ln.ptr))
    for name, what, start, end, ptr in ranges:
        n = int(start.numel())
        longest = int((end - start).max()) if n else 0
        case = {"case": name, "what": what, "ranges": n, "bytes_covered": int((end - start).sum()), "longest_range": longest}
        s, case["sort"] = timed(lambda: fd.sort((start, end, ptr)), a.reps)
        case["rounds"], case["distinct"] = s.rounds, int(s.distinct.sum())
        s2, case["no_skip"] = timed(lambda: fd.sort((start, end, ptr), max_rounds=longest // 7 + 2, _skip=False), a.reps)     # a round per seven bytes
        case["no_skip"]["rounds"] = s2.rounds
        assert torch.equal(s.index, s2.index) and torch.equal(s.first, s2.first), f"{name}: the skip changes the result"
        G = int(ptr.numel()) - 1
        group = torch.repeat_interleave(torch.arange(G, dtype=torch.int64, device=dev), ptr[1:] - ptr[:-1])
        case["kernels"] = instrumented(lib, fd, start.contiguous(), end.contiguous(), group, G)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        today = host_route(fd, start, end, ptr)
        case["today_text_cpu_sorted_ms"] = (time.perf_counter() - t0) * 1e3
        case["today_over_sort"] = case["today_text_cpu_sorted_ms"] / max(case["sort"]["median_ms"], 1e-9)
        assert s.index.tolist() == today, f"{name}: the host route and the device disagree"
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "order", f"order_{a.bytes >> 20}MiB.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
