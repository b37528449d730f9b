"""Substitute / redact (hmse_amd.find substitute, redact; hmse_subst_apply) over an ingested wiki-synth store, against the two routes
that existed before it.
    python tools/subst_bench.py [--bytes N (64 MiB)] [--seed 42] [--reps 5] [--host-max-edits 20000000] [--out profiles/subst/subst_bench.json]
Ingests wiki-synth(seed) with the default configuration into a one-shard store, opens a StoreFinder and measures two shapes of edit list,
each in literal mode (a 10-byte replacement) and in fill mode:
  sparse      one 12-byte edit per 4 KiB of corpus;
  dense       every run of ASCII letters replaced (the runs are found with torch on the corpus itself: finding them is no part of any route).
Per shape and mode, with device events around each call, one warm-up, then --reps rounds in which the routes ALTERNATE:
  apply       ops.subst_apply alone (the three kernels of one hmse_subst_apply call) on prepared edits and out_off;
  substitute  StoreFinder.substitute / redact: the merge, the checks, out_off by cumsum, then the call;
  scatter     route (2) of before: text() over the kept ranges (hmse_lines_gather), then torch scatters of the kept bytes and of the
              replacement bytes through int64 indices as long as the output;
  host        route (1) of before, wall clock, once: read_store -> .cpu() -> a splice in Python (b"".join over slices) -> upload; left
              out, and said so, above --host-max-edits edits (a Python loop over 10^8 edits measures the interpreter);
  copy        a plain device copy of the output's size, for scale.
`rw_GBps` is (bytes read + bytes written) / time with both taken as the output's size.  The new path's output is held against the
per-position definition of include/hmse_subst.h, computed in torch from read_store's corpus at 2^24 random positions and around 2^31
and 2^32 (`sampled_mismatches`: count and first position; asserted 0 for `apply`), and the other routes' outputs are compared with it
byte for byte (`first_difference_from_apply`, -1: none; recorded, not asserted: a route of before may fail at a size it was never run at).
Appends to one JSON file keyed by the corpus size and prints each case as it is measured."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from hmse_amd import IngestConfig, corpus, find, ingest, manifest, ops, read


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def summary(ms, total):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms), "rw_GBps": 2 * total / (med * 1e-3) / 1e9}


def out_offsets(start, end, rlen, n_bytes):
    off = torch.zeros(start.numel() + 1, dtype=torch.int64, device=start.device)
    torch.cumsum(rlen - (end - start), 0, out=off[1:])
    off[:-1] += start
    off[-1] += n_bytes
    return off


def scatter_route(fd, start, end, repl, fill, out_off, total):
    """Route (2): the kept ranges through text(), then two scatters through int64 indices."""
    dev, n = fd.dev, start.numel()
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    kstart, kend = torch.cat([z, end]), torch.cat([start, z + fd.n_bytes])
    kept, koff = fd.text((kstart, kend), max_bytes=1 << 40)
    rlen = end - start if fill else torch.full((n,), repl.numel(), dtype=torch.int64, device=dev)
    kout = torch.cat([z, out_off[:-1] + rlen])                                   # where each kept range begins in the output
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    idx = torch.repeat_interleave(kout - koff[:-1], kend - kstart) + torch.arange(kept.numel(), dtype=torch.int64, device=dev)
    out[idx] = kept
    roff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(rlen, 0, out=roff[1:])
    within = torch.arange(int(roff[-1]), dtype=torch.int64, device=dev) - torch.repeat_interleave(roff[:-1], rlen)
    ridx = torch.repeat_interleave(out_off[:-1], rlen) + within
    out[ridx] = repl[0].expand(ridx.numel()) if fill else repl[within]
    return out


def host_route(store, dev, start, end, repl, fill):
    """Route (1): the corpus to the host, a splice in Python, the result back."""
    host = read.read_store(store, dev).cpu().numpy().tobytes()
    parts, at = [], 0
    for s, e in zip(start, end):
        parts.append(host[at:s])
        parts.append(repl * (e - s) if fill else repl)
        at = e
    parts.append(host[at:])
    import numpy as np
    out = torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    return out


def sample_check(out, c, start, out_off, rlen, repl, fill, n_samples=1 << 24):
    """`out` against the per-position form of include/hmse_subst.h at random positions and around 2^31 and 2^32, in torch: an answer that
    does not pass through any of the routes, and no tensor of more than n_samples elements.  -> (mismatches, the first one or -1)"""
    dev, n, total, N = out.device, start.numel(), out.numel(), c.numel()
    if total == 0:
        return 0, -1
    p = torch.randint(0, total, (n_samples,), dtype=torch.int64, device=dev)
    for edge in (1 << 31, 1 << 32):
        if total > edge - 4096:
            p = torch.cat([p, torch.arange(edge - 4096, min(edge + 4096, total), dtype=torch.int64, device=dev)])
    p = torch.cat([p, torch.arange(max(total - 4096, 0), total, dtype=torch.int64, device=dev)])
    i = torch.searchsorted(out_off[:n].contiguous(), p, right=True) - 1         # the last edit with out_off[i] <= p, -1: none
    ic = i.clamp(min=0)
    in_rep = (i >= 0) & (p < out_off[ic] + rlen[ic]) if n else torch.zeros_like(p, dtype=torch.bool)
    start_ext = torch.cat([start, torch.tensor([N], dtype=torch.int64, device=dev)])
    q = (p - (out_off[i + 1] - start_ext[i + 1])).clamp(0, max(N - 1, 0))       # p - D
    from_rep = repl[0].expand(p.numel()) if fill else repl[(p - out_off[ic]).clamp(0, repl.numel() - 1)]
    want = torch.where(in_rep, from_rep, c[q] if N else from_rep)
    bad = out[p] != want
    k = int(bad.sum())
    return k, (int(p[bad].min()) if k else -1)


def first_difference(a, b, piece=1 << 28):
    if a.numel() != b.numel():
        return min(a.numel(), b.numel())
    for at in range(0, a.numel(), piece):
        d = a[at: at + piece] != b[at: at + piece]
        if bool(d.any()):
            return at + int(torch.nonzero(d)[0])
    return -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=64 << 20)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max-edits", type=int, default=20_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subst", "subst_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    data = corpus.wiki_synth(a.bytes, seed=a.seed)
    r = ingest.ingest_shard(torch.from_numpy(data).to(dev), IngestConfig())
    store = manifest.Store([manifest.build_manifest(r)])
    del r, data
    torch.cuda.empty_cache()
    fd = find.StoreFinder(store, dev)
    N = fd.n_bytes
    res = {"bytes": a.bytes, "decoded_unique_bytes": int(fd.raw.numel()), "chunks": int(fd.slot.numel()), "cases": []}
    tabs = (fd.raw, fd.raw_off, fd.cuts, fd.slot)
    # the edit lists
    s = torch.arange(0, N - 4096, 4096, dtype=torch.int64, device=dev) + 1000
    shapes = [("sparse", s, s + 12)]
    c = read.read_store(store, dev)
    low = c | 0x20
    alpha = (low >= 97) & (low <= 122)
    del low
    edge = torch.zeros(N + 1, dtype=torch.int8, device=dev)
    edge[:N] = alpha.to(torch.int8)
    edge[1:] -= alpha.to(torch.int8)                                              # +1 where a run begins, -1 one behind its end
    shapes.append(("dense", torch.nonzero(edge == 1).reshape(-1), torch.nonzero(edge == -1).reshape(-1)))
    del alpha, edge
    torch.cuda.empty_cache()
    for shape, start, end in shapes:
        n = int(start.numel())
        for fill in (False, True):
            repl_b = b"*" if fill else b"[REDACTED]"
            repl = torch.tensor(list(repl_b), dtype=torch.uint8, device=dev)
            rep_off = torch.tensor([0, len(repl_b)], dtype=torch.int64, device=dev)
            sel = torch.zeros(n, dtype=torch.int64, device=dev)
            rlen = end - start if fill else torch.full((n,), len(repl_b), dtype=torch.int64, device=dev)
            out_off = out_offsets(start, end, rlen, N)
            total = int(out_off[-1])
            case = {"shape": shape, "mode": "fill" if fill else "literal", "edits": n, "bytes_replaced": int((end - start).sum()), "bytes_out": total}
            routes = {"apply": lambda: ops.subst_apply(*tabs, start, end, sel, repl, rep_off, out_off, total, fill),
                      "substitute": lambda: (fd.redact if fill else fd.substitute)((start, end), repl_b, max_bytes=1 << 40).data,
                      "scatter": lambda: scatter_route(fd, start, end, repl, fill, out_off, total)}
            src = torch.empty(total, dtype=torch.uint8, device=dev)
            routes["copy"] = lambda: torch.empty_like(src).copy_(src)
            outs = {k: fn() for k, fn in routes.items()}                         # warm-up, and the outputs to compare
            torch.cuda.synchronize()
            # the new path against the definition at 2^24 sampled positions; the other routes against the new path, byte for byte
            want = outs["apply"]
            case["sampled_mismatches"] = {k: sample_check(outs[k], c, start, out_off, rlen, repl, fill) for k in ("apply", "substitute", "scatter")}
            case["first_difference_from_apply"] = {k: first_difference(want, outs[k]) for k in ("substitute", "scatter")}
            print(json.dumps({"shape": shape, "fill": fill, "checks": [case["sampled_mismatches"], case["first_difference_from_apply"]]}), flush=True)
            assert case["sampled_mismatches"]["apply"] == (0, -1), f"{shape}: hmse_subst_apply's output is not the definition's"
            del outs
            ms = {k: [] for k in routes}
            for _ in range(a.reps):                                              # the routes alternate
                for k, fn in routes.items():
                    ms[k].append(event_ms(fn)[1])
            for k in routes:
                case[k] = summary(ms[k], total)
            if n <= a.host_max_edits:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = host_route(store, dev, start.tolist(), end.tolist(), repl_b, fill)
                case["host"] = {"wall_ms": (time.perf_counter() - t0) * 1e3, "reps": 1}
                assert torch.equal(got, want), f"{shape}: the host route disagrees"
                del got
            else:
                case["host"] = {"skipped": f"{n} edits exceed --host-max-edits = {a.host_max_edits}: a Python loop over them measures the interpreter"}
            case["scatter_over_apply"] = case["scatter"]["median_ms"] / case["apply"]["median_ms"]
            case["apply_share_of_copy_rate"] = case["apply"]["rw_GBps"] / case["copy"]["rw_GBps"]
            del want, src, routes
            torch.cuda.empty_cache()
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    all_runs = {}
    if os.path.exists(a.out):
        all_runs = json.load(open(a.out))
    all_runs[f"{a.bytes >> 20}MiB"] = res
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(all_runs, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
