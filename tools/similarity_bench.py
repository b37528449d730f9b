"""Near-duplicate search (hmse_amd.similarity) on an ingested wiki-synth corpus.
    python tools/similarity_bench.py [--bytes N (1 GiB)] [--seed 42] [--top-k 8] [--out profiles/r5/similarity_<size>.json]
Ingests wiki-synth(seed) with the default configuration (ingest_shard), builds the index (stored keys by hmse_l4_lsh, then
hmse_l4_index_build), runs the self-join (near_duplicates) and a query of a 256 MiB slice of the corpus with about 0.5 % of its bytes
edited.  Every phase is timed with a device sync around it (best of 3 for the search phases, after a warm-up).  Reported: ms per phase,
the work bound sum w_i and max w_i (w_i = sum over bands of the query's key-run lengths, counted here with torch.searchsorted: a
diagnostic, not the product path), candidates and hits, and the signature bytes the score kernel gathers (one 512-byte row per run
entry) per second against the 8 TB/s HBM peak.  Writes one JSON file and prints it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hmse_amd import IngestConfig, corpus, ingest, ops, similarity

HBM_PEAK = 8.0e12


def timed(fn, reps=1):
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return out, best


def work(ix, keys_q):
    """(sum w_i, max w_i) of queries with band keys keys_q [q, bands]."""
    w = torch.zeros(keys_q.shape[0], dtype=torch.int64, device=keys_q.device)
    for b in range(ix.bands):
        sk = ix.sorted_keys[b].to(torch.int64) & 0xFFFFFFFF
        k = keys_q[:, b].to(torch.int64) & 0xFFFFFFFF
        w += torch.searchsorted(sk, k, right=True) - torch.searchsorted(sk, k, right=False)
    return int(w.sum()), int(w.max()) if w.numel() else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--top-k", type=int, default=8)
    ap.add_argument("--query-bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = IngestConfig()
    t0 = time.perf_counter()
    host = corpus.wiki_synth(a.bytes, seed=a.seed)
    gen_s = time.perf_counter() - t0
    data = torch.from_numpy(host).to(dev)
    res, ingest_ms = timed(lambda: ingest.ingest_shard(data, cfg, want_stats=False))
    del data
    sig = res.sig.contiguous()
    n = int(sig.shape[0])
    keys, keys_ms = timed(lambda: ops.l4_lsh(sig, cfg)[0])
    (sk, si), index_ms = timed(lambda: ops.l4_index_build(keys), 3)
    ix = similarity.SimilarityIndex(sig, cfg)
    selfj, self_ms = timed(lambda: ix.near_duplicates(top_k=a.top_k), 3)
    sw, mw = work(ix, ix.keys)
    # query: a slice with about 0.5 % of its bytes changed
    qlen = min(a.query_bytes, a.bytes)
    rng = np.random.default_rng(a.seed)
    q0 = int(rng.integers(0, a.bytes - qlen + 1)) // cfg.seg_size * cfg.seg_size
    q = host[q0: q0 + qlen].copy()
    pos = rng.integers(0, qlen, qlen // 200)
    q[pos] = rng.integers(97, 123, pos.size, dtype=np.uint8)
    qd = torch.from_numpy(q).to(dev)
    (qcuts, qsig), qsig_ms = timed(lambda: ix.query_signatures(qd), 3)
    qkeys, qkeys_ms = timed(lambda: ops.l4_lsh(qsig, ix.search_cfg)[0], 3)
    qhits, qsearch_ms = timed(lambda: ix.search(qsig, a.top_k, 0, keys_q=qkeys), 3)
    qsw, qmw = work(ix, qkeys)
    _, qtotal_ms = timed(lambda: ix.query(qd, top_k=a.top_k), 1)
    gb = lambda w, ms: w * 512 / (ms * 1e-3)
    out = {
        "bytes": a.bytes, "seed": a.seed, "corpus_gen_s": round(gen_s, 2), "stored_chunks": n, "bands": ix.bands, "top_k": a.top_k,
        "signature_bytes": n * 512, "ingest_ms": round(ingest_ms, 1),
        "index": {"keys_ms": round(keys_ms, 3), "index_build_ms": round(index_ms, 3)},
        "self_join": {"ms": round(self_ms, 3), "sum_w": sw, "max_w": mw, "candidates": int(selfj.n_candidates.sum()), "hits": int(selfj.n_hits.sum()),
                      "queries_with_hits": int((selfj.n_hits > 0).sum()), "max_candidates": int(selfj.n_candidates.max()) if n else 0,
                      "gather_bytes_per_s": round(gb(sw, self_ms)), "fraction_of_hbm_peak": round(gb(sw, self_ms) / HBM_PEAK, 4)},
        "query": {"bytes": qlen, "offset": q0, "edited_bytes": int(pos.size), "chunks": int(qsig.shape[0]), "chunk_sign_ms": round(qsig_ms, 3),
                  "keys_ms": round(qkeys_ms, 3), "search_ms": round(qsearch_ms, 3), "total_ms": round(qtotal_ms, 3), "sum_w": qsw, "max_w": qmw,
                  "candidates": int(qhits.n_candidates.sum()), "hits": int(qhits.n_hits.sum()),
                  "queries_with_hits": int((qhits.n_hits > 0).sum()), "top1_score_128": int((qhits.scores[:, 0] == 128).sum()),
                  "gather_bytes_per_s": round(gb(qsw, qsearch_ms)), "fraction_of_hbm_peak": round(gb(qsw, qsearch_ms) / HBM_PEAK, 4)},
        "library": os.environ.get("HMSE_LIB_VARIANT") or "default",
    }
    path = a.out or os.path.join("profiles", "r5", f"similarity_{a.bytes >> 20}MiB{'_' + out['library'] if out['library'] != 'default' else ''}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
