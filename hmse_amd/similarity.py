"""Near-duplicate search over a store's MinHash/LSH index (Broder 1997; README.md:1373 "MinHash Agreement: 108 / 128 = 0.844 ≈
Jaccard", the band S-curve of README.md:2229-2256).

Every store already carries a 128-hash MinHash signature per stored chunk (L4).  A SimilarityIndex holds those signatures in HBM,
their band keys under a SEARCH banding of B bands x 128/B rows (B in 1, 2, 4, 8, 16; default: the store's own) and, per band, the
stored ids sorted by key (hmse_l4_index_build).  Definitions (tests/similarity_ref.py is the numpy reference):
  * stored id = the chunk's slot; for a merged Store the global slot in (shard, slot) order (read.read_store's numbering);
  * c is a CANDIDATE of query i iff some band of Q_i equals the same band of S_c word by word (a band key only routes the search);
    in a self-join (near_duplicates) c != i;
  * score(i, c) = number of equal hashes of 128 (the Jaccard estimate is score / 128);
  * the result of query i: its candidates with score >= min_score, by score descending, then id ascending, the first top_k
    (1..64); n_candidates counts the candidates before min_score and top_k.
Queries from bytes are chunked as ingest_shard chunks a fresh input and signed by hmse_l4_minhash; the work runs in the HIP
kernels of hmse_amd/csrc/l4_query.hip (hmse_l4_query).  Stored keys are always recomputed on the device from the signatures.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .config import LAYER_L2, IngestConfig
from .manifest import Store, merged_shards


@dataclass
class Hits:
    ids: torch.Tensor            # int64 [q, top_k] stored ids, -1 padding
    scores: torch.Tensor         # int32 [q, top_k] equal hashes of 128, 0 padding
    n_hits: torch.Tensor         # int32 [q] ids returned
    n_candidates: torch.Tensor   # int64 [q] candidates before min_score and top_k
    cuts: torch.Tensor | None = None   # query(): int64 [q + 1] the query chunks' ends in the query bytes


@dataclass
class Locations:
    ptr: torch.Tensor            # int64 [len(ids) + 1]: id k's chunks are offsets[ptr[k]:ptr[k + 1]]
    offsets: torch.Tensor        # int64 corpus offsets of every chunk that holds the id, ascending per id
    lengths: torch.Tensor        # int64 [len(ids)] the id's chunk length


class SimilarityIndex:
    def __init__(self, sig: torch.Tensor, cfg: IngestConfig, bands: int | None = None, chunk_slot: torch.Tensor | None = None,
                 cuts: torch.Tensor | None = None):
        """sig: int32 [n, 128] signatures of the stored chunks in stored-id order, in HBM.  cfg: the store's ingest configuration
        (query chunking, MinHash).  bands: the search banding (default cfg.bands).  chunk_slot (int64 [n_chunks], the stored id of
        every chunk of the corpus in order) and cuts (int64 [n_chunks + 1]) serve locate()."""
        ops._require_gpu(sig, "sig")
        if sig.dim() != 2 or sig.shape[1] != 128 or sig.dtype != torch.int32:
            raise ValueError(f"similarity: signatures must be int32 [n, 128], got {sig.dtype} {tuple(sig.shape)}")
        self.cfg = cfg
        self.bands = int(cfg.bands if bands is None else bands)
        self.search_cfg = ops.search_cfg(cfg, self.bands)
        self.dev = sig.device
        self.sig = sig
        self.keys = ops.l4_lsh(sig, self.search_cfg)[0]
        self.sorted_keys, self.sorted_ids = ops.l4_index_build(self.keys)
        self._loc = None
        if chunk_slot is not None:
            ops._require_gpu(chunk_slot, "chunk_slot")
            ops._require_gpu(cuts, "cuts")
            n = sig.shape[0]
            if chunk_slot.numel() and (int(chunk_slot.min()) < 0 or int(chunk_slot.max()) >= n):
                raise ValueError("similarity: a chunk names a stored id outside the signatures")
            order = torch.argsort(chunk_slot, stable=True)                 # chunks grouped by id, corpus order inside
            count = torch.bincount(chunk_slot, minlength=n)
            start = torch.cumsum(count, 0) - count
            length = torch.zeros(n, dtype=torch.int64, device=self.dev)
            length[chunk_slot] = cuts[1:] - cuts[:-1]
            self._loc = (cuts[:-1][order], start, count, length)

    @property
    def n(self) -> int:
        return int(self.sig.shape[0])

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_result(res, cfg: IngestConfig, bands: int | None = None) -> "SimilarityIndex":
        """The index of one shard's ingest: a ShardResult of ingest_shard or StreamIngest.finish()."""
        if res.sig is None:
            raise ValueError("similarity: the result carries no L4 signatures")
        ops._require_gpu(res.cuts, "res.cuts")
        n_chunks = res.cuts.numel() - 1
        if res.chunk_base != 0 or res.n_global != n_chunks:
            raise ValueError("similarity: one shard of a sharded ingest; build the index from the merged store (from_store)")
        dev = res.cuts.device
        slot_of = torch.full((n_chunks,), -1, dtype=torch.int64, device=dev)
        slot_of[res.uniq_ids] = torch.arange(res.uniq_ids.numel(), dtype=torch.int64, device=dev)
        chunk_slot = slot_of[res.first_occ] if res.first_occ is not None else slot_of
        return SimilarityIndex(res.sig.contiguous(), cfg, bands, chunk_slot, res.cuts)

    @staticmethod
    def from_store(store, cfg: IngestConfig, device, band_tables=None, bands: int | None = None) -> "SimilarityIndex":
        """The index of a Manifest or a merged Store.  band_tables: one sidecar (bytes) for a Manifest, a list with one per shard
        for a Store; the signatures come from its HMSESIGS section.  Without it the store is decoded on the GPU and every stored
        chunk signed by hmse_l4_minhash."""
        from . import bandtable, read
        shards = merged_shards(store, "similarity")
        if isinstance(band_tables, (bytes, bytearray, memoryview)) and len(shards) == 1:
            band_tables = [band_tables]
        if band_tables is not None and len(band_tables) != len(shards):
            raise ValueError(f"similarity: one band-table sidecar per shard ({len(shards)}), got {len(band_tables)}")
        sides = band_tables
        slot, lens = read.chunk_slots(shards)
        u = sum(len(m.index) for m in shards)
        if len(slot) and (slot.max() >= u or (np.bincount(slot, minlength=u) == 0).any()):
            raise ValueError("similarity: the chunk map and the index disagree on the stored chunks")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        cuts = t(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
        chunk_slot = t(slot.astype(np.int64))
        keys_side = None
        if sides is not None:
            sigs, keys = [], []
            for i, (m, bt) in enumerate(zip(shards, sides)):
                try:
                    k, sg = bandtable.read_signatures(bytes(bt))
                except (AssertionError, ValueError, struct.error) as e:            # a truncated or foreign file
                    raise ValueError(f"similarity: band-table sidecar {i} is unreadable ({type(e).__name__}: {e})") from None
                if sg is None:
                    raise ValueError(f"similarity: band-table sidecar {i} has no HMSESIGS section")
                if sg.shape[0] != len(m.index) or k.shape[0] != len(m.index):
                    raise ValueError(f"similarity: band-table sidecar {i} holds {sg.shape[0]} signatures, shard {i} stores {len(m.index)} chunks")
                if sg.shape[1] != 128:
                    raise ValueError(f"similarity: band-table sidecar {i} holds {sg.shape[1]}-hash signatures, not 128")
                if k.shape[1] != cfg.bands:
                    raise ValueError(f"similarity: band-table sidecar {i} is banded {k.shape[1]} x, the configuration {cfg.bands} x")
                sigs.append(sg); keys.append(k)
            sig = t(np.concatenate(sigs).view(np.int32)) if u else torch.zeros((0, 128), dtype=torch.int32, device=device)
            keys_side = np.concatenate(keys) if u else None
        else:
            data = read.read_store(Store(shards), device)
            _, first = np.unique(slot, return_index=True)                  # one chunk holding each stored id
            sig = ops.l4_minhash(data, cuts, cfg, t(first.astype(np.int64))) if u else torch.zeros((0, 128), dtype=torch.int32, device=device)
        ix = SimilarityIndex(sig, cfg, bands, chunk_slot, cuts)
        if keys_side is not None and ix.bands == cfg.bands and not np.array_equal(ix.keys.cpu().numpy().view(np.uint32), keys_side):
            raise ValueError("similarity: the sidecar's band keys are not those of its signatures under this configuration")
        return ix

    # ------------------------------------------------------------------ search
    def query_signatures(self, data: torch.Tensor, seg_off: torch.Tensor | None = None):
        """-> (cuts int64 [q + 1], signatures int32 [q, 128]) of query bytes, chunked as ingest_shard chunks a fresh input."""
        from .ingest import fixed_cuts
        ops._require_gpu(data, "data")
        if data.dtype != torch.uint8:
            raise ValueError("similarity: query data must be a uint8 tensor")
        n = data.numel()
        if n == 0:
            cuts = torch.zeros(1, dtype=torch.int64, device=data.device)
        elif self.cfg.layers & LAYER_L2:
            cuts = ops.l2_cdc(data, self.cfg, seg_off)
        else:
            cuts = fixed_cuts(n, self.cfg, seg_off if seg_off is not None else ops.segment_offsets(n, self.cfg.seg_size, data.device))
        return cuts, ops.l4_minhash(data, cuts, self.cfg)

    def search(self, sig_q: torch.Tensor, top_k: int = 8, min_score: int = 0, exclude_self: bool = False, keys_q=None) -> Hits:
        """Query signatures (int32 [q, 128]) against the index; keys_q (int32 [q, bands]) routes the search (default: hmse_l4_lsh of
        sig_q under the search banding)."""
        _check_limits(top_k, min_score)
        ops._require_gpu(sig_q, "sig_q")
        if keys_q is None:
            keys_q = ops.l4_lsh(sig_q, self.search_cfg)[0]
        ids, scores, n_hits, n_cand = ops.l4_query(sig_q, keys_q, self.sig, self.sorted_keys, self.sorted_ids, self.search_cfg,
                                                   top_k, min_score, exclude_self)
        return Hits(ids, scores, n_hits, n_cand)

    def query(self, data: torch.Tensor, top_k: int = 8, min_score: int = 0, seg_off: torch.Tensor | None = None) -> Hits:
        """Near-duplicates of every chunk of `data` (uint8, in HBM) among the stored chunks."""
        _check_limits(top_k, min_score)
        cuts, sig_q = self.query_signatures(data, seg_off)
        hits = self.search(sig_q, top_k, min_score)
        hits.cuts = cuts
        return hits

    def near_duplicates(self, top_k: int = 8, min_score: int = 0) -> Hits:
        """Self-join: every stored chunk against all the others (c != i)."""
        return self.search(self.sig, top_k, min_score, exclude_self=True, keys_q=self.keys)

    def locate(self, ids) -> Locations:
        """Per stored id the corpus offsets of EVERY chunk that holds it (a POINTER's chunk included) and its length."""
        if self._loc is None:
            raise ValueError("similarity: this index was built without a chunk map")
        occ, start, count, length = self._loc
        ids = torch.as_tensor(ids, dtype=torch.int64).to(self.dev).flatten()
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.n):
            raise ValueError(f"similarity: stored ids lie in [0, {self.n})")
        cnt = count[ids]
        ptr = torch.zeros(ids.numel() + 1, dtype=torch.int64, device=self.dev)
        torch.cumsum(cnt, 0, out=ptr[1:])
        total = int(ptr[-1])
        pos = torch.repeat_interleave(start[ids] - ptr[:-1], cnt, output_size=total) + torch.arange(total, dtype=torch.int64, device=self.dev)
        return Locations(ptr, occ[pos], length[ids])


def _check_limits(top_k: int, min_score: int) -> None:
    if not 1 <= int(top_k) <= 64:
        raise ValueError(f"similarity: top_k lies in [1, 64], got {top_k}")
    if not 0 <= int(min_score) <= 128:
        raise ValueError(f"similarity: min_score lies in [0, 128], got {min_score}")
