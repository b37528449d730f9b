"""Exact byte-pattern search over a store: where does this byte string occur?

Today's answer — read.read_store(...), .cpu(), bytes.find on the host — decodes the whole corpus, moves it over PCIe and scans every
duplicate chunk once per occurrence.  A corpus of N bytes holds only U <= N unique record bytes, so a StoreFinder decodes every record
ONCE (read.StoreReader.decode), keeps the records and the chunk map in HBM, and answers a query with
  scan    every pattern is looked for once per stored record (hmse_find_scan: each unique byte read once);
  place   every in-record hit belongs to every chunk that maps to the record, POINTERs included (sort, hmse_find_place);
  seams   only the max(m) - 1 bytes in front of each chunk boundary get a second look, through the chunk map (hmse_find_seams).
Definitions (tests/find_ref.py restates them in plain Python):
  * C is the N bytes read.read_store(store) returns (a multi-rank stream's store: in stream order); patterns are P >= 0 byte strings of
    1..256 bytes, equal ones may repeat and each is answered on its own;
  * an occurrence of pattern j is any offset o with C[o : o + m_j] == pat_j; overlapping occurrences all count;
  * ignore_case folds the ASCII letters A-Z to a-z on both sides, every other byte value (>= 0x80 included) compares exactly:
    bytes.lower() on both sides;
  * result: counts int64[P], and in CSR form ptr int64[P + 1], offsets int64[ptr[P]] — ascending per pattern, no offset twice.
Sorting, prefix sums and searchsorted go through torch (plumbing, as SimilarityIndex.locate does); the byte work runs in the HIP kernels
of hmse_amd/csrc/find.hip.  There is no CPU path.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .read import StoreReader

MAX_PATTERN_LEN = ops.FIND_MAX_LEN
GROUP = ops.FIND_MAX_PATTERNS      # patterns per launch; more are answered in groups


@dataclass
class Found:
    ptr: torch.Tensor            # int64 [P + 1]: pattern j's occurrences are offsets[ptr[j]:ptr[j + 1]]
    offsets: torch.Tensor        # int64 corpus offsets, ascending per pattern
    counts: torch.Tensor         # int64 [P] occurrences per pattern


def pack_patterns(patterns):
    """A list of bytes-like patterns (bytes, bytearray, memoryview, uint8 numpy array) -> (uint8 numpy array of all of them back to
    back, list of P + 1 bounds).  ValueError for a str, an empty pattern or one over 256 bytes."""
    if isinstance(patterns, (str, bytes, bytearray, memoryview)) or (isinstance(patterns, np.ndarray) and patterns.ndim == 1 and patterns.dtype == np.uint8):
        raise ValueError("find: patterns is a LIST of byte strings (for one pattern: [pattern])")
    parts, off = [], [0]
    for i, p in enumerate(patterns):
        if isinstance(p, str):
            raise ValueError(f"find: pattern {i} is a str; patterns are bytes (encode it)")
        if isinstance(p, np.ndarray):
            if p.dtype != np.uint8 or p.ndim != 1:
                raise ValueError(f"find: pattern {i} is a {p.dtype} array of {p.ndim} dimensions; a numpy pattern is a 1-D uint8 array")
            b = p.tobytes()
        elif isinstance(p, (bytes, bytearray, memoryview)):
            b = bytes(p)
        else:
            raise ValueError(f"find: pattern {i} is a {type(p).__name__}; patterns are bytes-like")
        if not 1 <= len(b) <= MAX_PATTERN_LEN:
            raise ValueError(f"find: pattern {i} has {len(b)} bytes; a pattern has 1 to {MAX_PATTERN_LEN}")
        parts.append(b)
        off.append(off[-1] + len(b))
    return np.frombuffer(b"".join(parts), np.uint8), off


class StoreFinder:
    def __init__(self, store, device, verify: bool = True):
        """store: a Manifest or a merged Store (read.StoreReader refuses what cannot be read: unmerged parts, unresolved pointers).
        Decodes every record once; verify checks the SHA-256 of the decoded records where the store carries digests."""
        rd = StoreReader(store, device)
        self.dev = torch.device(device)
        self.n_bytes = int(rd.n_bytes)
        self.n_records = int(len(rd.kind))
        if self.n_records:
            self.raw, self.raw_off = rd.decode(verify=verify)
        else:
            self.raw = torch.zeros(0, dtype=torch.uint8, device=device)
            self.raw_off = torch.zeros(1, dtype=torch.int64, device=device)
        self.slot = rd._t(rd.slot.astype(np.int64), torch.int64)
        self.cuts = rd._t(rd.cuts, torch.int64)
        if self.slot.numel() and int(self.slot.max()) >= self.n_records:
            raise ValueError("find: the chunk map names a record outside the index")
        # how many chunks map to each record: an in-record hit occurs that often in the corpus
        self.mult = torch.bincount(self.slot, minlength=self.n_records).to(torch.int32) if self.n_records else torch.zeros(0, dtype=torch.int32, device=device)
        self.resident_bytes = sum(t.numel() * t.element_size() for t in (self.raw, self.raw_off, self.slot, self.cuts, self.mult))

    # ------------------------------------------------------------------ the groups of a query
    def _groups(self, patterns):
        flat, off = pack_patterns(patterns)
        n = len(off) - 1
        pat = torch.from_numpy(flat.copy()).to(self.dev) if n else None
        return pat, [off[g: min(g + GROUP, n) + 1] for g in range(0, n, GROUP)], n

    def _count_group(self, pat, off, ignore_case):
        """-> (occurrences int64[p], in-record hits of the scan, seam hits): two count-only launches."""
        _, n_scan, c_scan = ops.find_scan(self.raw, self.raw_off, self.mult, pat, off, ignore_case, hits_cap=0)
        _, n_seam, c_seam = ops.find_seams(self.raw, self.raw_off, self.cuts, self.slot, pat, off, ignore_case, hits_cap=0)
        return c_scan + c_seam, n_scan, n_seam

    def count(self, patterns, ignore_case: bool = False) -> torch.Tensor:
        """Occurrences per pattern, int64[P] on the device: two count-only launches per 32 patterns, nothing is materialised."""
        pat, groups, n = self._groups(patterns)
        if n == 0 or self.n_records == 0:
            return torch.zeros(n, dtype=torch.int64, device=self.dev)
        return torch.cat([self._count_group(pat, off, ignore_case)[0] for off in groups])

    def find(self, patterns, ignore_case: bool = False, max_hits: int = 1 << 24) -> Found:
        """Every occurrence of every pattern.  Counts first: ValueError naming the counts if their sum exceeds max_hits."""
        pat, groups, n = self._groups(patterns)
        dev = self.dev
        if n == 0 or self.n_records == 0:
            z = torch.zeros(n, dtype=torch.int64, device=dev)
            return Found(torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), z)
        counted = [self._count_group(pat, off, ignore_case) for off in groups]
        counts = torch.cat([c[0] for c in counted])
        total = int(counts.sum())
        if total > int(max_hits):
            raise ValueError(f"find: {total} occurrences exceed max_hits = {max_hits}; counts per pattern: {counts.tolist()}")
        parts = []
        for off, (c, n_scan, n_seam) in zip(groups, counted):
            found = []
            if n_scan:
                hits, _, c_scan = ops.find_scan(self.raw, self.raw_off, self.mult, pat, off, ignore_case, hits_cap=n_scan)
                hits = torch.sort(hits)[0]                                   # by position in raw, then pattern
                rec_lo = torch.searchsorted(hits, self.raw_off << 8)         # first hit of every record
                per_chunk = (rec_lo[1:] - rec_lo[:-1])[self.slot]
                chunk_out = torch.zeros(self.slot.numel() + 1, dtype=torch.int64, device=dev)
                torch.cumsum(per_chunk, 0, out=chunk_out[1:])
                found.append(ops.find_place(hits, self.raw_off, self.cuts, self.slot, chunk_out, int(c_scan.sum())))
            if n_seam:
                found.append(ops.find_seams(self.raw, self.raw_off, self.cuts, self.slot, pat, off, ignore_case, hits_cap=n_seam)[0])
            if found:
                h = torch.cat(found)
                key = torch.sort(((h & 0xFF) << 56) | (h >> 8))[0]          # by (pattern, offset): offsets stay below 2^56
                parts.append(key & ((1 << 56) - 1))
        offsets = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=dev)
        ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=ptr[1:])
        if offsets.numel() != total:
            raise ops.HmseError(-1, f"find: {offsets.numel()} occurrences located, {total} counted")
        return Found(ptr, offsets, counts)


def find(store, patterns, device, ignore_case: bool = False, max_hits: int = 1 << 24, verify: bool = True) -> Found:
    """One-off form of StoreFinder(store, device, verify).find(patterns, ignore_case, max_hits)."""
    return StoreFinder(store, device, verify).find(patterns, ignore_case, max_hits)
