"""Multi-member gzip (RFC 1952) and BGZF come into the project: WARC/WET crawls, BGZF files, concatenated log rotations, export.to_gzip's
own output.  The result is the decoded bytes in HBM with the members' cuts — what ingest.ingest_shard takes.

A gzip member does not say how long it is, so a sequential reader is serial over the whole file.  Here the front of the pipe is parallel
over members (hmse_amd/csrc/gunzip.hip): every position that carries the magic is a CANDIDATE (hmse_gzip_candidates); one wavefront per
candidate parses the header and finds the member's end — from the BC subfield of a BGZF block, else by walking the DEFLATE stream for
its length only (hmse_gzip_measure).  The members are exactly the candidates reachable from offset 0 by following the ends (pointer
doubling with torch ops, on the device): a candidate inside compressed data, or a whole member nested in a stored block, is measured like
any other but never joins the chain, because only real ends lead to the next member; every true start carries the magic and so is a
candidate.  The members are then decoded by the unchanged ops.l1_inflate (one stream per wavefront or per lane, picked by their number)
and their CRC-32s compared with ops.crc32's.  Cost: a generic member is walked twice (length, then decode), a BGZF block once; a member
is serial inside one wavefront or lane.  Nothing here has a CPU path; only counts, totals and the culprit of an error are read back.

The definition is stock zlib: a chain of zlib.decompressobj(wbits=31) over what the one before left unused — the same members, the same
bytes, accepted if and only if that chain accepts (reserved flags, header CRC, data CRC, ISIZE).  One difference: a BGZF block's BC
subfield is believed, so a block whose BSIZE disagrees with its stream is refused (when it is decoded); zlib does not look at BSIZE.
Unlike gzip(1), which warns about trailing garbage and ignores it, bytes behind the last member are refused.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .config import KIND_FULL


class GunzipError(ValueError):
    """What zlib would refuse, with the member's index in the chain and its byte offset in the data."""

    def __init__(self, member: int, offset: int, why: str):
        super().__init__(f"gzip member {member} at offset {offset}: {why}")
        self.member, self.offset = member, offset


@dataclass
class GzipImport:
    raw: torch.Tensor           # uint8 in HBM: the members' bytes back to back
    cuts: torch.Tensor          # int64[n_members + 1]: member k decodes to raw[cuts[k], cuts[k + 1])
    member_off: torch.Tensor    # int64[n_members + 1]: member k = data[member_off[k], member_off[k + 1])
    crc32: int                  # of everything (from the trailers' CRCs; with verify=True they were checked)
    n_members: int
    n_candidates: int           # positions that carry the magic; those beyond n_members lie inside members
    n_bgzf: int                 # members whose end came from a BC subfield: nothing was walked for them


def _load(src, device) -> torch.Tensor:
    if isinstance(src, torch.Tensor):
        if src.dtype != torch.uint8 or src.dim() != 1:
            raise TypeError("from_gzip: a tensor must be uint8 and one-dimensional")
        return src.contiguous() if src.is_cuda else src.contiguous().to(device)
    if isinstance(src, (str, os.PathLike)):
        src = np.fromfile(src, dtype=np.uint8)
    elif isinstance(src, (bytes, bytearray, memoryview)):
        src = np.frombuffer(src, np.uint8)
    a = np.ascontiguousarray(src)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise TypeError("from_gzip: an array must be uint8 and one-dimensional")
    return torch.from_numpy(a.copy()).to(device)


def _on_chain(nxt: torch.Tensor) -> torch.Tensor:
    """nxt int64[m]: every node's successor, the last two nodes their own (END, DEAD).  -> bool[m]: reachable from node 0.  Pointer
    doubling: after round r the marks cover every distance below 2^r and `jump` is the 2^r-th successor."""
    m = nxt.numel()
    mark = torch.zeros(m, dtype=torch.int32, device=nxt.device)
    mark[0] = 1
    jump = nxt
    for _ in range(m.bit_length()):
        mark = (mark + torch.zeros_like(mark).index_add_(0, jump, mark)).clamp_(max=1)
        jump = jump[jump]
    return mark != 0


def from_gzip(src, device, verify: bool = True, max_bytes: int = 1 << 34, max_candidates: int | None = None) -> GzipImport:
    """Decode multi-member gzip / BGZF on the GPU.  `src`: bytes, a uint8 numpy array, a path, or a uint8 tensor (a device tensor is
    used where it is).  verify: compare every member's CRC-32 with its trailer.  ValueError before anything is decoded if the members
    decode to more than max_bytes, and before anything is measured if more than max_candidates positions carry the magic — default
    len(data) // 20 + 1, the most members data of that length can hold (the smallest member has 20 bytes).  GunzipError (a ValueError)
    names member and offset of what zlib would refuse: data that does not start with a member, an invalid member on the chain, bytes
    behind the last member, a member that does not decode, a CRC mismatch."""
    data = _load(src, device)
    dev, n = data.device, data.numel()
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    if n == 0:
        return GzipImport(ops._buf(0, torch.uint8, dev), i64([0]), i64([0]), 0, 0, 0, 0)
    if max_candidates is None:
        max_candidates = n // ops.GZIP_MIN_MEMBER + 1
    # 1. candidates (most files have far fewer than one per KiB: a second pass only when they do not)
    cap = min(max_candidates, n // 1024 + 1024)
    cand, n_cand = ops.gzip_candidates(data, cap)
    if n_cand > max_candidates:
        raise ValueError(f"{n_cand} positions carry the gzip magic, max_candidates is {max_candidates}")
    if n_cand > cap:
        cand, n_cand = ops.gzip_candidates(data, n_cand)
    cand = cand[:n_cand]
    if n_cand == 0 or int(cand[0].item()) != 0:
        raise GunzipError(0, 0, "the data does not start with a gzip member")
    # 2. measure
    stream_off, end, raw_len, crc, flags = ops.gzip_measure(data, cand)
    # 3. the chain from offset 0: next[c] = the candidate at end[c]; END = n_cand (an end at len(data)), DEAD = n_cand + 1
    valid = (flags & ops.GZIP_VALID) != 0
    at = torch.searchsorted(cand, end).clamp_(max=n_cand - 1)
    nxt = torch.where(valid & (cand[at] == end), at, torch.where(valid & (end == n), n_cand, n_cand + 1))
    mark = _on_chain(torch.cat([nxt, i64([n_cand, n_cand + 1])]))
    idx = torch.nonzero(mark[:n_cand]).squeeze(1)             # ascending = chain order: an end lies behind its start
    n_mem = idx.numel()
    rl = raw_len[idx]
    fast = (flags[idx] & ops.GZIP_FAST) != 0
    last = idx[-1]
    dead, total, n_bgzf, l_off, l_end, l_flags = torch.stack([mark[n_cand + 1].to(torch.int64), rl.sum(), fast.sum(), cand[last], end[last],
                                                              flags[last].to(torch.int64)]).tolist()
    if dead:                                                  # the chain's last member is its culprit
        if not l_flags & ops.GZIP_VALID:
            raise GunzipError(n_mem - 1, l_off, f"not a valid member ({ops.GZIP_WHY.get(l_flags >> ops.GZIP_WHY_SHIFT, 'unknown')})")
        raise GunzipError(n_mem, l_end, f"{n - l_end} bytes behind member {n_mem - 1} are not a gzip member")
    # 4. the size, before anything is allocated
    if total > max_bytes:
        raise ValueError(f"the members decode to {total} bytes, max_bytes is {max_bytes}")
    # 5. decode: kind FULL, no base; u32 stream lengths travel as int32 bits
    s_off = stream_off[idx]
    s_len = end[idx] - 8 - s_off
    s_len32 = torch.where(s_len >= (1 << 31), s_len - (1 << 32), s_len).to(torch.int32)
    kind = torch.full((n_mem,), KIND_FULL, dtype=torch.uint8, device=dev)
    raw, cuts, ok = ops.l1_inflate(data, s_off, kind, None, rl, stream_len=s_len32, check=False)
    member_off = torch.cat([cand[idx], i64([n])])
    bad = torch.nonzero(ok == 0)
    if bad.numel():
        k = int(bad[0].item())
        raise GunzipError(k, int(member_off[k].item()), "the member does not decode to its recorded end and length"
                          + (" (its BSIZE disagrees with its stream)" if bool(fast[k].item()) else ""))
    # 6. CRC-32
    want = crc[idx].contiguous()
    if verify:
        bad = torch.nonzero(ops.crc32(raw, cuts) != want)
        if bad.numel():
            k = int(bad[0].item())
            raise GunzipError(k, int(member_off[k].item()), "CRC-32 mismatch")
    return GzipImport(raw=raw, cuts=cuts, member_off=member_off, crc32=ops.crc32_combine(want, rl.contiguous()), n_members=n_mem,
                      n_candidates=n_cand, n_bgzf=int(n_bgzf))
