"""A written store leaves the project: multi-member gzip (RFC 1952) or BGZF, one member per chunk of the corpus in corpus order.

The records are complete raw DEFLATE streams already, so most of an export is a copy: a FULL record's member is a header, the stream as
stored, and a trailer of CRC-32 and raw length.  A DELTA record needs its dictionary, which gzip cannot express: it is encoded again
without one (ops.l1_deflate, base=None) — the known cost of the format.  The CRC-32 is computed on the GPU over the decoded unique
records, every unique byte once (hmse_crc32), the whole corpus's from the chunks' CRCs and lengths alone (hmse_crc32_combine), and the
members are laid out by one launch from the store's blob and the re-encoded streams (hmse_gzip_members).  `zcat`, `gzip -t`, Python's
gzip and — with bgzf=True — any BGZF reader take the result; nothing here has a CPU path.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .config import KIND_DELTA, KIND_FULL, IngestConfig
from .read import StoreReader

GZIP_HEADER, BGZF_HEADER, TRAILER = 10, 18, 8
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@dataclass
class GzipExport:
    data: torch.Tensor          # uint8 in HBM: the members back to back (BGZF: the EOF block behind them)
    member_off: torch.Tensor    # int64[n_chunks + 1]: member k = data[member_off[k], member_off[k + 1])
    cuts: torch.Tensor          # int64[n_chunks + 1]: the bytes of the corpus member k decodes to
    crc32: int                  # of the whole corpus
    n_copied: int               # records whose stream was copied as stored
    n_reencoded: int            # DELTA records encoded again without their dictionary

    def tobytes(self) -> bytes:
        return self.data.cpu().numpy().tobytes()

    def write(self, path) -> int:
        b = self.tobytes()
        with open(path, "wb") as f:
            f.write(b)
        return len(b)


def _chunk_crc(rd: StoreReader, verify: bool):
    """Steps 1-3: every record decoded once, its CRC-32 -> (raw, raw_off, crc int32[n_rec])."""
    raw, raw_off = rd.decode(verify=verify)
    return raw, raw_off, ops.crc32(raw, raw_off)


def _corpus_crc(rd: StoreReader, crc: torch.Tensor) -> int:
    if not len(rd.slot):
        return 0
    slot = rd._t(rd.slot, torch.int64)
    return ops.crc32_combine(crc[slot].contiguous(), rd._t(rd.cuts[1:] - rd.cuts[:-1], torch.int64))


def crc32(store, device, verify: bool = True) -> int:
    """The CRC-32 of the whole corpus of a store (or one manifest), every unique byte hashed once."""
    rd = StoreReader(store, device)
    return _corpus_crc(rd, _chunk_crc(rd, verify)[2])


def to_gzip(store, device, cfg: IngestConfig | None = None, bgzf: bool = False, verify: bool = True, max_bytes: int = 1 << 34) -> GzipExport:
    """The store (a Store, or one Manifest) as multi-member gzip, or with bgzf=True as BGZF (members of at most 64 KiB with their size in
    the header, the 28-byte EOF block at the end).  `cfg`: the encoder's configuration for the DELTA records (default IngestConfig()).
    ValueError before anything is written if the result would be larger than max_bytes."""
    rd = StoreReader(store, device)
    H = BGZF_HEADER if bgzf else GZIP_HEADER
    tail = len(BGZF_EOF) if bgzf else 0
    n_rec, n_chunks = len(rd.kind), len(rd.slot)
    is_delta = rd.kind == KIND_DELTA
    s_off, s_len = rd.stream_off.copy(), rd.stream_len.copy()

    def total_bytes(lens):
        return int((lens[rd.slot] + H + TRAILER).sum()) + tail
    least = total_bytes(np.where(is_delta, 0, s_len))          # before any work: the copied streams alone
    if least > max_bytes:
        raise ValueError(f"the export needs at least {least} bytes, max_bytes is {max_bytes}")
    t = rd._t
    raw, raw_off, crc = _chunk_crc(rd, verify)
    src1 = None
    delta_ids = np.nonzero(is_delta)[0]
    if delta_ids.size:
        src1, out_off, kind = ops.l1_deflate(raw, raw_off, cfg if cfg is not None else IngestConfig(), chunk_ids=t(delta_ids, torch.int64), base=None)
        if bool((kind != KIND_FULL).any()):
            raise ops.HmseError(-2, "export: a record encoded without a dictionary did not come back FULL")
        oo = out_off.cpu().numpy()
        s_off[delta_ids], s_len[delta_ids] = oo[:-1], oo[1:] - oo[:-1]
    member_off = np.concatenate([[0], np.cumsum(s_len[rd.slot] + H + TRAILER)]).astype(np.int64)
    total = int(member_off[-1]) + tail
    if total > max_bytes:
        raise ValueError(f"the export needs {total} bytes, max_bytes is {max_bytes}")
    data = ops._buf(total, torch.uint8, device)
    member_off_d = t(member_off, torch.int64)
    if n_chunks:
        ops.gzip_members(rd.blob, src1, t(s_off, torch.int64), t(s_len, torch.int64), t(is_delta, torch.uint8), crc, raw_off, t(rd.slot, torch.int64),
                         member_off_d, bgzf=bgzf, out=data[:total - tail] if tail else data)
    if tail:
        data[total - tail:] = t(np.frombuffer(BGZF_EOF, np.uint8), torch.uint8)
    return GzipExport(data=data, member_off=member_off_d, cuts=t(rd.cuts, torch.int64), crc32=_corpus_crc(rd, crc), n_copied=int(n_rec - delta_ids.size),
                      n_reencoded=int(delta_ids.size))


def read_member(exported: GzipExport, k: int):
    """(offset, size) of member k in exported.data — it decodes (zlib, wbits=31) to corpus[cuts[k], cuts[k + 1])."""
    n = exported.member_off.numel() - 1
    if not 0 <= k < n:
        raise IndexError(f"member {k} of {n}")
    a, b = (int(v) for v in exported.member_off[k: k + 2].tolist())
    return a, b - a
