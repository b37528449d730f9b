"""Replication of a store onto an older copy: diff, patch, apply — on the GPU.

Last night's store is on the replica (`have`), tonight's is here (`want`); only the difference should travel.  The contract is byte
identity with the store that already exists: apply_patch(have, make_patch(have, want)).to_bytes() == want.to_bytes().  Nothing is
re-encoded and no dictionary is re-selected.

  diff        a digest join (hmse_l3_dedup over [have's digests | want's digests]): which chunks of want the replica already holds
  make_patch  the join's candidates PROVEN byte-identical by hmse_sync_match — equal digests say the chunks are equal, not the stored
              streams: the same chunk is FULL in one store and DELTA in the other, or DELTA against another dictionary — and the
              streams that are not, gathered densely (hmse_record_gather)
  apply_patch want's blob laid out by ONE hmse_record_gather over pieces: per record its DeltaChunk header, its stream (from have's
              blobs or the patch's literals) and its padding

PyTorch is plumbing; the byte work happens in the kernels.  There is no CPU path.  What is pure numpy — the tiling check and the piece
table — lives in functions a test without a GPU can call (check_tiling, plan_pieces).
"""
from __future__ import annotations

import dataclasses
import hashlib
import struct

import numpy as np
import torch

from . import ops
from .config import KIND_DELTA, KIND_POINTER
from .manifest import Manifest, Store
from .read import ReadError, StoreReader, to_device

PATCH_MAGIC = b"HMSEPTCH"
PATCH_VERSION = 1
_PATCH_HDR = "<I32sQQQQQ"      # version, have_id, len(meta), blob size, records, DELTA records, literal bytes


# ---- diff -----------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class StoreDiff:
    present: np.ndarray        # bool[n_chunks]: per chunk of want in corpus order, its SHA-256 is a record of have
    new_ranges: np.ndarray     # int64[k, 2]: coalesced (offset, len) ranges of want's corpus whose chunks are absent
    shared_bytes: int
    new_bytes: int
    new_unique_bytes: int      # every absent record counted once
    unreferenced: np.ndarray   # int64: records of have, in (shard, slot) numbering, whose digest no chunk of want has


def _shards(store) -> list:
    return list(store.shards) if isinstance(store, Store) else [store]


def _index_digests(store) -> np.ndarray:
    """The records' digests in (shard, slot) order (StoreReader's numbering may differ: a global-L4 stream's store)."""
    sh = _shards(store)
    return np.concatenate([m.index["sha256"] for m in sh]).reshape(-1, 32) if sh else np.zeros((0, 32), np.uint8)


def _need_digests(sha: np.ndarray, who: str) -> None:
    if len(sha) and not sha.any():
        raise ValueError(f"{who} was written without L3: it carries no digests to compare")


def _join(sha_have: np.ndarray, sha_want: np.ndarray, device) -> torch.Tensor:
    """first_occ of hmse_l3_dedup over [have | want]: entry n_have + j < n_have names a record of have with want's digest j."""
    n = len(sha_have) + len(sha_want)
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=device)
    fo, _ = ops.l3_dedup(to_device(np.concatenate([sha_have, sha_want]), torch.uint8, device))
    return fo


def coalesce(offsets: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """Ascending (offset, len) pieces -> int64[k, 2] with touching pieces merged and empty ones dropped."""
    keep = lens > 0
    offsets, lens = offsets[keep].astype(np.int64), lens[keep].astype(np.int64)
    if not len(offsets):
        return np.zeros((0, 2), np.int64)
    start = np.ones(len(offsets), bool)
    start[1:] = offsets[1:] != offsets[:-1] + lens[:-1]
    first = np.nonzero(start)[0]
    end = np.concatenate([first[1:], [len(offsets)]]) - 1
    return np.stack([offsets[first], offsets[end] + lens[end] - offsets[first]], axis=1)


def diff(have, want, device) -> StoreDiff:
    """Which chunks of `want` (a Manifest or a merged Store; per chunk in corpus order, a multi-rank stream's store: stream order) the
    store `have` already holds, by SHA-256.  Both are opened through StoreReader (an unreadable store is refused there)."""
    StoreReader(have, device)          # (only to refuse what a reader refuses: have's digests are taken in (shard, slot) order, not the reader's)
    rw = StoreReader(want, device)
    sha_h, sha_w = _index_digests(have), rw.sha.reshape(-1, 32)
    _need_digests(sha_h, "diff: have"); _need_digests(sha_w, "diff: want")
    n_h, n_w = len(sha_h), len(sha_w)
    fo = _join(sha_h, sha_w, device)
    rec_present = fo[n_h:] < n_h                                                   # per record of want (the reader's numbering)
    first_new = fo[n_h:] == torch.arange(n_h, n_h + n_w, dtype=torch.int64, device=fo.device)   # absent, and the first of its digest
    mark = torch.zeros(n_h, dtype=torch.bool, device=fo.device)
    mark[fo[n_h:][rec_present]] = True
    unref = torch.nonzero(~mark[fo[:n_h]]).flatten()                             # (a duplicate digest inside have follows its first)
    rec_present, first_new = rec_present.cpu().numpy(), first_new.cpu().numpy()
    present = rec_present[rw.slot] if len(rw.slot) else np.zeros(0, bool)
    lens = np.diff(rw.cuts)
    new_bytes = int(lens[~present].sum())
    return StoreDiff(present, coalesce(rw.cuts[:-1][~present], lens[~present]), rw.n_bytes - new_bytes, new_bytes,
                     int(rw.raw_len[first_new].sum()), unref.cpu().numpy().astype(np.int64))


# ---- planning (pure numpy) ------------------------------------------------------------------------------------------------------------
def slot_kinds(m: Manifest) -> np.ndarray:
    """The kind of every record, from the chunk map (every record is some chunk's own)."""
    k = np.zeros(len(m.index), np.uint8)
    own = m.chunk_map["kind"] != KIND_POINTER
    k[m.chunk_map["slot"][own]] = m.chunk_map["kind"][own]
    return k


def check_tiling(lba_unit: int, index: np.ndarray, kind: np.ndarray, blob_size: int, blob: np.ndarray | None = None) -> np.ndarray:
    """The records must TILE the blob in ascending lba order — no gap other than padding shorter than lba_unit, no overlap, every
    padding byte 0 (checked when `blob` is given), a DELTA record at least its 8-byte header — else ValueError: apply could not
    reproduce such a blob.  Returns the records in blob order."""
    off = index["lba"].astype(np.int64) * int(lba_unit)
    ln = index["length"].astype(np.int64)
    order = np.lexsort((ln, off))
    if ((kind == KIND_DELTA) & (ln < 8)).any():
        raise ValueError("a DELTA record is shorter than its DeltaChunk header")
    start = np.concatenate([off[order], [int(blob_size)]])
    end = np.concatenate([[0], off[order] + ln[order]])
    gap = start - end                  # gap[i]: in front of the i-th record in blob order; gap[-1]: behind the last
    if (gap < 0).any():
        raise ValueError("the records do not tile the blob: two records overlap (or one ends past the blob)")
    if (gap >= max(int(lba_unit), 1)).any():
        raise ValueError(f"the records do not tile the blob: a gap of {int(gap.max())} bytes is no padding (lba_unit {lba_unit})")
    if blob is not None:
        if blob.size != int(blob_size):
            raise ValueError("the blob's size is not the declared one")
        g = np.nonzero(gap)[0]
        if len(g):
            pos = np.repeat(end[g] - np.concatenate([[0], np.cumsum(gap[g])[:-1]]), gap[g]) + np.arange(int(gap[g].sum()))
            if blob[pos].any():
                raise ValueError("the blob has non-zero padding between its records")
    return order


def plan_pieces(lba_unit: int, index: np.ndarray, kind: np.ndarray, blob_size: int, src: np.ndarray, have_bytes: int):
    """The piece table of apply_patch, for ONE hmse_record_gather: per record in blob order its DeltaChunk header, its stream and its
    padding.  Source 0 is have's blobs concatenated in shard order; source 1 is [DeltaChunk headers in slot order | literal streams in
    slot order | a run of zeros].  `src[k]` is -1 (a literal) or record k's byte position in source 0.
    -> (src_off int64[p], src_sel uint8[p], dst_off int64[p + 1], second-source layout (header bytes, literal bytes, zero bytes))."""
    u = len(index)
    if len(src) != u or len(kind) != u:
        raise ValueError("the patch's source table does not match its index")
    order = check_tiling(lba_unit, index, kind, blob_size)
    off = index["lba"].astype(np.int64) * int(lba_unit)
    ln = index["length"].astype(np.int64)
    is_delta = kind == KIND_DELTA
    hdr = np.where(is_delta, 8, 0).astype(np.int64)
    s_len = ln - hdr
    lit = src < 0
    if (src[~lit] + s_len[~lit] > int(have_bytes)).any():
        raise ValueError("the patch copies from outside the store it is applied to")
    hdr_bytes, lit_bytes = 8 * int(is_delta.sum()), int(s_len[lit].sum())
    hdr_at = 8 * (np.cumsum(is_delta) - is_delta)                                   # position of slot k's header in source 1
    lit_at = hdr_bytes + np.cumsum(np.where(lit, s_len, 0)) - np.where(lit, s_len, 0)
    pad = np.concatenate([off[order], [int(blob_size)]])[1:] - (off[order] + ln[order])      # behind every record, in blob order
    zero_bytes = int(pad.max()) if u else 0
    # three pieces per record, in blob order; the empty ones are dropped
    p_len = np.stack([hdr[order], s_len[order], pad], axis=1).reshape(-1)
    p_src = np.stack([hdr_at[order], np.where(lit, lit_at, src)[order], np.full(u, hdr_bytes + lit_bytes, np.int64)], axis=1).reshape(-1)
    p_sel = np.stack([np.ones(u, np.uint8), lit[order].astype(np.uint8), np.ones(u, np.uint8)], axis=1).reshape(-1)
    keep = p_len > 0
    dst_off = np.concatenate([[0], np.cumsum(p_len[keep])]).astype(np.int64)
    assert int(dst_off[-1]) == int(blob_size)
    return p_src[keep].astype(np.int64), p_sel[keep], dst_off, (hdr_bytes, lit_bytes, zero_bytes)


# ---- the patch ------------------------------------------------------------------------------------------------------------------------
def have_id(have) -> bytes:
    """What a patch is bound to: SHA-256 over every shard's (lba_unit, len(index), blob.size) and index bytes (40 B per record)."""
    h = hashlib.sha256()
    for m in _shards(have):
        h.update(struct.pack("<IQQ", int(m.lba_unit), len(m.index), int(m.blob.size)))
        h.update(np.ascontiguousarray(m.index).tobytes())
    return h.digest()


@dataclasses.dataclass
class Patch:
    meta: bytes              # want's manifest serialised with an EMPTY blob: header, index, chunk map, pointers (and tables behind)
    blob_size: int
    delta_hdrs: np.ndarray   # uint8[n_delta, 8]: the DeltaChunk headers in slot order
    src: np.ndarray          # int64[records]: -1 = a literal, else the stream's byte position in have's blobs concatenated in shard order
    literals: np.ndarray     # uint8: the literal streams back to back, in slot order
    have_id: bytes
    copied_bytes: int = 0    # stream bytes apply takes from have

    @property
    def literal_bytes(self) -> int:
        return int(self.literals.size)

    @property
    def nbytes(self) -> int:
        return 8 + struct.calcsize(_PATCH_HDR) + len(self.meta) + self.delta_hdrs.size + 8 * len(self.src) + self.literals.size

    def to_bytes(self) -> bytes:
        hdr = struct.pack(_PATCH_HDR, PATCH_VERSION, self.have_id, len(self.meta), self.blob_size, len(self.src), len(self.delta_hdrs),
                          self.literals.size)
        return (PATCH_MAGIC + hdr + self.meta + np.ascontiguousarray(self.delta_hdrs, np.uint8).tobytes()
                + np.ascontiguousarray(self.src, "<i8").tobytes() + np.ascontiguousarray(self.literals, np.uint8).tobytes())

    @staticmethod
    def from_bytes(b: bytes) -> "Patch":
        o = 8 + struct.calcsize(_PATCH_HDR)
        if len(b) < o or b[:8] != PATCH_MAGIC:
            raise ValueError("not a patch (magic HMSEPTCH)")
        ver, hid, n_meta, blob_size, n_rec, n_delta, n_lit = struct.unpack_from(_PATCH_HDR, b, 8)
        if ver != PATCH_VERSION:
            raise ValueError(f"patch version {ver}: this reader knows version {PATCH_VERSION}")
        if len(b) != o + n_meta + 8 * n_delta + 8 * n_rec + n_lit:
            raise ValueError("the patch is truncated or has bytes behind its end")
        meta = bytes(b[o:o + n_meta]); o += n_meta
        hdrs = np.frombuffer(b, np.uint8, 8 * n_delta, o).reshape(n_delta, 8); o += 8 * n_delta
        src = np.frombuffer(b, "<i8", n_rec, o).astype(np.int64); o += 8 * n_rec
        lit = np.frombuffer(b, np.uint8, n_lit, o)
        m = Manifest.from_bytes(meta)
        kind = slot_kinds(m)
        s_len = m.index["length"].astype(np.int64) - np.where(kind == KIND_DELTA, 8, 0)
        if len(m.index) != n_rec or int((kind == KIND_DELTA).sum()) != n_delta or int(s_len[src < 0].sum()) != n_lit:
            raise ValueError("the patch's tables do not match its manifest")
        return Patch(meta, int(blob_size), hdrs, src, lit, hid, int(s_len[src >= 0].sum()))


def _one_shard(want) -> Manifest:
    if isinstance(want, Store):
        if len(want.shards) != 1:
            raise ValueError(f"make_patch: want is a store of {len(want.shards)} shards; a patch describes ONE shard (multi-shard want is not supported)")
        m = want.shards[0]
    elif isinstance(want, Manifest):
        m = want
    else:
        raise ValueError(f"make_patch: want must be a Manifest or a Store, not {type(want).__name__}")
    if m.n_remote():
        raise ValueError("make_patch: records of want use dictionaries stored in other shards (remote_bases): not supported")
    return m


def make_patch(have, want, device) -> Patch:
    """What turns `have` (any readable store) into `want` (a one-shard Manifest, or a Store of one shard, without remote dictionaries):
    per record of want either a byte position in have's blobs — the digest join's candidate, proven byte-identical by
    hmse_sync_match — or a literal stream."""
    m = _one_shard(want)
    kind = slot_kinds(m)
    check_tiling(m.lba_unit, m.index, kind, m.blob.size, m.blob)
    sha_w = m.index["sha256"].reshape(-1, 32)
    _need_digests(sha_w, "make_patch: want")
    rw, rh = StoreReader(m, device), StoreReader(have, device)        # (refuses an unreadable store; the blobs in HBM)
    _need_digests(rh.sha, "make_patch: have")
    u, n_h = len(m.index), len(rh.sha)
    is_delta = kind == KIND_DELTA
    rec_off = m.index["lba"].astype(np.int64) * m.lba_unit
    s_off = rec_off + np.where(is_delta, 8, 0)
    s_len = m.index["length"].astype(np.int64) - np.where(is_delta, 8, 0)
    hdrs = m.blob[rec_off[is_delta][:, None] + np.arange(8)[None, :]].reshape(-1, 8).copy()
    t = lambda a, dt: to_device(a, dt, device)
    # 1. the digest join: the reader's numbering of have's records (its digests, offsets and lengths are renumbered together)
    fo = _join(rh.sha.reshape(-1, 32), sha_w, device)[n_h:]
    cand = torch.where(fo < n_h, fo, torch.full_like(fo, -1))
    # 2. the byte proof
    a_blob = rw.blob[:m.blob.size]
    b_blob = rh.blob if n_h else rh.blob[:0]
    same, status = ops.sync_match(a_blob, t(s_off, torch.int64), t(s_len, torch.int32), b_blob, t(rh.stream_off, torch.int64),
                                  t(rh.stream_len, torch.int32), cand)
    if status:
        raise ReadError("make_patch: a record's stream reaches outside its blob")
    same = same != 0
    # 3. the literals, densely
    lit = torch.nonzero(~same).flatten()
    s_len_d = t(s_len, torch.int64)
    dst_off = torch.zeros(lit.numel() + 1, dtype=torch.int64, device=device)
    torch.cumsum(s_len_d[lit], 0, out=dst_off[1:])
    literals = ops.record_gather(a_blob, None, t(s_off, torch.int64)[lit].contiguous(), torch.zeros(lit.numel(), dtype=torch.uint8, device=device), dst_off)
    src = torch.where(same, t(rh.stream_off, torch.int64)[cand.clamp(min=0)] if n_h else cand, torch.full_like(cand, -1))
    copied = int(s_len_d[same].sum().item())
    meta = dataclasses.replace(m, blob=np.zeros(0, np.uint8)).to_bytes()
    return Patch(meta, int(m.blob.size), hdrs, src.cpu().numpy().astype(np.int64), literals.cpu().numpy(), have_id(have), copied)


def apply_patch(have, patch: Patch, device, verify: bool = True) -> Manifest:
    """`have` + `patch` -> the wanted store's one shard as a Manifest, byte for byte.  ValueError: the patch was made against another
    store (have_id), or its tables are inconsistent.  With `verify` the result is opened with StoreReader and every record is decoded
    and SHA-256-checked: a damaged copy surfaces as ReadError, never as a silently wrong store."""
    if have_id(have) != patch.have_id:
        raise ValueError("apply_patch: the patch was made against another store (have_id differs)")
    m = Manifest.from_bytes(patch.meta)
    kind = slot_kinds(m)
    rh = StoreReader(have, device)
    have_bytes = sum(int(s.blob.size) for s in _shards(have))
    src_off, src_sel, dst_off, (hdr_bytes, lit_bytes, zero_bytes) = plan_pieces(m.lba_unit, m.index, kind, patch.blob_size, patch.src, have_bytes)
    if hdr_bytes != patch.delta_hdrs.size or lit_bytes != patch.literals.size:
        raise ValueError("apply_patch: the patch's headers or literals do not match its index")
    second = np.concatenate([np.ascontiguousarray(patch.delta_hdrs, np.uint8).reshape(-1), np.ascontiguousarray(patch.literals, np.uint8),
                             np.zeros(zero_bytes, np.uint8)])
    t = lambda a, dt: to_device(a, dt, device)
    blob = ops.record_gather(rh.blob if have_bytes else rh.blob[:0], t(second, torch.uint8), t(src_off, torch.int64), t(src_sel, torch.uint8),
                             t(dst_off, torch.int64))
    out = dataclasses.replace(m, blob=blob.cpu().numpy())
    if verify:
        try:
            StoreReader(out, device).decode(verify=True)
        except ops.HmseError as e:
            raise ReadError(f"apply_patch: the result does not decode: {e}") from e
    return out
