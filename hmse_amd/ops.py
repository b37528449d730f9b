"""Stage operators L2/L3/L4/L1 over the C-ABI (include/hmse.h): tensors in, tensors out.

PyTorch is plumbing here (device memory, current HIP stream); every byte of work happens in the
hand-written gfx950 kernels of hmse_amd/csrc.  u64 arrays travel as torch.int64, u32 as torch.int32
(same bits).  All ops run on the tensor's device and torch's current stream and raise HmseError
on a non-zero status — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .config import IngestConfig

STAGE_L2, STAGE_SHA, STAGE_DEDUP, STAGE_MINHASH, STAGE_LSH, STAGE_DEFLATE = 2, 3, 4, 5, 6, 7
STAGE_INFLATE, STAGE_ASSEMBLE, STAGE_MANIFEST = 16, 17, 18
STAGE_GC_PLAN, STAGE_RECORD_GATHER = 24, 25
STAGE_L4_INDEX, STAGE_L4_QUERY = 26, 27
STAGE_SCRUB_RECORDS, STAGE_SCRUB_ATTRIBUTE = 28, 29
STAGE_FIND_SCAN, STAGE_FIND_PLACE = 30, 31
STAGE_SYNC_MATCH = 19
STAGE_EXPORT_CRC, STAGE_EXPORT_MEMBERS = 0, 1
GZIP_BGZF = 1
QUERY_EXCLUDE_SELF = 1
FIND_MAX_PATTERNS, FIND_MAX_LEN, FIND_IGNORE_CASE = 32, 256, 1
LINES_START_CUT, LINES_END_CUT, LINES_BAD, LINES_MAX_REACH = 1, 2, 128, 1 << 24
FINDSET_MAX_PATTERNS, FINDSET_MIN_LEN, FINDSET_ID_BITS, FINDSET_BITMAP_BITS, FINDSET_HASH = 1 << 20, 4, 24, 19, 0x9E3779B1


class HmseError(RuntimeError):
    def __init__(self, code: int, where: str):
        msg = _lib.hip_lib().hmse_strerror(code).decode()
        super().__init__(f"{where}: {msg} ({code})")
        self.code = code


def _check(rc: int, where: str) -> None:
    if rc != 0:
        raise HmseError(rc, where)


def _require_gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise HmseError(-1, f"{name} must live in HBM (got a {t.device} tensor; hmse_amd has no CPU path)")
    if not t.is_contiguous():
        raise HmseError(-1, f"{name} must be contiguous")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _buf(shape, dtype, device, fill: int | None = None) -> torch.Tensor:
    """Every device buffer this module hands to the library besides a workspace (_ws): outputs, status words, placeholders.
    `fill` (0 or -1) is the wrapper's own caution, not part of the C contract: include/hmse.h tells a caller to clear nothing, the
    library writes every element it declares valid.  tests/arena.py replaces _ws and _buf to decide what memory a call sees."""
    if fill is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if fill == 0:
        return torch.zeros(shape, dtype=dtype, device=device)
    return torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device=device)


def workspace_bytes(stage: int, n: int, cfg: IngestConfig) -> int:
    c = cfg.to_c()
    return int(_lib.hip_lib().hmse_workspace_bytes(stage, n, C.byref(c)))


def segment_offsets(n: int, seg_size: int, device) -> torch.Tensor:
    k = max(1, -(-n // seg_size))
    off = torch.arange(k + 1, dtype=torch.int64, device=device) * seg_size
    return torch.clamp(off, max=n)


def l2_cdc(data: torch.Tensor, cfg: IngestConfig, seg_off: torch.Tensor | None = None) -> torch.Tensor:
    """FastCDC cut points. Returns int64 cuts[n_chunks+1] (cuts[0] == 0). README.md:2456-2490."""
    _require_gpu(data, "data")
    n = data.numel()
    dev = data.device
    if seg_off is None:
        seg_off = segment_offsets(n, cfg.seg_size, dev)
    _require_gpu(seg_off, "seg_off")
    n_seg = seg_off.numel() - 1
    c = cfg.to_c()
    lib = _lib.hip_lib()
    cap = n // cfg.min_size + n_seg + 2
    cuts = _buf(cap, torch.int64, dev)
    meta = _buf(2, torch.int64, dev, fill=0)  # [n_cuts, status]
    # exact workspace for this segmentation: the generic sizing assumes ceil(n/seg_size) segments
    ws_bytes = workspace_bytes(STAGE_L2, n, cfg) + 24 * max(0, n_seg - n // cfg.seg_size) + 4096
    # The provisioned candidate list holds 8x the expected density.  Bytes that are denser still (status bit 0) are legitimate
    # input: run once more with a list of one entry per byte, which nothing can overflow (include/hmse.h).
    for extra in (0, 4 * n + 256):
        ws = _ws(ws_bytes + extra, dev)
        rc = lib.hmse_l2_cdc(_ptr(data), n, _ptr(seg_off), n_seg, C.byref(c), _ptr(cuts), cap, meta.data_ptr(),
                             meta.data_ptr() + 8, ws.data_ptr(), ws.numel(), _stream())
        _check(rc, "hmse_l2_cdc")
        n_cuts, status = (int(v) for v in meta.tolist())
        if not (status & 1):
            break
        del ws
    if status & 0xFFFFFFFF:
        raise HmseError(-2, f"hmse_l2_cdc device status {status & 0xFFFFFFFF:#x}")
    return cuts[: n_cuts + 1]


def l3_sha256(data: torch.Tensor, cuts: torch.Tensor) -> torch.Tensor:
    """SHA-256 of every chunk -> uint8 [n_chunks, 32]. README.md:2543."""
    _require_gpu(data, "data")
    _require_gpu(cuts, "cuts")
    n_chunks = cuts.numel() - 1
    out = _buf((max(n_chunks, 0), 32), torch.uint8, data.device)
    if n_chunks <= 0:
        return out
    ws = _ws(workspace_bytes(STAGE_SHA, n_chunks, IngestConfig()), data.device)
    rc = _lib.hip_lib().hmse_l3_sha256(_ptr(data), data.numel(), _ptr(cuts), n_chunks, _ptr(out), ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_l3_sha256")
    return out


def l3_dedup(digests: torch.Tensor):
    """first_occ int64[n], refcount int32[n]. README.md:1288-1292."""
    _require_gpu(digests, "digests")
    n = digests.shape[0]
    dev = digests.device
    fo = _buf(n, torch.int64, dev)
    rc_t = _buf(n, torch.int32, dev)
    if n == 0:
        return fo, rc_t
    c = IngestConfig().to_c()
    nb = int(_lib.hip_lib().hmse_workspace_bytes(STAGE_DEDUP, n, C.byref(c)))
    ws = _ws(nb, dev)
    rc = _lib.hip_lib().hmse_l3_dedup(_ptr(digests), n, _ptr(fo), _ptr(rc_t), ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_l3_dedup")
    return fo, rc_t


def l3_index_slots(capacity_chunks: int) -> int:
    return int(_lib.hip_lib().hmse_l3_index_slots(int(capacity_chunks)))


def l3_index_update(digests_all: torch.Tensor, n_old: int, n_new: int, first_occ: torch.Tensor, refcount: torch.Tensor,
                    table: torch.Tensor) -> None:
    """Persistent L3 index: digests [n_old, n_old + n_new) join `table` (int32[l3_index_slots(capacity)], kept by the
    caller across calls); first_occ / refcount tails are written in place.  README.md:1288-1292."""
    for t, nm in ((digests_all, "digests"), (first_occ, "first_occ"), (refcount, "refcount"), (table, "table")):
        _require_gpu(t, nm)
    if digests_all.shape[0] < n_old + n_new or first_occ.numel() < n_old + n_new or refcount.numel() < n_old + n_new:
        raise HmseError(-1, "l3_index_update: arrays shorter than n_old + n_new")
    rc = _lib.hip_lib().hmse_l3_index_update(_ptr(digests_all), n_old, n_new, _ptr(first_occ), _ptr(refcount), _ptr(table), table.numel(), _stream())
    _check(rc, "hmse_l3_index_update")


def l4_lsh_slots(capacity_chunks: int) -> int:
    return int(_lib.hip_lib().hmse_l4_lsh_slots(int(capacity_chunks)))


def l4_lsh_update(sig_all: torch.Tensor, n_old: int, n_new: int, cfg: IngestConfig, band_keys: torch.Tensor, base: torch.Tensor | None,
                  tables: torch.Tensor, keys_given: bool = False) -> None:
    """Persistent L4b band tables: signatures [n_old, n_old + n_new) join `tables` (int32[bands, l4_lsh_slots(capacity)]);
    band_keys / base tails are written in place.  README.md:1554-1576, 1937-1945."""
    for t, nm in ((sig_all, "sig"), (band_keys, "band_keys"), (tables, "tables")):
        _require_gpu(t, nm)
    if sig_all.shape[0] < n_old + n_new or band_keys.shape[0] < n_old + n_new or (base is not None and base.numel() < n_old + n_new):
        raise HmseError(-1, "l4_lsh_update: arrays shorter than n_old + n_new")
    c = cfg.to_c()
    rc = _lib.hip_lib().hmse_l4_lsh_update(_ptr(sig_all), n_old, n_new, C.byref(c), _ptr(band_keys), _ptr(base), _ptr(tables), tables.shape[1],
                                          1 if keys_given else 0, _stream())
    _check(rc, "hmse_l4_lsh_update")


def l4_minhash(data: torch.Tensor, cuts: torch.Tensor, cfg: IngestConfig, chunk_ids: torch.Tensor | None = None,
               memo: bool = True) -> torch.Tensor:
    """MinHash signatures -> int32 [n_sel, 128] (uint32 bits). README.md:2578-2598.
    memo=False hands the C-ABI a workspace too small for its memo table (include/hmse.h): every hash is then computed."""
    _require_gpu(data, "data")
    _require_gpu(cuts, "cuts")
    if chunk_ids is not None:
        _require_gpu(chunk_ids, "chunk_ids")
    n_sel = (cuts.numel() - 1) if chunk_ids is None else chunk_ids.numel()
    sig = _buf((max(n_sel, 0), cfg.n_hashes), torch.int32, data.device)
    if n_sel <= 0:
        return sig
    c = cfg.to_c()
    ws = _ws(workspace_bytes(STAGE_MINHASH, n_sel, cfg) if memo else 256, data.device)
    rc = _lib.hip_lib().hmse_l4_minhash(_ptr(data), data.numel(), _ptr(cuts), _ptr(chunk_ids), n_sel, C.byref(c), _ptr(sig),
                                        ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_l4_minhash")
    return sig


def l4_lsh(sig: torch.Tensor, cfg: IngestConfig):
    """band keys int32 [n, bands], base int64 [n] (-1 = none). README.md:1375-1383, 1987-1996."""
    _require_gpu(sig, "sig")
    n = sig.shape[0]
    dev = sig.device
    keys = _buf((n, cfg.bands), torch.int32, dev)
    base = _buf(n, torch.int64, dev)
    if n == 0:
        return keys, base
    c = cfg.to_c()
    nb = int(_lib.hip_lib().hmse_workspace_bytes(STAGE_LSH, n, C.byref(c)))
    ws = _ws(nb, dev)
    rc = _lib.hip_lib().hmse_l4_lsh(_ptr(sig), n, C.byref(c), _ptr(keys), _ptr(base), ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_l4_lsh")
    return keys, base


def record_bytes(lens: torch.Tensor, has_dict=None) -> torch.Tensor:
    """hmse_l1_deflate_record_bytes() — where `has_dict` (bool tensor) is set: hmse_l1_deflate_record_bytes_dict() — for a
    tensor of chunk lengths (0 above 32768: such a chunk is never encoded)."""
    body = 1296 + 4 * ((lens + 3) & ~3)
    if has_dict is not None:
        body = body + torch.where(has_dict, lens + 21, torch.zeros_like(lens))
    return torch.where(lens <= 32768, (body + 255) & ~255, torch.zeros_like(lens))


DEFLATE_WS_LIMIT = 64 << 30   # upper bound of the per-job records one hmse_l1_deflate call may hold (l1_deflate splits a larger selection)


def deflate_ws_limit(device) -> int:
    """Record workspace one hmse_l1_deflate call may take: at most DEFLATE_WS_LIMIT and at most half of the HBM that is free
    right now (cached blocks of the allocator count as free) — a resident corpus, streams and index then still fit beside it."""
    free, _ = torch.cuda.mem_get_info(device)
    cached = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    return max(256 << 20, min(DEFLATE_WS_LIMIT, (free + cached) // 2))


# windows T = dictionary + chunk of the match kernel's size classes S, S2, SG, SG2, SG3 (hmse_amd/csrc/l1_deflate.hip: HMSE_TCAP_*; above: class B) —
# diagnostics only (bench.py's per-class algorithmic bytes, tools/): the library classifies on the device
DEFLATE_CLASS_CAPS = (10048, 13952, 17408, 22976, 32768)


def l1_deflate(data: torch.Tensor, cuts: torch.Tensor, cfg: IngestConfig, chunk_ids: torch.Tensor | None = None,
               base: torch.Tensor | None = None, base_is_chunk_id: bool = False, ws: torch.Tensor | None = None,
               ws_limit: int | None = None):
    """Per-chunk raw DEFLATE with the base chunk as dictionary (`base`: index into the selection, or — with
    base_is_chunk_id — a chunk index into `cuts`, e.g. a chunk stored by an earlier batch of a stream).

    The C-ABI call keeps one record per chunk (histograms, token list sized for the all-literal worst case — the FULL stream
    later overwrites it; a chunk with a dictionary has the DELTA stream's slot behind it: ~4.2 / 5.2 x the chunk) in its workspace.  A selection whose records exceed `ws_limit`
    bytes (default DEFLATE_WS_LIMIT) is encoded in consecutive pieces that each fit — same streams, same order, a bounded
    workspace whatever the shard size.

    Returns (out uint8[total], out_off int64[n_sel+1], kind uint8[n_sel]). README.md:2374-2378, 2182-2189."""
    if ws is not None:
        _require_gpu(ws, "ws")
    _require_gpu(data, "data")
    _require_gpu(cuts, "cuts")
    dev = data.device
    n_sel = (cuts.numel() - 1) if chunk_ids is None else chunk_ids.numel()
    out_off = _buf(max(n_sel, 0) + 1, torch.int64, dev, fill=0)
    kind = _buf(max(n_sel, 0), torch.uint8, dev, fill=0)
    if n_sel <= 0:
        return _buf(0, torch.uint8, dev), out_off, kind
    lens = (cuts[1:] - cuts[:-1]) if chunk_ids is None else (cuts[chunk_ids + 1] - cuts[chunk_ids])
    # per-chunk record of the C-ABI workspace = hmse_l1_deflate_record_bytes[_dict](len), evaluated on the device;
    # tests/test_abi.py holds the formulas together
    rec = record_bytes(lens, None if base is None else base >= 0)
    raw, need = (int(v) for v in torch.stack([lens.sum(), rec.sum()]).tolist())
    cap = raw + 5 * n_sel + 64  # a stored block is the worst case
    out = _buf(cap, torch.uint8, dev)
    status = _buf(1, torch.int32, dev, fill=0)
    c = cfg.to_c()
    limit = deflate_ws_limit(dev) if ws_limit is None else int(ws_limit)
    if need <= limit:
        pieces = [(0, n_sel, need)]
        ids_all, base_all, by_id = chunk_ids, base, base_is_chunk_id
    else:
        # consecutive pieces of the selection whose records fit; dictionaries are named by chunk id so that a piece may
        # use a chunk of an earlier piece
        csum = torch.cumsum(rec, 0)
        ends, lo, start = [], 0, 0
        while start < n_sel:
            e = int(torch.searchsorted(csum, torch.tensor([lo + limit], dtype=csum.dtype, device=dev), right=True).item())
            e = max(e, start + 1)
            ends.append(e); lo = int(csum[e - 1].item()); start = e
        cs = [0] + [int(csum[e - 1].item()) for e in ends]
        pieces = [(a, e, cs[i + 1] - cs[i]) for i, (a, e) in enumerate(zip([0] + ends[:-1], ends))]
        ids_all = chunk_ids if chunk_ids is not None else torch.arange(n_sel, dtype=torch.int64, device=dev)
        base_all = None if base is None else (base if base_is_chunk_id else torch.where(base >= 0, ids_all[base.clamp(min=0)], base))
        by_id = True
        out_off[:1] = 0     # (the pieces' offsets are copied behind it: the one element no call writes)
    total = 0
    for a, e, need_p in pieces:
        n_p = e - a
        nb = int(_lib.hip_lib().hmse_workspace_bytes(STAGE_DEFLATE, n_p, C.byref(c)))
        if ws is None or ws.numel() < nb + need_p + 4096:   # (`ws`: a caller-held workspace, e.g. the streaming front end's, reused when big enough)
            ws = None
            ws = _ws(nb + need_p + 4096, dev)
        ids_p = None if ids_all is None else ids_all[a:e]
        base_p = None if base_all is None else base_all[a:e]
        off_p = out_off[a: e + 1] if len(pieces) == 1 else _buf(n_p + 1, torch.int64, dev, fill=0)
        rc = _lib.hip_lib().hmse_l1_deflate_ex(_ptr(data), data.numel(), _ptr(cuts), _ptr(ids_p), _ptr(base_p), n_p, C.byref(c),
                                               1 if by_id else 0, out.data_ptr() + total, cap - total, _ptr(off_p), _ptr(kind[a:e]), _ptr(status),
                                               ws.data_ptr(), ws.numel(), _stream())
        _check(rc, "hmse_l1_deflate")
        st, tot_p = (int(v) for v in torch.stack([status[0].to(torch.int64), off_p[-1]]).tolist())
        if st:
            raise HmseError(-2, f"hmse_l1_deflate device status {st:#x}")
        if len(pieces) > 1:
            out_off[a + 1: e + 1] = off_p[1:] + total
        total += tot_p
    return out[:total], out_off, kind


def l1_inflate_mode(mode: int) -> None:
    """0: pick the decoder by stream count (default); 1: one stream per wavefront; 2: one stream per lane (include/hmse.h)."""
    _check(_lib.hip_lib().hmse_l1_inflate_mode(int(mode)), "hmse_l1_inflate_mode")


def l1_inflate(streams: torch.Tensor, stream_off: torch.Tensor, kind: torch.Tensor, base: torch.Tensor | None,
               raw_len: torch.Tensor, stream_len: torch.Tensor | None = None, check: bool = True):
    """Raw-DEFLATE decode of stored chunks; DELTA chunks use their base chunk's raw bytes as dictionary.

    `stream_off` int64[n+1] (dense) or int64[n] starts with `stream_len` int32[n]; `raw_len` int64[n] raw chunk sizes.
    Returns (raw uint8[sum(raw_len)], raw_off int64[n+1], ok uint8[n]); with check=True a corrupt record raises.
    README.md:2397-2400, 1635-1669."""
    _require_gpu(streams, "streams")
    _require_gpu(stream_off, "stream_off")
    _require_gpu(kind, "kind")
    _require_gpu(raw_len, "raw_len")
    dev = streams.device
    n_sel = kind.numel()
    if stream_off.numel() != (n_sel if stream_len is not None else n_sel + 1) or raw_len.numel() != n_sel:
        raise HmseError(-1, "l1_inflate: stream_off / raw_len do not match kind")
    raw_off = _buf(n_sel + 1, torch.int64, dev)
    raw_off[:1] = 0        # (an input of the call, built here: exclusive sums of raw_len)
    torch.cumsum(raw_len, 0, out=raw_off[1:])
    total = int(raw_off[-1].item()) if n_sel else 0
    raw = _buf(total, torch.uint8, dev)
    status = _buf(1, torch.int32, dev, fill=0)
    ok = _buf(n_sel, torch.uint8, dev, fill=0)
    if n_sel == 0:
        return raw, raw_off, ok
    if base is not None:
        _require_gpu(base, "base")
    if stream_len is not None:
        _require_gpu(stream_len, "stream_len")
    ws = _ws(workspace_bytes(STAGE_INFLATE, n_sel, IngestConfig()), dev)
    keep = _buf(1, torch.uint8, dev) if total == 0 else raw  # a valid pointer even when every chunk is empty
    rc = _lib.hip_lib().hmse_l1_inflate(_ptr(streams), streams.numel(), _ptr(stream_off), _ptr(stream_len), _ptr(kind), _ptr(base),
                                        n_sel, _ptr(raw_off), _ptr(keep), total, _ptr(ok), _ptr(status), ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_l1_inflate")
    st = int(status.item())
    if check and st:
        raise HmseError(-1, f"hmse_l1_inflate: {int((ok == 0).sum().item())} corrupt record(s), device status {st:#x}")
    return raw, raw_off, ok


def read_assemble(cuts: torch.Tensor, slot_of_chunk: torch.Tensor, raw_off: torch.Tensor, raw: torch.Tensor) -> torch.Tensor:
    """Lay the stored chunks out as the original data: chunk i <- raw bytes of slot_of_chunk[i]. README.md:1635-1669."""
    for t, nm in ((cuts, "cuts"), (slot_of_chunk, "slot_of_chunk"), (raw_off, "raw_off"), (raw, "raw")):
        _require_gpu(t, nm)
    n_chunks = cuts.numel() - 1
    n = int(cuts[-1].item()) if n_chunks > 0 else 0
    out = _buf(n, torch.uint8, cuts.device)
    status = _buf(1, torch.int32, cuts.device, fill=0)
    if n_chunks <= 0 or n == 0:
        return out
    rc = _lib.hip_lib().hmse_read_assemble(_ptr(cuts), n_chunks, _ptr(slot_of_chunk), raw_off.numel() - 1, _ptr(raw_off), _ptr(raw),
                                           _ptr(out), n, _ptr(status), _stream())
    _check(rc, "hmse_read_assemble")
    if int(status.item()):
        raise HmseError(-1, "hmse_read_assemble: chunk map disagrees with the stored lengths")
    return out


def manifest_pack(res, shard: int, n_shards: int, shard_bases, rec_off: torch.Tensor, lba_unit: int, ptr_index: torch.Tensor,
                  blob: torch.Tensor, index: torch.Tensor, chunk_map: torch.Tensor, pointers: torch.Tensor, any_target: bool = False) -> None:
    """hmse_manifest_pack over a ShardResult: blob, ChunkIndex table, chunk map and pointer records written in place.
    README.md:1263-1270, 2182-2189, 1312, 1448."""
    for t, nm in ((res.cuts, "cuts"), (res.uniq_ids, "uniq_ids"), (res.streams, "streams"), (res.stream_off, "stream_off"), (res.kind, "kind"),
                  (rec_off, "rec_off"), (ptr_index, "ptr_index"), (blob, "blob"), (index, "index"), (chunk_map, "chunk_map"), (pointers, "pointers")):
        _require_gpu(t, nm)
    dev = res.cuts.device
    n = res.cuts.numel() - 1
    status = _buf(1, torch.int32, dev, fill=0)
    ws = _ws(workspace_bytes(STAGE_MANIFEST, n, IngestConfig()), dev)
    base = res.base if res.base is not None else torch.full((res.uniq_ids.numel(),), -1, dtype=torch.int64, device=dev)   # (an input, built here)
    if res.base_global is not None:   # dictionaries stored on other shards: -2 (an unresolved DeltaChunk header)
        base = torch.where((res.base_global >= 0) & (base < 0), torch.full_like(base, -2), base)
    sb = None
    if n_shards > 1:
        sb = torch.as_tensor(list(shard_bases), dtype=torch.int64, device=dev)
        if sb.numel() != n_shards:
            raise HmseError(-1, "manifest_pack: one chunk base per shard")
    keep = blob if blob.numel() else _buf(1, torch.uint8, dev)
    rc = _lib.hip_lib().hmse_manifest_pack_ex(_ptr(res.streams), _ptr(res.stream_off), _ptr(res.kind), _ptr(base), _ptr(res.uniq_ids),
                                          res.uniq_ids.numel(), _ptr(res.digests), _ptr(res.refcount), _ptr(res.cuts), n, _ptr(res.first_occ),
                                          int(res.chunk_base), shard, _ptr(sb), n_shards, 1 if any_target else 0, _ptr(rec_off), lba_unit, _ptr(ptr_index), _ptr(keep),
                                          blob.numel(), _ptr(index), _ptr(chunk_map), _ptr(pointers) if pointers.numel() else None,
                                          pointers.shape[0], _ptr(status), ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_manifest_pack")
    st = int(status.item())
    if st:
        raise HmseError(-2, f"hmse_manifest_pack device status {st:#x}")


def gc_plan(cuts: torch.Tensor, slot: torch.Tensor, n_slots: int, seg_off: torch.Tensor, drop: torch.Tensor, digests_old: torch.Tensor) -> dict:
    """hmse_gc_plan: the old chunk map (`cuts` int64[n+1], `slot` int32[n]) and the dropped segments (`seg_off` int64[n_seg+1], `drop`
    uint8[n_seg]) -> the L3 arrays of the surviving store as a fresh ingest of the remainder numbers them.  `digests_old` uint8[n_slots, 32].
    Returns {old_chunk, first_occ, refcount, digests, uniq_ids, old_slot (int64[u_new]), new_slot_of_old (int64[n_slots], -1 gone)}.
    README.md:1268, 1886 (the refcount kept for garbage collection)."""
    for t, nm in ((cuts, "cuts"), (slot, "slot"), (seg_off, "seg_off"), (drop, "drop"), (digests_old, "digests_old")):
        _require_gpu(t, nm)
    dev = cuts.device
    n = cuts.numel() - 1
    n_seg = seg_off.numel() - 1
    if slot.numel() != n or drop.numel() != n_seg or digests_old.shape != (n_slots, 32) or n_seg < 1:
        raise HmseError(-1, "gc_plan: slot / drop / digests_old do not match cuts / seg_off / n_slots")
    counts = _buf(2, torch.int64, dev, fill=0)
    status = _buf(1, torch.int32, dev, fill=0)
    e = lambda *shape, dt=torch.int64: _buf(shape, dt, dev)
    old_chunk, first_occ, refcount, digests = e(max(n, 1)), e(max(n, 1)), e(max(n, 1), dt=torch.int32), e(max(n, 1), 32, dt=torch.uint8)
    uniq_ids, old_slot, new_slot_of_old = e(max(n_slots, 1)), e(max(n_slots, 1)), e(max(n_slots, 1))
    ws = _ws(workspace_bytes(STAGE_GC_PLAN, n, IngestConfig()), dev)
    rc = _lib.hip_lib().hmse_gc_plan(_ptr(cuts), n, _ptr(slot), int(n_slots), _ptr(seg_off), n_seg, _ptr(drop), _ptr(digests_old), _ptr(counts),
                                     _ptr(old_chunk), _ptr(first_occ), _ptr(refcount), _ptr(digests), _ptr(uniq_ids), _ptr(old_slot),
                                     _ptr(new_slot_of_old), _ptr(status), ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_gc_plan")
    n_new, u_new, st = (int(v) for v in torch.cat([counts, status.to(torch.int64)]).tolist())   # the one host sync: output sizes
    if st:
        raise HmseError(-2, f"hmse_gc_plan device status {st:#x}")
    if n_new > n or u_new > min(n_new, n_slots):
        raise HmseError(-2, f"hmse_gc_plan: {n_new} chunks / {u_new} slots survive of {n} / {n_slots}")
    if u_new:   # every index the caller will gather with lies inside its array (torch's device-side indexing does not check)
        lim = torch.stack([old_chunk[:n_new].min(), old_chunk[:n_new].max(), uniq_ids[:u_new].min(), uniq_ids[:u_new].max(),
                           old_slot[:u_new].min(), old_slot[:u_new].max()]).tolist()
        if lim[0] < 0 or lim[1] >= n or lim[2] < 0 or lim[3] >= n_new or lim[4] < 0 or lim[5] >= n_slots:
            raise HmseError(-2, f"hmse_gc_plan: an index outside its array ({lim})")
    return {"old_chunk": old_chunk[:n_new], "first_occ": first_occ[:n_new], "refcount": refcount[:n_new], "digests": digests[:n_new],
            "uniq_ids": uniq_ids[:u_new], "old_slot": old_slot[:u_new], "new_slot_of_old": new_slot_of_old[:n_slots]}


def record_gather(src0: torch.Tensor, src1: torch.Tensor | None, src_off: torch.Tensor, src_sel: torch.Tensor, dst_off: torch.Tensor,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """hmse_record_gather: record k = bytes [src_off[k], + dst_off[k+1] - dst_off[k]) of (src1 if src_sel[k] else src0), laid out
    densely at dst_off (int64[n+1]).  Returns the uint8 destination (`out`, or a new tensor of dst_off[-1] bytes)."""
    srcs = [src0] + ([src1] if src1 is not None else [])
    for t, nm in [(t, "src") for t in srcs] + [(src_off, "src_off"), (src_sel, "src_sel"), (dst_off, "dst_off")]:
        _require_gpu(t, nm)
    dev = dst_off.device
    n = src_sel.numel()
    if src_off.numel() != n or dst_off.numel() != n + 1:
        raise HmseError(-1, "record_gather: src_off / src_sel / dst_off do not match")
    if out is None:
        out = _buf(int(dst_off[-1].item()), torch.uint8, dev)
    _require_gpu(out, "out")
    status = _buf(1, torch.int32, dev, fill=0)
    keep = lambda t: t if t is not None and t.numel() else None
    rc = _lib.hip_lib().hmse_record_gather(_ptr(keep(src0)), src0.numel(), _ptr(keep(src1)), 0 if src1 is None else src1.numel(), _ptr(src_off),
                                           _ptr(src_sel), _ptr(dst_off), n, _ptr(out) if out.numel() else None, out.numel(), _ptr(status), _stream())
    _check(rc, "hmse_record_gather")
    if n and int(status.item()):
        raise HmseError(-2, "hmse_record_gather: a record lies outside its source or the destination")
    return out


def sync_match(a: torch.Tensor, a_off: torch.Tensor, a_len: torch.Tensor, b: torch.Tensor, b_off: torch.Tensor, b_len: torch.Tensor,
               cand: torch.Tensor):
    """hmse_sync_match: same[k] = 1 iff record k of a — bytes [a_off[k], + a_len[k]) — and record cand[k] of b are byte-identical
    (cand < 0: no candidate, 0).  a, b uint8; a_off, b_off int64; a_len, b_len int32; cand int64.  Returns (same uint8[n], status):
    status bit 0 = a candidate >= len(b_off) or a record that reaches outside its blob (same is 0 there; nothing outside is read)."""
    for t, nm in ((a, "a"), (a_off, "a_off"), (a_len, "a_len"), (b, "b"), (b_off, "b_off"), (b_len, "b_len"), (cand, "cand")):
        _require_gpu(t, nm)
    for t, nm, dt in ((a, "a", torch.uint8), (b, "b", torch.uint8), (a_off, "a_off", torch.int64), (b_off, "b_off", torch.int64),
                      (a_len, "a_len", torch.int32), (b_len, "b_len", torch.int32), (cand, "cand", torch.int64)):
        if t.dtype != dt:
            raise HmseError(-1, f"sync_match: {nm} must be {dt}")
    n, n_b = cand.numel(), b_off.numel()
    if a_off.numel() != n or a_len.numel() != n or b_len.numel() != n_b:
        raise HmseError(-1, "sync_match: a_off / a_len / cand or b_off / b_len do not match")
    dev = cand.device
    same = _buf(n, torch.uint8, dev)
    status = _buf(1, torch.int32, dev, fill=0)
    keep = lambda t: _ptr(t) if t.numel() else None
    rc = _lib.hip_lib().hmse_sync_match(keep(a), a.numel(), keep(a_off), keep(a_len), n, keep(b), b.numel(), keep(b_off), keep(b_len), n_b,
                                        keep(cand), keep(same), _ptr(status), _stream())
    _check(rc, "hmse_sync_match")
    return same, int(status.item())


def stream_batch_workspace_bytes(batch_bytes: int, cfg: IngestConfig) -> int:
    c = cfg.to_c()
    return int(_lib.hip_lib().hmse_stream_batch_workspace_bytes(int(batch_bytes), C.byref(c)))


def stream_workspace(batch_bytes: int, cfg: IngestConfig, device) -> torch.Tensor:
    """A workspace for hmse_stream_batch / hmse_stream_piece_*: allocated and prepared once (hmse_stream_workspace_init: the MinHash
    memo table inside persists across the stream's batches), then passed to every batch."""
    ws = _ws(stream_batch_workspace_bytes(batch_bytes, cfg), device)
    c = cfg.to_c()
    _check(_lib.hip_lib().hmse_stream_workspace_init(ws.data_ptr(), ws.numel(), int(batch_bytes), C.byref(c), _stream()), "hmse_stream_workspace_init")
    return ws


class StreamArrays:
    """A stream's descriptor (include/hmse.h: hmse_stream), built ONCE per stream from keyword arguments named after the struct's fields: a tensor gives
    its address (checked and kept alive here), anything else is a capacity or world / rank; None is NULL (the library refuses a call that misses a field)."""

    def __init__(self, **fields):
        fields = {k: v for k, v in fields.items() if v is not None}
        self.tensors = {k: v for k, v in fields.items() if isinstance(v, torch.Tensor)}
        for k, t in self.tensors.items():
            _require_gpu(t, k)
        self.c = _lib.HmseStream(struct_size=C.sizeof(_lib.HmseStream), **{k: v.data_ptr() if k in self.tensors else int(v) for k, v in fields.items()})


def _stream_call(name: str, *args, **tensors) -> None:
    """One streaming entry point: `args`, then the workspace and the stream.  `tensors`: what it gets besides the descriptor (None: absent)."""
    for nm, t in tensors.items():
        if t is not None:
            _require_gpu(t, nm)
    ws = tensors["ws"]
    _check(getattr(_lib.hip_lib(), name)(*args, ws.data_ptr(), ws.numel(), _stream()), name)


def stream_batch(data: torch.Tensor, batch_bytes: int, seg_off: torch.Tensor, cfg: IngestConfig, s: StreamArrays, ws: torch.Tensor,
                 data_origin: int = 0) -> None:
    """hmse_stream_batch: the whole per-batch chain (L2 -> L3 -> index -> L4 -> band tables -> L1) enqueued without a host
    read; capturable into a hipGraph (hmse_amd/stream.py).  README.md:1519-1580."""
    # data_origin: `data` holds the stream's bytes [data_origin, data_origin + data.numel()) — the resident WINDOW of a stream longer than
    # the buffer (stream.StreamIngest(window_bytes=)); the chain addresses bytes by stream offset, so it gets the buffer's address minus the origin
    _stream_call("hmse_stream_batch", data.data_ptr() - int(data_origin), int(data_origin) + data.numel(), int(batch_bytes), _ptr(seg_off),
                 seg_off.numel() - 1, C.byref(cfg.to_c()), C.byref(s.c), data=data, seg_off=seg_off, ws=ws)


def stream_row_bytes(cap_bytes: int, cfg: IngestConfig) -> int:
    c = cfg.to_c()
    return int(_lib.hip_lib().hmse_stream_row_bytes(int(cap_bytes), C.byref(c)))


def stream_piece_hash(data: torch.Tensor, piece_bytes: int, cap_bytes: int, seg_off: torch.Tensor | None, cfg: IngestConfig, s: StreamArrays,
                      row: torch.Tensor, ws: torch.Tensor) -> None:
    """hmse_stream_piece_hash: phase A of a multi-rank stream's batch (L2 + L3 hash of this rank's piece -> its exchange row).
    README.md:1519-1540."""
    _stream_call("hmse_stream_piece_hash", _ptr(data), data.numel(), int(piece_bytes), int(cap_bytes), _ptr(seg_off),
                 0 if seg_off is None else seg_off.numel() - 1, C.byref(cfg.to_c()), C.byref(s.c), _ptr(row), data=data, seg_off=seg_off, row=row, ws=ws)


def stream_piece_encode(data: torch.Tensor, piece_bytes: int, cap_bytes: int, cfg: IngestConfig, s: StreamArrays, rows: torch.Tensor,
                        ws: torch.Tensor) -> None:
    """hmse_stream_piece_encode: phase B (gathered rows -> global index -> this rank's stored chunks -> L4 -> L1).  README.md:1538-1580."""
    if rows.numel() != s.c.world * stream_row_bytes(cap_bytes, cfg):
        raise HmseError(-1, "stream_piece_encode: rows must hold one exchange row per rank")
    _stream_call("hmse_stream_piece_encode", _ptr(data), data.numel(), int(piece_bytes), int(cap_bytes), C.byref(cfg.to_c()), C.byref(s.c), _ptr(rows),
                 data=data, rows=rows, ws=ws)


# ---- global L4 of a multi-rank stream as captured phases (include/hmse.h: hmse_gl4) ---------------------------------------------
def stream_sig_cap(cap_bytes: int, cfg: IngestConfig) -> int:
    c = cfg.to_c()
    return int(_lib.hip_lib().hmse_stream_sig_cap(int(cap_bytes), C.byref(c)))


def stream_sig_row_bytes(cap_bytes: int, cfg: IngestConfig) -> int:
    c = cfg.to_c()
    return int(_lib.hip_lib().hmse_stream_sig_row_bytes(int(cap_bytes), C.byref(c)))


def stream_piece_sign(data, piece_bytes, cap_bytes, cfg, s: StreamArrays, rows, sig_row, ws) -> None:
    """hmse_stream_piece_sign: gathered digest rows -> global index -> this rank's new stored chunks -> MinHash -> its signature row."""
    _stream_call("hmse_stream_piece_sign", _ptr(data), data.numel(), int(piece_bytes), int(cap_bytes), C.byref(cfg.to_c()), C.byref(s.c), _ptr(rows), _ptr(sig_row),
                 data=data, rows=rows, sig_row=sig_row, ws=ws)


def stream_piece_bases(cap_bytes, cfg, s: StreamArrays, sig_rows, gl4, ws) -> None:
    """hmse_stream_piece_bases: gathered signature rows -> global band tables -> dictionaries of this rank's new stored chunks + requests.
    `gl4`: a _lib.HmseGl4 (kept alive by the caller together with the tensors it points to)."""
    _stream_call("hmse_stream_piece_bases", int(cap_bytes), C.byref(cfg.to_c()), C.byref(s.c), _ptr(sig_rows), C.byref(gl4), sig_rows=sig_rows, ws=ws)


def stream_piece_encode_g(data, piece_bytes, cap_bytes, cfg, s: StreamArrays, gstate, ws) -> None:
    """hmse_stream_piece_encode_g: DEFLATE of the new stored chunks with the dictionaries resolved by stream_piece_bases, tails, states advanced."""
    _stream_call("hmse_stream_piece_encode_g", _ptr(data), data.numel(), int(piece_bytes), int(cap_bytes), C.byref(cfg.to_c()), C.byref(s.c), _ptr(gstate),
                 data=data, gstate=gstate, ws=ws)


def band_tables_write(keys: torch.Tensor, sig: torch.Tensor | None, band_bits: int) -> torch.Tensor:
    """hmse_band_tables_write: the band-table sidecar of `keys` (int32 [n, bands], uint32 bits) and, when given, the signatures
    (int32 [n, n_hashes]) -> a device uint8 tensor, byte for byte bandtable.write_band_tables().  One host sync (the size)."""
    _require_gpu(keys, "keys")
    if keys.dim() != 2 or keys.dtype != torch.int32:
        raise HmseError(-1, "band_tables_write: keys must be int32 [n, bands]")
    n, bands = keys.shape
    nh = 0
    if sig is not None:
        _require_gpu(sig, "sig")
        if sig.dim() != 2 or sig.dtype != torch.int32 or sig.shape[0] != n:
            raise HmseError(-1, "band_tables_write: sig must be int32 [n, n_hashes]")
        nh = int(sig.shape[1])
    if n >= 1 << 24:
        raise ValueError("3-byte chunk ids hold at most 16 777 215 stored chunks (README.md:1943)")
    if not 1 <= band_bits <= 16:
        raise ValueError("band_hash is a u16")
    dev = keys.device
    lib = _lib.hip_lib()
    cap = int(lib.hmse_band_tables_bound(n, bands, band_bits, nh))
    out = _buf(cap, torch.uint8, dev)
    meta = _buf(2, torch.int64, dev, fill=0)      # [out_bytes, status]
    ws = _ws(lib.hmse_band_tables_workspace_bytes(n), dev)
    rc = lib.hmse_band_tables_write(_ptr(keys) if n else None, n, bands, band_bits, _ptr(sig) if n and nh else None, nh, out.data_ptr(), cap,
                                    meta.data_ptr(), meta.data_ptr() + 8, ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_band_tables_write")
    size, st = (int(v) for v in meta.tolist())
    if st & 0xFFFFFFFF:
        raise HmseError(-2, f"hmse_band_tables_write device status {st & 0xFFFFFFFF:#x}")
    if size > cap:
        raise HmseError(-2, f"hmse_band_tables_write: {size} bytes written into {cap}")
    return out[:size]


def search_cfg(cfg: IngestConfig, bands: int) -> IngestConfig:
    """`cfg` with the search banding bands x (128 / bands); ValueError unless hmse_cfg_validate accepts it (bands in 1, 2, 4, 8, 16)."""
    if int(bands) not in (1, 2, 4, 8, 16) or cfg.n_hashes != 128:
        raise ValueError(f"a search banding is bands x rows = 128 with bands in (1, 2, 4, 8, 16), got bands={bands} (n_hashes {cfg.n_hashes})")
    sc = cfg.with_(bands=int(bands), rows=128 // int(bands))
    c = sc.to_c()
    if _lib.hip_lib().hmse_cfg_validate(C.byref(c)) != 0:
        raise ValueError(f"configuration {sc} is not supported by the device path")
    return sc


def l4_index_build(keys: torch.Tensor):
    """hmse_l4_index_build: band keys int32 [n, bands] (uint32 bits) -> (sorted_keys, sorted_ids), int32 [bands, n] each: per band the
    ids sorted stably by their key in uint32 order."""
    _require_gpu(keys, "keys")
    if keys.dim() != 2 or keys.dtype != torch.int32:
        raise HmseError(-1, "l4_index_build: keys must be int32 [n, bands]")
    n, bands = keys.shape
    dev = keys.device
    sk = _buf((bands, n), torch.int32, dev)
    si = _buf((bands, n), torch.int32, dev)
    status = _buf(1, torch.int32, dev, fill=0)
    ws = _ws(workspace_bytes(STAGE_L4_INDEX, n, search_cfg(IngestConfig(), bands)) if bands in (1, 2, 4, 8, 16) else 256, dev)
    rc = _lib.hip_lib().hmse_l4_index_build(_ptr(keys) if n else None, n, bands, sk.data_ptr() if n else None, si.data_ptr() if n else None,
                                            status.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_l4_index_build")
    return sk, si


def l4_query(sig_q: torch.Tensor, keys_q: torch.Tensor, sig_s: torch.Tensor, sorted_keys: torch.Tensor, sorted_ids: torch.Tensor,
             cfg: IngestConfig, top_k: int = 8, min_score: int = 0, exclude_self: bool = False):
    """hmse_l4_query under the banding of `cfg` -> (ids int64 [q, top_k] (-1 padding), scores int32 [q, top_k] (0 padding),
    n_hits int32 [q], n_candidates int64 [q]).  One host sync (the status word)."""
    for t, name in ((sig_q, "sig_q"), (keys_q, "keys_q"), (sig_s, "sig_s"), (sorted_keys, "sorted_keys"), (sorted_ids, "sorted_ids")):
        _require_gpu(t, name)
    n_q, n_s = sig_q.shape[0], sig_s.shape[0]
    if sig_q.shape[1:] != (128,) or sig_s.shape[1:] != (128,) or keys_q.shape != (n_q, cfg.bands) or \
            sorted_keys.shape != (cfg.bands, n_s) or sorted_ids.shape != (cfg.bands, n_s):
        raise HmseError(-1, "l4_query: shapes of the signatures, keys and index do not agree with each other or with the banding")
    dev = sig_q.device
    ids = _buf((n_q, int(top_k)), torch.int64, dev)
    scores = _buf((n_q, int(top_k)), torch.int32, dev)
    n_hits = _buf(n_q, torch.int32, dev)
    n_cand = _buf(n_q, torch.int64, dev)
    status = _buf(1, torch.int32, dev, fill=0)
    c = cfg.to_c()
    ws = _ws(workspace_bytes(STAGE_L4_QUERY, n_q, cfg), dev)
    q = lambda t: _ptr(t) if n_q else None
    s = lambda t: _ptr(t) if n_s else None
    rc = _lib.hip_lib().hmse_l4_query(q(sig_q), q(keys_q), n_q, s(sig_s), n_s, s(sorted_keys), s(sorted_ids), C.byref(c), int(top_k),
                                      int(min_score), QUERY_EXCLUDE_SELF if exclude_self else 0, q(ids), q(scores), q(n_hits), q(n_cand),
                                      status.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_l4_query")
    st = int(status.item())
    if st:
        raise HmseError(-1, f"hmse_l4_query device status {st:#x}: an index entry names an id outside the stored signatures")
    return ids, scores, n_hits, n_cand


def scrub_records(blob: torch.Tensor, rec_shard: torch.Tensor, shard_blob: torch.Tensor, shard_slot: torch.Tensor, lba_unit: torch.Tensor,
                  lba: torch.Tensor, rec_len: torch.Tensor, kind: torch.Tensor, remote: torch.Tensor, sorted_lba: torch.Tensor,
                  sorted_slot: torch.Tensor, steps: int, meta: torch.Tensor):
    """hmse_scrub_records: per record (global slot) its STRUCTURE / HEADER flags and resolved dictionary, plus the non-zero padding
    bytes of the blobs.  u32 arrays travel as int32.  Returns (status uint8[n], dict int64[n], padding int64[1]) on the device."""
    tensors = (blob, rec_shard, shard_blob, shard_slot, lba_unit, lba, rec_len, kind, remote, sorted_lba, sorted_slot, meta)
    for t, nm in zip(tensors, ("blob", "rec_shard", "shard_blob", "shard_slot", "lba_unit", "lba", "rec_len", "kind", "remote", "sorted_lba",
                               "sorted_slot", "meta")):
        _require_gpu(t, nm)
    dev = blob.device
    n = lba.numel()
    n_shards = lba_unit.numel()
    if any(t.numel() != n for t in (rec_shard, rec_len, kind, remote, sorted_lba, sorted_slot, meta)) or shard_blob.numel() != n_shards + 1 \
            or shard_slot.numel() != n_shards + 1:
        raise HmseError(-1, "scrub_records: per-record / per-shard arrays do not match")
    status = _buf(max(n, 1), torch.uint8, dev, fill=0)
    dict_ = _buf(max(n, 1), torch.int64, dev, fill=-1)
    pad = _buf(1, torch.int64, dev, fill=0)
    if n_shards == 0:
        return status[:0], dict_[:0], pad
    p = lambda t: _ptr(t) if t.numel() else None
    rc = _lib.hip_lib().hmse_scrub_records(_ptr(blob), blob.numel(), n, n_shards, p(rec_shard), p(shard_blob), p(shard_slot), p(lba_unit),
                                           p(lba), p(rec_len), p(kind), p(remote), p(sorted_lba), p(sorted_slot), int(steps), p(meta), _ptr(status),
                                           _ptr(dict_), _ptr(pad), _stream())
    _check(rc, "hmse_scrub_records")
    return status[:n], dict_[:n], pad


def scrub_attribute(status: torch.Tensor, dict_: torch.Tensor, ok: torch.Tensor, got: torch.Tensor, want: torch.Tensor, check_digest: bool,
                    chunk_slot: torch.Tensor, cuts: torch.Tensor, max_depth_log2: int) -> dict:
    """hmse_scrub_attribute: final record flags and roots, chunk roots, per-root losses and the damaged ranges.  Returns device
    tensors {status, root, chunk_root, root_records, root_chunks, root_bytes, ranges (u64[2 (n_chunks / 2 + 1)]), counts (u64[8])}."""
    for t, nm in ((status, "status"), (dict_, "dict"), (ok, "ok"), (got, "got"), (want, "want"), (chunk_slot, "chunk_slot"), (cuts, "cuts")):
        _require_gpu(t, nm)
    dev = cuts.device
    n, nc = status.numel(), chunk_slot.numel()
    if dict_.numel() != n or ok.numel() != n or cuts.numel() != nc + 1 or (check_digest and (got.shape != (n, 32) or want.shape != (n, 32))):
        raise HmseError(-1, "scrub_attribute: per-record / per-chunk arrays do not match")
    e = lambda k, dt=torch.int64: _buf(max(k, 1), dt, dev, fill=0)
    out = {"status": e(n, torch.uint8), "root": e(n), "chunk_root": e(nc), "root_records": e(n), "root_chunks": e(n), "root_bytes": e(n),
           "ranges": e(2 * (nc // 2 + 1)), "counts": e(8)}
    ws = _ws(workspace_bytes(STAGE_SCRUB_ATTRIBUTE, max(n, nc), IngestConfig()), dev)
    p = lambda t, keep=True: _ptr(t) if keep and t.numel() else None
    rc = _lib.hip_lib().hmse_scrub_attribute(n, p(status), p(dict_), p(ok), p(got, check_digest), p(want, check_digest), 1 if check_digest else 0,
                                             int(max_depth_log2), nc, p(chunk_slot), _ptr(cuts), _ptr(out["status"]), _ptr(out["root"]),
                                             _ptr(out["chunk_root"]), _ptr(out["root_records"]), _ptr(out["root_chunks"]), _ptr(out["root_bytes"]),
                                             _ptr(out["ranges"]), _ptr(out["counts"]), ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "hmse_scrub_attribute")
    return out


def _find_bounds(pat: torch.Tensor, pat_off):
    """The patterns' bounds as the HOST u32 array hmse_find_* read during the call."""
    off = [int(v) for v in pat_off]
    if len(off) < 1 or off[-1] > pat.numel() or any(v < 0 for v in off):
        raise HmseError(-1, "find: pat_off does not lie inside pat")
    return (C.c_uint32 * len(off))(*off), len(off) - 1


_BAD_TABLES = ((2, "inconsistent tables"),)
_BAD_TABLES_OR_AUTOMATON = _BAD_TABLES + ((4, "bad automaton"),)


def _hit_list(call, where: str, n_counts: int, hits_cap: int | None, dev, refuse=_BAD_TABLES):
    """The calling convention the scan and seams entry points of hmse_find_*, hmse_findset_* and hmse_regex_* share: `call(hits, cap,
    meta, counts)` enqueues one; meta = [n_hits, status]; `counts` has n_counts entries.  `refuse`: (status bit, message) pairs, the
    first one set raises.  hits_cap 0: count only; None: sized by a count-only call.  A list that ran out (status bit 0) is filled by
    ONE more call with hits_cap = n_hits (as l2_cdc repeats with the larger candidate list).
    -> (hits int64[n_hits], n_hits, counts int64[n_counts])."""
    cap = hits_cap
    for _ in range(3):
        hits = _buf(max(int(cap or 0), 1), torch.int64, dev)
        meta = _buf(2, torch.int64, dev, fill=0)      # [n_hits, status]
        counts = _buf(n_counts, torch.int64, dev, fill=0)
        _check(call(hits, int(cap or 0), meta, counts), where)
        n_hits, status = (int(v) for v in meta.tolist())
        status &= 0xFFFFFFFF
        for bit, what in refuse:
            if status & bit:
                raise HmseError(-1, f"{where}: {what} (device status {status:#x})")
        if cap is None or (status & 1):
            if cap is not None and cap >= n_hits:
                break
            cap = n_hits                              # exact: the second call cannot run out
            if cap == 0:
                return hits[:0], 0, counts
            continue
        return hits[:min(n_hits, int(cap))], n_hits, counts
    raise HmseError(-2, f"{where}: the hit list ran out twice ({n_hits} hits, {cap} entries)")


def _records_args(where: str, raw, raw_off, mult, more=()) -> int:
    """The "records" arguments of a scan: raw, raw_off and the optional mult.  -> n_rec."""
    for t, nm in ((raw, "raw"), (raw_off, "raw_off")) + more + (((mult, "mult"),) if mult is not None else ()):
        _require_gpu(t, nm)
    n_rec = raw_off.numel() - 1
    if n_rec < 0 or (mult is not None and mult.numel() != n_rec):
        raise HmseError(-1, f"{where}: raw_off / mult do not match")
    return n_rec


def _chunk_map_args(where: str, raw, raw_off, cuts, slot, more=()) -> int:
    """The "chunk map" arguments: raw, raw_off, cuts and slot (and what else the call takes on the device).  -> n_chunks."""
    for t, nm in ((raw, "raw"), (raw_off, "raw_off"), (cuts, "cuts"), (slot, "slot")) + more:
        _require_gpu(t, nm)
    n_chunks = slot.numel()
    if cuts.numel() != n_chunks + 1 or raw_off.numel() < 1:
        raise HmseError(-1, f"{where}: cuts / slot / raw_off do not match")
    return n_chunks


def find_scan(raw: torch.Tensor, raw_off: torch.Tensor, mult: torch.Tensor | None, pat: torch.Tensor, pat_off, ignore_case: bool = False,
              hits_cap: int | None = None, raw_bytes: int | None = None):
    """hmse_find_scan: every match of the patterns (`pat` uint8 on the device, `pat_off` host bounds) lying wholly inside one record
    [raw_off[r], raw_off[r + 1]) of `raw`.  -> (hits int64[n] = position in raw << 8 | pattern, any order; n_hits; counts int64[P] =
    per pattern the sum of mult[record] (int32, None: 1 each)).  hits_cap 0: count only (hits empty).  Replaces the read_store +
    host bytes.find loop."""
    n_rec = _records_args("find_scan", raw, raw_off, mult, ((pat, "pat"),))
    bounds, n_pat = _find_bounds(pat, pat_off)
    nb = raw.numel() if raw_bytes is None else int(raw_bytes)
    flags = FIND_IGNORE_CASE if ignore_case else 0
    lib = _lib.hip_lib()
    call = lambda hits, cap, meta, counts: lib.hmse_find_scan(_ptr(raw) if raw.numel() else None, nb, _ptr(raw_off), max(n_rec, 0), _ptr(mult),
                                                              _ptr(pat), bounds, n_pat, flags, _ptr(hits) if cap else None, cap,
                                                              meta.data_ptr(), _ptr(counts), meta.data_ptr() + 8, _stream())
    return _hit_list(call, "hmse_find_scan", n_pat, hits_cap, raw_off.device)


def find_seams(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, pat: torch.Tensor, pat_off,
               ignore_case: bool = False, hits_cap: int | None = None):
    """hmse_find_seams: the occurrences that start in a chunk and end behind it, read through the chunk map (`cuts` int64[n + 1],
    `slot` int64[n]: the record of every chunk).  -> (hits int64[n] = corpus offset << 8 | pattern, any order; n_hits; counts)."""
    n_chunks = _chunk_map_args("find_seams", raw, raw_off, cuts, slot, ((pat, "pat"),))
    bounds, n_pat = _find_bounds(pat, pat_off)
    flags = FIND_IGNORE_CASE if ignore_case else 0
    lib = _lib.hip_lib()
    keep = lambda t: _ptr(t) if t.numel() else None
    call = lambda hits, cap, meta, counts: lib.hmse_find_seams(keep(raw), raw.numel(), _ptr(raw_off), raw_off.numel() - 1, _ptr(cuts), keep(slot),
                                                               n_chunks, _ptr(pat), bounds, n_pat, flags, _ptr(hits) if cap else None, cap,
                                                               meta.data_ptr(), _ptr(counts), meta.data_ptr() + 8, _stream())
    return _hit_list(call, "hmse_find_seams", n_pat, hits_cap, cuts.device)


def _place(name: str, hits, raw_off, cuts, slot, chunk_out, n_out: int) -> torch.Tensor:
    """hmse_find_place and hmse_findset_place: one kernel template, two widths of the hit word's low field (csrc/chunkmap.h)."""
    for t, nm in ((hits, "hits"), (raw_off, "raw_off"), (cuts, "cuts"), (slot, "slot"), (chunk_out, "chunk_out")):
        _require_gpu(t, nm)
    n_chunks = slot.numel()
    if cuts.numel() != n_chunks + 1 or chunk_out.numel() != n_chunks + 1 or raw_off.numel() < 1:
        raise HmseError(-1, f"{name}: cuts / slot / chunk_out do not match")
    dev = cuts.device
    out = _buf(max(int(n_out), 1), torch.int64, dev)
    status = _buf(1, torch.int32, dev, fill=0)
    keep = lambda t: _ptr(t) if t.numel() else None
    rc = getattr(_lib.hip_lib(), "hmse_" + name)(keep(hits), hits.numel(), _ptr(raw_off), raw_off.numel() - 1, _ptr(cuts), keep(slot), n_chunks,
                                                 _ptr(chunk_out), _ptr(out) if n_out else None, int(n_out), _ptr(status), _stream())
    _check(rc, "hmse_" + name)
    st = int(status.item())
    if st:
        raise HmseError(-2 if st == 1 else -1, f"hmse_{name} device status {st:#x}"
                        + (": inconsistent tables" if st & 2 else ": chunk_out[-1] exceeds the output"))
    return out[:int(n_out)]


def find_place(hits: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, chunk_out: torch.Tensor, n_out: int) -> torch.Tensor:
    """hmse_find_place: the scan's hits, SORTED ascending, laid out at every chunk that maps to their record.  `chunk_out` int64
    [n_chunks + 1]: exclusive prefix sum of the number of hits of record slot[k]; n_out = chunk_out[-1].  -> int64[n_out] =
    corpus offset << 8 | pattern, ascending."""
    return _place("find_place", hits, raw_off, cuts, slot, chunk_out, n_out)


def _lines_tables(where: str, raw, raw_off, cuts, slot, more):
    _chunk_map_args(where, raw, raw_off, cuts, slot, more)
    for t, nm in ((raw_off, "raw_off"), (cuts, "cuts"), (slot, "slot")) + more:
        if t.dtype != torch.int64:
            raise HmseError(-1, f"{where}: {nm} must be torch.int64 (the bits of the u64 array)")
    if raw.dtype != torch.uint8:
        raise HmseError(-1, f"{where}: raw must be torch.uint8")


def lines_extent(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, pos: torch.Tensor, delim: int = 0x0A,
                 before: int = 0, after: int = 0, reach: int = 1 << 16):
    """hmse_lines_extent: for every corpus offset pos[i] the extent [start, end) of the line it lies in, with `before` lines in front
    and `after` behind, looking at most `reach` bytes each way (include/hmse.h has the definitions).  The tables are find_seams'.
    -> (start int64[n], end int64[n], flags uint8[n] = LINES_START_CUT | LINES_END_CUT, or LINES_BAD with start = end = 0 for a
    pos[i] >= cuts[-1]; status: bit 0 = some position was bad).  Inconsistent tables (status bit 1) raise HmseError."""
    _lines_tables("lines_extent", raw, raw_off, cuts, slot, ((pos, "pos"),))
    n, dev = pos.numel(), cuts.device
    start, end, flags = _buf(n, torch.int64, dev), _buf(n, torch.int64, dev), _buf(n, torch.uint8, dev)
    status = _buf(1, torch.int32, dev, fill=0)
    keep = lambda t: _ptr(t) if t.numel() else None
    rc = _lib.hip_lib().hmse_lines_extent(keep(raw), raw.numel(), _ptr(raw_off), raw_off.numel() - 1, _ptr(cuts), keep(slot), slot.numel(),
                                          keep(pos), n, int(delim), int(before), int(after), int(reach), keep(start), keep(end), keep(flags),
                                          _ptr(status), _stream())
    _check(rc, "hmse_lines_extent")
    st = int(status.item()) & 0xFFFFFFFF
    if st & 2:
        raise HmseError(-1, f"hmse_lines_extent device status {st:#x}: inconsistent tables")
    return start, end, flags, st


def lines_gather(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, start: torch.Tensor, end: torch.Tensor,
                 out_off: torch.Tensor, n_out: int) -> torch.Tensor:
    """hmse_lines_gather: the corpus bytes [start[i], end[i]) of every range back to back.  `out_off` int64[n + 1]: exclusive prefix sum
    of end - start; n_out = out_off[-1].  -> uint8[n_out].  HmseError for an out_off[-1] above n_out (status bit 0), for inconsistent
    tables, a range that descends or leaves the corpus, or an out_off that is not the prefix sum (bit 1); nothing was written then."""
    _lines_tables("lines_gather", raw, raw_off, cuts, slot, ((start, "start"), (end, "end"), (out_off, "out_off")))
    n, dev = start.numel(), cuts.device
    if end.numel() != n or out_off.numel() != n + 1:
        raise HmseError(-1, "lines_gather: start / end / out_off do not match")
    out = _buf(max(int(n_out), 1), torch.uint8, dev)
    status = _buf(1, torch.int32, dev, fill=0)
    keep = lambda t: _ptr(t) if t.numel() else None
    rc = _lib.hip_lib().hmse_lines_gather(keep(raw), raw.numel(), _ptr(raw_off), raw_off.numel() - 1, _ptr(cuts), keep(slot), slot.numel(),
                                          keep(start), keep(end), _ptr(out_off), n, _ptr(out) if n_out else None, int(n_out), _ptr(status),
                                          _stream())
    _check(rc, "hmse_lines_gather")
    st = int(status.item()) & 0xFFFFFFFF
    if st:
        raise HmseError(-1 if st & 2 else -2, f"hmse_lines_gather device status {st:#x}"
                        + (": inconsistent tables, a range that descends or leaves the corpus, or out_off is not the prefix sum of the lengths"
                           if st & 2 else ": out_off[-1] exceeds the output"))
    return out[:int(n_out)]


@dataclass
class FindSet:
    """The device arrays and the header of a compiled pattern set (include/hmse.h `hmse_findset`; built by find.PatternSet)."""
    upat: torch.Tensor           # uint8: the entries' bytes back to back
    uoff: torch.Tensor           # int32 [n + 1]
    ukey: torch.Tensor           # int32 [n]: the first four bytes of every entry (bit pattern of the u32)
    uid: torch.Tensor            # int32 [n]: the id reported for every entry
    dir: torch.Tensor            # int32 [2^dir_bits + 1]
    bitmap: torch.Tensor         # int32 [16384]
    n_ids: int
    dir_bits: int
    max_len: int
    ignore_case: bool

    def header(self) -> "_lib.HmseFindset":
        n = self.ukey.numel()
        keep = lambda t: _ptr(t) if t.numel() else None
        return _lib.HmseFindset(C.sizeof(_lib.HmseFindset), FIND_IGNORE_CASE if self.ignore_case else 0, n, int(self.n_ids), int(self.dir_bits),
                                int(self.max_len), self.upat.numel(), keep(self.upat), keep(self.uoff), keep(self.ukey), keep(self.uid),
                                keep(self.dir), keep(self.bitmap))


def _findset_args(fs: FindSet):
    for t, nm in ((fs.upat, "upat"), (fs.uoff, "uoff"), (fs.ukey, "ukey"), (fs.uid, "uid"), (fs.dir, "dir"), (fs.bitmap, "bitmap")):
        _require_gpu(t, nm)
    n = fs.ukey.numel()
    if n and (fs.uoff.numel() != n + 1 or fs.uid.numel() != n or fs.dir.numel() != (1 << int(fs.dir_bits)) + 1
              or fs.bitmap.numel() != 1 << (FINDSET_BITMAP_BITS - 5) or any(t.element_size() != 4 for t in (fs.uoff, fs.ukey, fs.uid, fs.dir, fs.bitmap))):
        raise HmseError(-1, "findset: the set's arrays do not match its header")
    return fs.header(), FIND_IGNORE_CASE if fs.ignore_case else 0


def findset_scan(raw: torch.Tensor, raw_off: torch.Tensor, mult: torch.Tensor | None, fs: FindSet, hits_cap: int | None = None,
                 raw_bytes: int | None = None):
    """hmse_findset_scan: every match of the set's patterns lying wholly inside one record of `raw` (find_scan's contract).
    -> (hits int64[n] = position in raw << 24 | id, any order; n_hits; counts int64[n_ids] weighted by mult)."""
    n_rec = _records_args("findset_scan", raw, raw_off, mult)
    hdr, flags = _findset_args(fs)
    nb = raw.numel() if raw_bytes is None else int(raw_bytes)
    lib = _lib.hip_lib()
    call = lambda hits, cap, meta, counts: lib.hmse_findset_scan(_ptr(raw) if raw.numel() else None, nb, _ptr(raw_off), max(n_rec, 0), _ptr(mult),
                                                                 C.byref(hdr), flags, _ptr(hits) if cap else None, cap, meta.data_ptr(),
                                                                 _ptr(counts) if fs.n_ids else None, meta.data_ptr() + 8, _stream())
    return _hit_list(call, "hmse_findset_scan", int(fs.n_ids), hits_cap, raw_off.device)


def findset_seams(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, fs: FindSet, hits_cap: int | None = None):
    """hmse_findset_seams: the set's occurrences that start in a chunk and end behind it (find_seams' contract).
    -> (hits int64[n] = corpus offset << 24 | id, any order; n_hits; counts int64[n_ids])."""
    n_chunks = _chunk_map_args("findset_seams", raw, raw_off, cuts, slot)
    hdr, flags = _findset_args(fs)
    lib = _lib.hip_lib()
    keep = lambda t: _ptr(t) if t.numel() else None
    call = lambda hits, cap, meta, counts: lib.hmse_findset_seams(keep(raw), raw.numel(), _ptr(raw_off), raw_off.numel() - 1, _ptr(cuts), keep(slot),
                                                                  n_chunks, C.byref(hdr), flags, _ptr(hits) if cap else None, cap, meta.data_ptr(),
                                                                  _ptr(counts) if fs.n_ids else None, meta.data_ptr() + 8, _stream())
    return _hit_list(call, "hmse_findset_seams", int(fs.n_ids), hits_cap, cuts.device)


def findset_place(hits: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, chunk_out: torch.Tensor, n_out: int) -> torch.Tensor:
    """hmse_findset_place: find_place for the hit word position << 24 | id.  -> int64[n_out] = corpus offset << 24 | id, ascending."""
    return _place("findset_place", hits, raw_off, cuts, slot, chunk_out, n_out)


REGEX_MAX_LEN, REGEX_MAX_TABLE, REGEX_ACCEPT = 256, 16384, 0x8000


@dataclass
class Regex:
    """The device arrays and the header of a compiled regular expression (include/hmse.h `hmse_regex`; built by regex.Regex)."""
    table: torch.Tensor          # int16 [n_states * n_classes]: the bits of the u16 entries
    classmap: torch.Tensor       # uint8 [256]
    n_states: int
    n_classes: int
    reach: int

    def header(self) -> "_lib.HmseRegex":
        return _lib.HmseRegex(C.sizeof(_lib.HmseRegex), int(self.n_states), int(self.n_classes), int(self.reach), _ptr(self.table), _ptr(self.classmap))


def _regex_args(rx: Regex):
    for t, nm in ((rx.table, "table"), (rx.classmap, "classmap")):
        _require_gpu(t, nm)
    if (rx.table.element_size() != 2 or rx.table.numel() != int(rx.n_states) * int(rx.n_classes) or rx.classmap.numel() != 256
            or rx.classmap.element_size() != 1):
        raise HmseError(-1, "regex: the automaton's arrays do not match its header")
    return rx.header()


def regex_scan(raw: torch.Tensor, raw_off: torch.Tensor, mult: torch.Tensor | None, rx: Regex, hits_cap: int | None = None,
               raw_bytes: int | None = None):
    """hmse_regex_scan: the occurrence of the regex at every SCAN start p of every record (raw_off[r + 1] - p >= reach).
    -> (hits int64[n] = position in raw << 8 | (length - 1), any order; n_hits; count int64[1] = the sum of mult[record] over the hits
    (int32, None: 1 each)).  hits_cap 0: count only; None: sized by a count-only call.  HmseError for inconsistent tables (device
    status bit 1) or a bad automaton (bit 2)."""
    n_rec = _records_args("regex_scan", raw, raw_off, mult)
    hdr = _regex_args(rx)
    nb = raw.numel() if raw_bytes is None else int(raw_bytes)
    lib = _lib.hip_lib()
    call = lambda hits, cap, meta, counts: lib.hmse_regex_scan(_ptr(raw) if raw.numel() else None, nb, _ptr(raw_off), max(n_rec, 0), _ptr(mult),
                                                               C.byref(hdr), _ptr(hits) if cap else None, cap, meta.data_ptr(), _ptr(counts),
                                                               meta.data_ptr() + 8, _stream())
    return _hit_list(call, "hmse_regex_scan", 1, hits_cap, raw_off.device, _BAD_TABLES_OR_AUTOMATON)


def regex_seams(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, rx: Regex, hits_cap: int | None = None):
    """hmse_regex_seams: the occurrence of the regex at every SEAM start o of every chunk (cuts[k + 1] - o < reach), walked through
    the chunk map.  -> (hits int64[n] = corpus offset << 8 | (length - 1), any order; n_hits; count int64[1] = n_hits)."""
    n_chunks = _chunk_map_args("regex_seams", raw, raw_off, cuts, slot)
    hdr = _regex_args(rx)
    lib = _lib.hip_lib()
    keep = lambda t: _ptr(t) if t.numel() else None
    call = lambda hits, cap, meta, counts: lib.hmse_regex_seams(keep(raw), raw.numel(), _ptr(raw_off), raw_off.numel() - 1, _ptr(cuts), keep(slot),
                                                                n_chunks, C.byref(hdr), _ptr(hits) if cap else None, cap, meta.data_ptr(),
                                                                _ptr(counts), meta.data_ptr() + 8, _stream())
    return _hit_list(call, "hmse_regex_seams", 1, hits_cap, cuts.device, _BAD_TABLES_OR_AUTOMATON)


APPROX_MAX_PATTERNS, APPROX_MAX_LEN, APPROX_MAX_K = 8, 64, 16


def _approx_bounds(pat: torch.Tensor, pat_off, k=None):
    """The patterns' bounds and error bounds as the HOST arrays hmse_approx_* read during the call."""
    bounds, n_pat = _find_bounds(pat, pat_off)
    if k is None:
        return bounds, None, n_pat
    ks = [int(v) for v in k]
    if len(ks) != n_pat or any(not 0 <= v <= 255 for v in ks):
        raise HmseError(-1, "approx: k is one value of 0..255 per pattern")
    return bounds, (C.c_uint8 * max(n_pat, 1))(*ks), n_pat


def approx_scan(raw: torch.Tensor, raw_off: torch.Tensor, mult: torch.Tensor | None, pat: torch.Tensor, pat_off, k, ignore_case: bool = False,
                hits_cap: int | None = None, raw_bytes: int | None = None):
    """hmse_approx_scan: every SCAN end of every record [raw_off[r], raw_off[r + 1]) of `raw` — a position p with some text ending at p
    within k[j] edits of pattern j and p + 1 - raw_off[r] >= m_j + k[j] (`pat` uint8 on the device, `pat_off` and `k` host values).
    -> (hits int64[n] = position of the match's last byte in raw << 8 | errors << 3 | pattern, any order; n_hits; counts int64[P] = per
    pattern the sum of mult[record] (int32, None: 1 each)).  hits_cap 0: count only; None: sized by a count-only call.  HmseError for
    inconsistent tables (device status bit 1).  Replaces the read_store + host dynamic-programme loop."""
    n_rec = _records_args("approx_scan", raw, raw_off, mult, ((pat, "pat"),))
    bounds, ks, n_pat = _approx_bounds(pat, pat_off, k)
    nb = raw.numel() if raw_bytes is None else int(raw_bytes)
    flags = FIND_IGNORE_CASE if ignore_case else 0
    lib = _lib.hip_lib()
    call = lambda hits, cap, meta, counts: lib.hmse_approx_scan(_ptr(raw) if raw.numel() else None, nb, _ptr(raw_off), max(n_rec, 0), _ptr(mult),
                                                                _ptr(pat), bounds, ks, n_pat, flags, _ptr(hits) if cap else None, cap,
                                                                meta.data_ptr(), _ptr(counts), meta.data_ptr() + 8, _stream())
    return _hit_list(call, "hmse_approx_scan", n_pat, hits_cap, raw_off.device)


def approx_seams(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, pat: torch.Tensor, pat_off, k,
                 ignore_case: bool = False, hits_cap: int | None = None):
    """hmse_approx_seams: every SEAM end of every chunk — the first m_j + k[j] - 1 ends of the chunk, walked through the chunk map from
    m_j + k[j] bytes in front.  -> (hits int64[n] = corpus offset of the match's last byte << 8 | errors << 3 | pattern, any order;
    n_hits; counts int64[P] = the seam hits per pattern)."""
    n_chunks = _chunk_map_args("approx_seams", raw, raw_off, cuts, slot, ((pat, "pat"),))
    bounds, ks, n_pat = _approx_bounds(pat, pat_off, k)
    flags = FIND_IGNORE_CASE if ignore_case else 0
    lib = _lib.hip_lib()
    keep = lambda t: _ptr(t) if t.numel() else None
    call = lambda hits, cap, meta, counts: lib.hmse_approx_seams(keep(raw), raw.numel(), _ptr(raw_off), raw_off.numel() - 1, _ptr(cuts), keep(slot),
                                                                 n_chunks, _ptr(pat), bounds, ks, n_pat, flags, _ptr(hits) if cap else None, cap,
                                                                 meta.data_ptr(), _ptr(counts), meta.data_ptr() + 8, _stream())
    return _hit_list(call, "hmse_approx_seams", n_pat, hits_cap, cuts.device)


def approx_spans(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, pat: torch.Tensor, pat_off,
                 ignore_case: bool, hits: torch.Tensor):
    """hmse_approx_spans: for every hit word (CORPUS offset of the last byte << 8 | errors << 3 | pattern; int64, any order) the start
    of its shortest best match.  -> (start int64[n], status: bit 0 = some hit lies outside the corpus, names no pattern or has errors
    that no text ending there attains; its start is offset + 1).  Inconsistent tables (status bit 1) raise HmseError."""
    _chunk_map_args("approx_spans", raw, raw_off, cuts, slot, ((pat, "pat"), (hits, "hits")))
    if hits.dtype != torch.int64:
        raise HmseError(-1, "approx_spans: hits must be torch.int64 (the bits of the u64 hit words)")
    bounds, _, n_pat = _approx_bounds(pat, pat_off)
    n, dev = hits.numel(), cuts.device
    start = _buf(max(n, 1), torch.int64, dev)
    status = _buf(1, torch.int32, dev, fill=0)
    keep = lambda t: _ptr(t) if t.numel() else None
    rc = _lib.hip_lib().hmse_approx_spans(keep(raw), raw.numel(), _ptr(raw_off), raw_off.numel() - 1, _ptr(cuts), keep(slot), slot.numel(),
                                          _ptr(pat), bounds, n_pat, FIND_IGNORE_CASE if ignore_case else 0, keep(hits), n,
                                          _ptr(start) if n else None, _ptr(status), _stream())
    _check(rc, "hmse_approx_spans")
    st = int(status.item()) & 0xFFFFFFFF
    if st & 2:
        raise HmseError(-1, f"hmse_approx_spans device status {st:#x}: inconsistent tables")
    return start[:n], st


def crc32(data: torch.Tensor, cuts: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """hmse_crc32: the zlib / gzip CRC-32 of every range data[cuts[k], cuts[k + 1]) (`cuts` int64[n + 1], ascending; ranges may be empty,
    start at any byte and have any length).  -> int32[n] (u32 bits; `out` if given).  Descending cuts or cuts[-1] > data.numel() are
    refused and `out` is left as it was."""
    _require_gpu(data, "data")
    _require_gpu(cuts, "cuts")
    n = cuts.numel() - 1
    if n < 0:
        raise HmseError(-1, "crc32: cuts is empty")
    dev = cuts.device
    if out is None:
        out = _buf(n, torch.int32, dev)
    _require_gpu(out, "out")
    if out.numel() != n or out.dtype != torch.int32:
        raise HmseError(-1, "crc32: out is not int32[n]")
    status = _buf(1, torch.int32, dev, fill=0)
    rc = _lib.hip_lib().hmse_crc32(_ptr(data) if data.numel() else None, data.numel(), _ptr(cuts), n, _ptr(out) if n else None, _ptr(status), _stream())
    _check(rc, "hmse_crc32")
    if n and int(status.item()):
        raise HmseError(-1, "hmse_crc32: cuts descends or ends behind the data")
    return out


def crc32_combine(crc: torch.Tensor, lens: torch.Tensor) -> int:
    """hmse_crc32_combine: the CRC-32 of the concatenation of ranges given only their CRCs (int32[n], u32 bits) and lengths (int64[n];
    exponents only: any values whose sum stays below 2^61).  -> the CRC as a Python int (0 for n == 0)."""
    _require_gpu(crc, "crc")
    _require_gpu(lens, "lens")
    n = crc.numel()
    if lens.numel() != n or crc.dtype != torch.int32 or lens.dtype != torch.int64:
        raise HmseError(-1, "crc32_combine: crc int32[n] / lens int64[n] do not match")
    meta = _buf(2, torch.int32, crc.device, fill=0)       # [out, status]
    rc = _lib.hip_lib().hmse_crc32_combine(_ptr(crc) if n else None, _ptr(lens) if n else None, n, meta.data_ptr(), meta.data_ptr() + 4, _stream())
    _check(rc, "hmse_crc32_combine")
    return int(meta[0].item()) & 0xFFFFFFFF


def gzip_members(src0: torch.Tensor, src1: torch.Tensor | None, src_off: torch.Tensor, stream_len: torch.Tensor, src_sel: torch.Tensor,
                 crc: torch.Tensor, raw_off: torch.Tensor, slot: torch.Tensor, member_off: torch.Tensor, bgzf: bool = False,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """hmse_gzip_members: one gzip (or BGZF) member per chunk at member_off (int64[n_chunks + 1], the caller's prefix sum of header +
    stream + 8): header, the stream of record slot[i] — stream_len[r] bytes at src_off[r] of (src1 if src_sel[r] else src0) —, crc[r]
    and the record's raw length raw_off[r + 1] - raw_off[r].  Returns the uint8 destination (`out`, or a new tensor of member_off[-1]
    bytes).  A member outside its source or destination, or a size that is not header + stream + 8, is refused: nothing is written."""
    srcs = [(src0, "src0")] + ([(src1, "src1")] if src1 is not None else [])
    for t, nm in srcs + [(src_off, "src_off"), (stream_len, "stream_len"), (src_sel, "src_sel"), (crc, "crc"), (raw_off, "raw_off"), (slot, "slot"),
                         (member_off, "member_off")]:
        _require_gpu(t, nm)
    n_rec, n_chunks = src_off.numel(), slot.numel()
    if stream_len.numel() != n_rec or src_sel.numel() != n_rec or crc.numel() != n_rec or raw_off.numel() != n_rec + 1 or member_off.numel() != n_chunks + 1:
        raise HmseError(-1, "gzip_members: the record tables / slot / member_off do not match")
    if crc.dtype != torch.int32 or src_sel.dtype != torch.uint8 or any(t.dtype != torch.int64 for t in (src_off, stream_len, raw_off, slot, member_off)):
        raise HmseError(-1, "gzip_members: crc int32, src_sel uint8, the other tables int64")
    dev = member_off.device
    if out is None:
        out = _buf(int(member_off[-1].item()), torch.uint8, dev)
    _require_gpu(out, "out")
    status = _buf(1, torch.int32, dev, fill=0)
    keep = lambda t: t if t is not None and t.numel() else None
    rc = _lib.hip_lib().hmse_gzip_members(_ptr(keep(src0)), src0.numel(), _ptr(keep(src1)), 0 if src1 is None else src1.numel(), _ptr(src_off),
                                          _ptr(stream_len), _ptr(src_sel), _ptr(crc), _ptr(raw_off), n_rec, _ptr(slot), n_chunks, _ptr(member_off),
                                          GZIP_BGZF if bgzf else 0, _ptr(out) if out.numel() else None, out.numel(), _ptr(status), _stream())
    _check(rc, "hmse_gzip_members")
    st = int(status.item()) if n_chunks else 0
    if st & 1:
        raise HmseError(-2, "hmse_gzip_members: a member lies outside its source or the destination, or its size is not header + stream + 8")
    if st & 2:
        raise HmseError(-2, "hmse_gzip_members: a BGZF member above 65536 bytes")
    return out
