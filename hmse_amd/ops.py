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


def _addr(t) -> int | None:
    """The address of a tensor that has elements; NULL for None and for an empty one."""
    return t.data_ptr() if t is not None and t.numel() else None


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


_DEVICE, _STRUCT, _SCALAR = _lib.DEVICE, _lib.STRUCT, _lib.SCALAR


def _call(name: str, *args) -> None:
    """Enqueue one entry point on torch's current stream: `args` in the order of include/hmse.h, without the stream.  _lib.SIGNATURES says
    what each one is.  For a device pointer: a tensor must live in HBM, be contiguous and have elements of the declared width, and gives its
    address (NULL when it is empty and the table says `?`); None is NULL; an int is a raw address.  An IngestConfig, a StreamArrays (whatever holds
    its struct as `.c`) or a mirror struct goes by reference; a host array as it is; a scalar as int().  A non-zero return raises HmseError (an _ex entry point
    under the name of the one it extends)."""
    params = (_lib.PARSED.get(name) or _lib.PARSED_REGEXA.get(name) or _lib.PARSED_TALLY.get(name) or _lib.PARSED_SUBST.get(name) or _lib.PARSED_ORDER[name])[1]
    if len(args) != len(params) - 1:
        raise TypeError(f"{name} takes {len(params) - 1} arguments and the stream, got {len(args)}")
    out = list(args)
    for i, a in enumerate(args):                    # (this loop is the host cost of every call: DESIGN.md §11.26)
        if type(a) is int or a is None:             # a scalar as it is, a raw address, NULL
            continue
        pname, kind, _, width, null_if_empty = params[i]
        if kind == _DEVICE:
            _require_gpu(a, pname)
            if width and a.element_size() != width:
                raise HmseError(-1, f"{name}: {pname} must have {width}-byte elements")
            out[i] = None if null_if_empty and not a.numel() else a.data_ptr()
        elif kind == _STRUCT:
            out[i] = C.byref(a.to_c() if isinstance(a, IngestConfig) else getattr(a, "c", a))     # (.c: a StreamArrays' struct; no mirror has such a field)
        elif kind == _SCALAR:
            out[i] = int(a)
    rc = getattr(_lib.hip_lib(), name)(*out, _stream())
    if rc:
        _check(rc, name.removesuffix("_ex"))


def _host(name: str, *ints, cfg: IngestConfig | None = None) -> int:
    """A host-side entry point (sizes, bounds, validation): ints, then the configuration by reference where it takes one."""
    fn = getattr(_lib.hip_lib(), name)
    return int(fn(*ints) if cfg is None else fn(*ints, C.byref(cfg.to_c())))


def _status_word(device) -> torch.Tensor:
    return _buf(1, torch.int32, device, fill=0)


_ANY = 0xFFFFFFFF


def _refuse(status, rules, where: str = "") -> int:
    """Read a status word (a tensor: one host sync; an int as it is) and raise for the first of `rules` = (bits, code, text with {st} and
    {where}) that has a bit set.  -> the status."""
    st = (status if type(status) is int else int(status.item())) & _ANY
    for bits, code, text in rules:
        if st & bits:
            raise HmseError(code, text.format(st=st, where=where))
    return st


def workspace_bytes(stage: int, n: int, cfg: IngestConfig) -> int:
    return _host("hmse_workspace_bytes", stage, n, cfg=cfg)


def segment_offsets(n: int, seg_size: int, device) -> torch.Tensor:
    k = max(1, -(-n // seg_size))
    off = torch.arange(k + 1, dtype=torch.int64, device=device) * seg_size
    return torch.clamp(off, max=n)


def l2_cdc(data: torch.Tensor, cfg: IngestConfig, seg_off: torch.Tensor | None = None) -> torch.Tensor:
    """FastCDC cut points. Returns int64 cuts[n_chunks+1] (cuts[0] == 0). README.md:2456-2490."""
    n = data.numel()
    dev = data.device
    if seg_off is None:
        seg_off = segment_offsets(n, cfg.seg_size, dev)
    n_seg = seg_off.numel() - 1
    cap = n // cfg.min_size + n_seg + 2
    cuts = _buf(cap, torch.int64, dev)
    meta = _buf(2, torch.int64, dev, fill=0)  # [n_cuts, status]
    # exact workspace for this segmentation: the generic sizing assumes ceil(n/seg_size) segments
    ws_bytes = workspace_bytes(STAGE_L2, n, cfg) + 24 * max(0, n_seg - n // cfg.seg_size) + 4096
    # The provisioned candidate list holds 8x the expected density.  Bytes that are denser still (status bit 0) are legitimate
    # input: run once more with a list of one entry per byte, which nothing can overflow (include/hmse.h).
    for extra in (0, 4 * n + 256):
        ws = _ws(ws_bytes + extra, dev)
        _call("hmse_l2_cdc", data, n, seg_off, n_seg, cfg, cuts, cap, meta.data_ptr(), meta.data_ptr() + 8, ws, ws.numel())
        n_cuts, status = (int(v) for v in meta.tolist())
        if not (status & 1):
            break
        del ws
    _refuse(status, ((_ANY, -2, "hmse_l2_cdc device status {st:#x}"),))
    return cuts[: n_cuts + 1]


def l3_sha256(data: torch.Tensor, cuts: torch.Tensor) -> torch.Tensor:
    """SHA-256 of every chunk -> uint8 [n_chunks, 32]. README.md:2543."""
    _require_gpu(data, "data")
    n_chunks = cuts.numel() - 1
    out = _buf((max(n_chunks, 0), 32), torch.uint8, data.device)
    if n_chunks <= 0:
        return out
    ws = _ws(workspace_bytes(STAGE_SHA, n_chunks, IngestConfig()), data.device)
    _call("hmse_l3_sha256", data, data.numel(), cuts, n_chunks, out, ws, ws.numel())
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
    ws = _ws(workspace_bytes(STAGE_DEDUP, n, IngestConfig()), dev)
    _call("hmse_l3_dedup", digests, n, fo, rc_t, ws, ws.numel())
    return fo, rc_t


def l3_index_slots(capacity_chunks: int) -> int:
    return _host("hmse_l3_index_slots", int(capacity_chunks))


def l3_index_update(digests_all: torch.Tensor, n_old: int, n_new: int, first_occ: torch.Tensor, refcount: torch.Tensor,
                    table: torch.Tensor) -> None:
    """Persistent L3 index: digests [n_old, n_old + n_new) join `table` (int32[l3_index_slots(capacity)], kept by the
    caller across calls); first_occ / refcount tails are written in place.  README.md:1288-1292."""
    if digests_all.shape[0] < n_old + n_new or first_occ.numel() < n_old + n_new or refcount.numel() < n_old + n_new:
        raise HmseError(-1, "l3_index_update: arrays shorter than n_old + n_new")
    _call("hmse_l3_index_update", digests_all, n_old, n_new, first_occ, refcount, table, table.numel())


def l4_lsh_slots(capacity_chunks: int) -> int:
    return _host("hmse_l4_lsh_slots", int(capacity_chunks))


def l4_lsh_update(sig_all: torch.Tensor, n_old: int, n_new: int, cfg: IngestConfig, band_keys: torch.Tensor, base: torch.Tensor | None,
                  tables: torch.Tensor, keys_given: bool = False) -> None:
    """Persistent L4b band tables: signatures [n_old, n_old + n_new) join `tables` (int32[bands, l4_lsh_slots(capacity)]);
    band_keys / base tails are written in place.  README.md:1554-1576, 1937-1945."""
    if sig_all.shape[0] < n_old + n_new or band_keys.shape[0] < n_old + n_new or (base is not None and base.numel() < n_old + n_new):
        raise HmseError(-1, "l4_lsh_update: arrays shorter than n_old + n_new")
    _call("hmse_l4_lsh_update", sig_all, n_old, n_new, cfg, band_keys, base, tables, tables.shape[1], keys_given)


def l4_minhash(data: torch.Tensor, cuts: torch.Tensor, cfg: IngestConfig, chunk_ids: torch.Tensor | None = None,
               memo: bool = True) -> torch.Tensor:
    """MinHash signatures -> int32 [n_sel, 128] (uint32 bits). README.md:2578-2598.
    memo=False hands the C-ABI a workspace too small for its memo table (include/hmse.h): every hash is then computed."""
    _require_gpu(data, "data")
    n_sel = (cuts.numel() - 1) if chunk_ids is None else chunk_ids.numel()
    sig = _buf((max(n_sel, 0), cfg.n_hashes), torch.int32, data.device)
    if n_sel <= 0:
        return sig
    ws = _ws(workspace_bytes(STAGE_MINHASH, n_sel, cfg) if memo else 256, data.device)
    _call("hmse_l4_minhash", data, data.numel(), cuts, chunk_ids, n_sel, cfg, sig, ws, ws.numel())
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
    ws = _ws(workspace_bytes(STAGE_LSH, n, cfg), dev)
    _call("hmse_l4_lsh", sig, n, cfg, keys, base, ws, ws.numel())
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
    _require_gpu(data, "data")
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
    status = _status_word(dev)
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
        nb = workspace_bytes(STAGE_DEFLATE, n_p, cfg)
        if ws is None or ws.numel() < nb + need_p + 4096:   # (`ws`: a caller-held workspace, e.g. the streaming front end's, reused when big enough)
            ws = None
            ws = _ws(nb + need_p + 4096, dev)
        ids_p = None if ids_all is None else ids_all[a:e]
        base_p = None if base_all is None else base_all[a:e]
        off_p = out_off[a: e + 1] if len(pieces) == 1 else _buf(n_p + 1, torch.int64, dev, fill=0)
        _call("hmse_l1_deflate_ex", data, data.numel(), cuts, ids_p, base_p, n_p, cfg, by_id, out.data_ptr() + total, cap - total, off_p, kind[a:e],
              status, ws, ws.numel())
        st, tot_p = (int(v) for v in torch.stack([status[0].to(torch.int64), off_p[-1]]).tolist())
        _refuse(st, ((_ANY, -2, "hmse_l1_deflate device status {st:#x}"),))
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
    dev = streams.device
    n_sel = kind.numel()
    if stream_off.numel() != (n_sel if stream_len is not None else n_sel + 1) or raw_len.numel() != n_sel:
        raise HmseError(-1, "l1_inflate: stream_off / raw_len do not match kind")
    raw_off = _buf(n_sel + 1, torch.int64, dev)
    raw_off[:1] = 0        # (an input of the call, built here: exclusive sums of raw_len)
    torch.cumsum(raw_len, 0, out=raw_off[1:])
    total = int(raw_off[-1].item()) if n_sel else 0
    raw = _buf(total, torch.uint8, dev)
    status = _status_word(dev)
    ok = _buf(n_sel, torch.uint8, dev, fill=0)
    if n_sel == 0:
        return raw, raw_off, ok
    ws = _ws(workspace_bytes(STAGE_INFLATE, n_sel, IngestConfig()), dev)
    keep = _buf(1, torch.uint8, dev) if total == 0 else raw  # a valid pointer even when every chunk is empty
    _call("hmse_l1_inflate", streams, streams.numel(), stream_off, stream_len, kind, base, n_sel, raw_off, keep, total, ok, status, ws, ws.numel())
    st = int(status.item())
    if check and st:
        raise HmseError(-1, f"hmse_l1_inflate: {int((ok == 0).sum().item())} corrupt record(s), device status {st:#x}")
    return raw, raw_off, ok


def read_assemble(cuts: torch.Tensor, slot_of_chunk: torch.Tensor, raw_off: torch.Tensor, raw: torch.Tensor) -> torch.Tensor:
    """Lay the stored chunks out as the original data: chunk i <- raw bytes of slot_of_chunk[i]. README.md:1635-1669."""
    _require_gpu(cuts, "cuts")
    n_chunks = cuts.numel() - 1
    n = int(cuts[-1].item()) if n_chunks > 0 else 0
    out = _buf(n, torch.uint8, cuts.device)
    status = _status_word(cuts.device)
    if n_chunks <= 0 or n == 0:
        return out
    _call("hmse_read_assemble", cuts, n_chunks, slot_of_chunk, raw_off.numel() - 1, raw_off, raw, out, n, status)
    _refuse(status, ((_ANY, -1, "hmse_read_assemble: chunk map disagrees with the stored lengths"),))
    return out


def manifest_pack(res, shard: int, n_shards: int, shard_bases, rec_off: torch.Tensor, lba_unit: int, ptr_index: torch.Tensor,
                  blob: torch.Tensor, index: torch.Tensor, chunk_map: torch.Tensor, pointers: torch.Tensor, any_target: bool = False) -> None:
    """hmse_manifest_pack over a ShardResult: blob, ChunkIndex table, chunk map and pointer records written in place.
    README.md:1263-1270, 2182-2189, 1312, 1448."""
    dev = res.cuts.device
    n = res.cuts.numel() - 1
    status = _status_word(dev)
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
    _call("hmse_manifest_pack_ex", res.streams, res.stream_off, res.kind, base, res.uniq_ids, res.uniq_ids.numel(), res.digests, res.refcount,
          res.cuts, n, res.first_occ, res.chunk_base, shard, sb, n_shards, any_target, rec_off, lba_unit, ptr_index, keep, blob.numel(), index,
          chunk_map, pointers, pointers.shape[0], status, ws, ws.numel())
    _refuse(status, ((_ANY, -2, "hmse_manifest_pack device status {st:#x}"),))


def gc_plan(cuts: torch.Tensor, slot: torch.Tensor, n_slots: int, seg_off: torch.Tensor, drop: torch.Tensor, digests_old: torch.Tensor) -> dict:
    """hmse_gc_plan: the old chunk map (`cuts` int64[n+1], `slot` int32[n]) and the dropped segments (`seg_off` int64[n_seg+1], `drop`
    uint8[n_seg]) -> the L3 arrays of the surviving store as a fresh ingest of the remainder numbers them.  `digests_old` uint8[n_slots, 32].
    Returns {old_chunk, first_occ, refcount, digests, uniq_ids, old_slot (int64[u_new]), new_slot_of_old (int64[n_slots], -1 gone)}.
    README.md:1268, 1886 (the refcount kept for garbage collection)."""
    dev = cuts.device
    n = cuts.numel() - 1
    n_seg = seg_off.numel() - 1
    if slot.numel() != n or drop.numel() != n_seg or digests_old.shape != (n_slots, 32) or n_seg < 1:
        raise HmseError(-1, "gc_plan: slot / drop / digests_old do not match cuts / seg_off / n_slots")
    counts = _buf(2, torch.int64, dev, fill=0)
    status = _status_word(dev)
    e = lambda *shape, dt=torch.int64: _buf(shape, dt, dev)
    old_chunk, first_occ, refcount, digests = e(max(n, 1)), e(max(n, 1)), e(max(n, 1), dt=torch.int32), e(max(n, 1), 32, dt=torch.uint8)
    uniq_ids, old_slot, new_slot_of_old = e(max(n_slots, 1)), e(max(n_slots, 1)), e(max(n_slots, 1))
    ws = _ws(workspace_bytes(STAGE_GC_PLAN, n, IngestConfig()), dev)
    _call("hmse_gc_plan", cuts, n, slot, n_slots, seg_off, n_seg, drop, digests_old, counts, old_chunk, first_occ, refcount, digests, uniq_ids,
          old_slot, new_slot_of_old, status, ws, ws.numel())
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
    dev = dst_off.device
    n = src_sel.numel()
    if src_off.numel() != n or dst_off.numel() != n + 1:
        raise HmseError(-1, "record_gather: src_off / src_sel / dst_off do not match")
    if out is None:
        out = _buf(int(dst_off[-1].item()), torch.uint8, dev)
    status = _status_word(dev)
    _call("hmse_record_gather", src0, src0.numel(), src1, 0 if src1 is None else src1.numel(), src_off, src_sel, dst_off, n, out, out.numel(), status)
    if n:
        _refuse(status, ((_ANY, -2, "hmse_record_gather: a record lies outside its source or the destination"),))
    return out


def sync_match(a: torch.Tensor, a_off: torch.Tensor, a_len: torch.Tensor, b: torch.Tensor, b_off: torch.Tensor, b_len: torch.Tensor,
               cand: torch.Tensor):
    """hmse_sync_match: same[k] = 1 iff record k of a — bytes [a_off[k], + a_len[k]) — and record cand[k] of b are byte-identical
    (cand < 0: no candidate, 0).  a, b uint8; a_off, b_off int64; a_len, b_len int32; cand int64.  Returns (same uint8[n], status):
    status bit 0 = a candidate >= len(b_off) or a record that reaches outside its blob (same is 0 there; nothing outside is read)."""
    for dt, given in ((torch.uint8, dict(a=a, b=b)), (torch.int64, dict(a_off=a_off, b_off=b_off)), (torch.int32, dict(a_len=a_len, b_len=b_len)),
                      (torch.int64, dict(cand=cand))):
        for nm, t in given.items():
            if t.dtype != dt:
                raise HmseError(-1, f"sync_match: {nm} must be {dt}")
    n, n_b = cand.numel(), b_off.numel()
    if a_off.numel() != n or a_len.numel() != n or b_len.numel() != n_b:
        raise HmseError(-1, "sync_match: a_off / a_len / cand or b_off / b_len do not match")
    same = _buf(n, torch.uint8, cand.device)
    status = _status_word(cand.device)
    _call("hmse_sync_match", a, a.numel(), a_off, a_len, n, b, b.numel(), b_off, b_len, n_b, cand, same, status)
    return same, int(status.item())


def stream_batch_workspace_bytes(batch_bytes: int, cfg: IngestConfig) -> int:
    return _host("hmse_stream_batch_workspace_bytes", int(batch_bytes), cfg=cfg)


def stream_workspace(batch_bytes: int, cfg: IngestConfig, device) -> torch.Tensor:
    """A workspace for hmse_stream_batch / hmse_stream_piece_*: allocated and prepared once (hmse_stream_workspace_init: the MinHash
    memo table inside persists across the stream's batches), then passed to every batch."""
    ws = _ws(stream_batch_workspace_bytes(batch_bytes, cfg), device)
    _call("hmse_stream_workspace_init", ws, ws.numel(), batch_bytes, cfg)
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


def stream_batch(data: torch.Tensor, batch_bytes: int, seg_off: torch.Tensor, cfg: IngestConfig, s: StreamArrays, ws: torch.Tensor,
                 data_origin: int = 0) -> None:
    """hmse_stream_batch: the whole per-batch chain (L2 -> L3 -> index -> L4 -> band tables -> L1) enqueued without a host
    read; capturable into a hipGraph (hmse_amd/stream.py).  README.md:1519-1580."""
    # data_origin: `data` holds the stream's bytes [data_origin, data_origin + data.numel()) — the resident WINDOW of a stream longer than
    # the buffer (stream.StreamIngest(window_bytes=)); the chain addresses bytes by stream offset, so it gets the buffer's address minus the origin
    _require_gpu(data, "data")
    _call("hmse_stream_batch", data.data_ptr() - int(data_origin), int(data_origin) + data.numel(), batch_bytes, seg_off, seg_off.numel() - 1, cfg, s,
          ws, ws.numel())


def stream_row_bytes(cap_bytes: int, cfg: IngestConfig) -> int:
    return _host("hmse_stream_row_bytes", int(cap_bytes), cfg=cfg)


def stream_piece_hash(data: torch.Tensor, piece_bytes: int, cap_bytes: int, seg_off: torch.Tensor | None, cfg: IngestConfig, s: StreamArrays,
                      row: torch.Tensor, ws: torch.Tensor) -> None:
    """hmse_stream_piece_hash: phase A of a multi-rank stream's batch (L2 + L3 hash of this rank's piece -> its exchange row).
    README.md:1519-1540."""
    _call("hmse_stream_piece_hash", data, data.numel(), piece_bytes, cap_bytes, seg_off, 0 if seg_off is None else seg_off.numel() - 1, cfg, s, row,
          ws, ws.numel())


def stream_piece_encode(data: torch.Tensor, piece_bytes: int, cap_bytes: int, cfg: IngestConfig, s: StreamArrays, rows: torch.Tensor,
                        ws: torch.Tensor) -> None:
    """hmse_stream_piece_encode: phase B (gathered rows -> global index -> this rank's stored chunks -> L4 -> L1).  README.md:1538-1580."""
    if rows.numel() != s.c.world * stream_row_bytes(cap_bytes, cfg):
        raise HmseError(-1, "stream_piece_encode: rows must hold one exchange row per rank")
    _call("hmse_stream_piece_encode", data, data.numel(), piece_bytes, cap_bytes, cfg, s, rows, ws, ws.numel())


# ---- global L4 of a multi-rank stream as captured phases (include/hmse.h: hmse_gl4) ---------------------------------------------
def stream_sig_cap(cap_bytes: int, cfg: IngestConfig) -> int:
    return _host("hmse_stream_sig_cap", int(cap_bytes), cfg=cfg)


def stream_sig_row_bytes(cap_bytes: int, cfg: IngestConfig) -> int:
    return _host("hmse_stream_sig_row_bytes", int(cap_bytes), cfg=cfg)


def stream_piece_sign(data, piece_bytes, cap_bytes, cfg, s: StreamArrays, rows, sig_row, ws) -> None:
    """hmse_stream_piece_sign: gathered digest rows -> global index -> this rank's new stored chunks -> MinHash -> its signature row."""
    _call("hmse_stream_piece_sign", data, data.numel(), piece_bytes, cap_bytes, cfg, s, rows, sig_row, ws, ws.numel())


def stream_piece_bases(cap_bytes, cfg, s: StreamArrays, sig_rows, gl4, ws) -> None:
    """hmse_stream_piece_bases: gathered signature rows -> global band tables -> dictionaries of this rank's new stored chunks + requests.
    `gl4`: a _lib.HmseGl4 (kept alive by the caller together with the tensors it points to)."""
    _call("hmse_stream_piece_bases", cap_bytes, cfg, s, sig_rows, gl4, ws, ws.numel())


def stream_piece_encode_g(data, piece_bytes, cap_bytes, cfg, s: StreamArrays, gstate, ws) -> None:
    """hmse_stream_piece_encode_g: DEFLATE of the new stored chunks with the dictionaries resolved by stream_piece_bases, tails, states advanced."""
    _call("hmse_stream_piece_encode_g", data, data.numel(), piece_bytes, cap_bytes, cfg, s, gstate, ws, ws.numel())


def band_tables_write(keys: torch.Tensor, sig: torch.Tensor | None, band_bits: int) -> torch.Tensor:
    """hmse_band_tables_write: the band-table sidecar of `keys` (int32 [n, bands], uint32 bits) and, when given, the signatures
    (int32 [n, n_hashes]) -> a device uint8 tensor, byte for byte bandtable.write_band_tables().  One host sync (the size)."""
    if keys.dim() != 2 or keys.dtype != torch.int32:
        raise HmseError(-1, "band_tables_write: keys must be int32 [n, bands]")
    n, bands = keys.shape
    nh = 0
    if sig is not None:
        if sig.dim() != 2 or sig.dtype != torch.int32 or sig.shape[0] != n:
            raise HmseError(-1, "band_tables_write: sig must be int32 [n, n_hashes]")
        nh = int(sig.shape[1])
    if n >= 1 << 24:
        raise ValueError("3-byte chunk ids hold at most 16 777 215 stored chunks (README.md:1943)")
    if not 1 <= band_bits <= 16:
        raise ValueError("band_hash is a u16")
    dev = keys.device
    cap = _host("hmse_band_tables_bound", n, bands, band_bits, nh)
    out = _buf(cap, torch.uint8, dev)
    meta = _buf(2, torch.int64, dev, fill=0)      # [out_bytes, status]
    ws = _ws(_host("hmse_band_tables_workspace_bytes", n), dev)
    _call("hmse_band_tables_write", keys, n, bands, band_bits, sig, nh, out, cap, meta.data_ptr(), meta.data_ptr() + 8, ws, ws.numel())
    size, st = (int(v) for v in meta.tolist())
    _refuse(st, ((_ANY, -2, "hmse_band_tables_write device status {st:#x}"),))
    if size > cap:
        raise HmseError(-2, f"hmse_band_tables_write: {size} bytes written into {cap}")
    return out[:size]


def search_cfg(cfg: IngestConfig, bands: int) -> IngestConfig:
    """`cfg` with the search banding bands x (128 / bands); ValueError unless hmse_cfg_validate accepts it (bands in 1, 2, 4, 8, 16)."""
    if int(bands) not in (1, 2, 4, 8, 16) or cfg.n_hashes != 128:
        raise ValueError(f"a search banding is bands x rows = 128 with bands in (1, 2, 4, 8, 16), got bands={bands} (n_hashes {cfg.n_hashes})")
    sc = cfg.with_(bands=int(bands), rows=128 // int(bands))
    if _host("hmse_cfg_validate", cfg=sc) != 0:
        raise ValueError(f"configuration {sc} is not supported by the device path")
    return sc


def l4_index_build(keys: torch.Tensor):
    """hmse_l4_index_build: band keys int32 [n, bands] (uint32 bits) -> (sorted_keys, sorted_ids), int32 [bands, n] each: per band the
    ids sorted stably by their key in uint32 order."""
    if keys.dim() != 2 or keys.dtype != torch.int32:
        raise HmseError(-1, "l4_index_build: keys must be int32 [n, bands]")
    n, bands = keys.shape
    dev = keys.device
    sk = _buf((bands, n), torch.int32, dev)
    si = _buf((bands, n), torch.int32, dev)
    status = _status_word(dev)
    ws = _ws(workspace_bytes(STAGE_L4_INDEX, n, search_cfg(IngestConfig(), bands)) if bands in (1, 2, 4, 8, 16) else 256, dev)
    _call("hmse_l4_index_build", keys, n, bands, sk, si, status, ws, ws.numel())
    return sk, si


def l4_query(sig_q: torch.Tensor, keys_q: torch.Tensor, sig_s: torch.Tensor, sorted_keys: torch.Tensor, sorted_ids: torch.Tensor,
             cfg: IngestConfig, top_k: int = 8, min_score: int = 0, exclude_self: bool = False):
    """hmse_l4_query under the banding of `cfg` -> (ids int64 [q, top_k] (-1 padding), scores int32 [q, top_k] (0 padding),
    n_hits int32 [q], n_candidates int64 [q]).  One host sync (the status word)."""
    n_q, n_s = sig_q.shape[0], sig_s.shape[0]
    if sig_q.shape[1:] != (128,) or sig_s.shape[1:] != (128,) or keys_q.shape != (n_q, cfg.bands) or \
            sorted_keys.shape != (cfg.bands, n_s) or sorted_ids.shape != (cfg.bands, n_s):
        raise HmseError(-1, "l4_query: shapes of the signatures, keys and index do not agree with each other or with the banding")
    dev = sig_q.device
    ids = _buf((n_q, int(top_k)), torch.int64, dev)
    scores = _buf((n_q, int(top_k)), torch.int32, dev)
    n_hits = _buf(n_q, torch.int32, dev)
    n_cand = _buf(n_q, torch.int64, dev)
    status = _status_word(dev)
    ws = _ws(workspace_bytes(STAGE_L4_QUERY, n_q, cfg), dev)
    _call("hmse_l4_query", sig_q, keys_q, n_q, sig_s, n_s, sorted_keys, sorted_ids, cfg, top_k, min_score, QUERY_EXCLUDE_SELF if exclude_self else 0,
          ids, scores, n_hits, n_cand, status, ws, ws.numel())
    _refuse(status, ((_ANY, -1, "hmse_l4_query device status {st:#x}: an index entry names an id outside the stored signatures"),))
    return ids, scores, n_hits, n_cand


def scrub_records(blob: torch.Tensor, rec_shard: torch.Tensor, shard_blob: torch.Tensor, shard_slot: torch.Tensor, lba_unit: torch.Tensor,
                  lba: torch.Tensor, rec_len: torch.Tensor, kind: torch.Tensor, remote: torch.Tensor, sorted_lba: torch.Tensor,
                  sorted_slot: torch.Tensor, steps: int, meta: torch.Tensor):
    """hmse_scrub_records: per record (global slot) its STRUCTURE / HEADER flags and resolved dictionary, plus the non-zero padding
    bytes of the blobs.  u32 arrays travel as int32.  Returns (status uint8[n], dict int64[n], padding int64[1]) on the device."""
    _require_gpu(blob, "blob")
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
    _call("hmse_scrub_records", blob, blob.numel(), n, n_shards, rec_shard, shard_blob, shard_slot, lba_unit, lba, rec_len, kind, remote, sorted_lba,
          sorted_slot, steps, meta, status, dict_, pad)
    return status[:n], dict_[:n], pad


def scrub_attribute(status: torch.Tensor, dict_: torch.Tensor, ok: torch.Tensor, got: torch.Tensor, want: torch.Tensor, check_digest: bool,
                    chunk_slot: torch.Tensor, cuts: torch.Tensor, max_depth_log2: int) -> dict:
    """hmse_scrub_attribute: final record flags and roots, chunk roots, per-root losses and the damaged ranges.  Returns device
    tensors {status, root, chunk_root, root_records, root_chunks, root_bytes, ranges (u64[2 (n_chunks / 2 + 1)]), counts (u64[8])}."""
    dev = cuts.device
    n, nc = status.numel(), chunk_slot.numel()
    if dict_.numel() != n or ok.numel() != n or cuts.numel() != nc + 1 or (check_digest and (got.shape != (n, 32) or want.shape != (n, 32))):
        raise HmseError(-1, "scrub_attribute: per-record / per-chunk arrays do not match")
    e = lambda k, dt=torch.int64: _buf(max(k, 1), dt, dev, fill=0)
    out = {"status": e(n, torch.uint8), "root": e(n), "chunk_root": e(nc), "root_records": e(n), "root_chunks": e(n), "root_bytes": e(n),
           "ranges": e(2 * (nc // 2 + 1)), "counts": e(8)}
    ws = _ws(workspace_bytes(STAGE_SCRUB_ATTRIBUTE, max(n, nc), IngestConfig()), dev)
    _call("hmse_scrub_attribute", n, status, dict_, ok, got if check_digest else None, want if check_digest else None, check_digest, max_depth_log2,
          nc, chunk_slot, cuts, *out.values(), ws, ws.numel())
    return out


def _find_bounds(pat: torch.Tensor, pat_off):
    """The patterns' bounds as the HOST u32 array hmse_find_* read during the call."""
    off = [int(v) for v in pat_off]
    if len(off) < 1 or off[-1] > pat.numel() or any(v < 0 for v in off):
        raise HmseError(-1, "find: pat_off does not lie inside pat")
    return (C.c_uint32 * len(off))(*off), len(off) - 1


_BAD_TABLES = ((2, -1, "{where}: inconsistent tables (device status {st:#x})"),)
_BAD_TABLES_OR_AUTOMATON = _BAD_TABLES + ((4, -1, "{where}: bad automaton (device status {st:#x})"),)


def _hit_list(call, where: str, n_counts: int, hits_cap: int | None, dev, refuse=_BAD_TABLES):
    """The calling convention the scan and seams entry points of hmse_find_*, hmse_findset_*, hmse_regex_* and hmse_approx_* share:
    `call(hits, cap, meta, counts)` enqueues one; meta = [n_hits, status]; `counts` has n_counts entries.  `refuse`: rules of _refuse,
    the first one set raises.  hits_cap 0: count only; None: sized by a count-only call.  A list that ran out (status
    bit 0) is filled by ONE more call with hits_cap = n_hits (as l2_cdc repeats with the larger candidate list).
    -> (hits int64[n_hits], n_hits, counts int64[n_counts])."""
    cap = hits_cap
    for _ in range(3):
        hits = _buf(max(int(cap or 0), 1), torch.int64, dev)
        meta = _buf(2, torch.int64, dev, fill=0)      # [n_hits, status]
        counts = _buf(n_counts, torch.int64, dev, fill=0)
        call(hits, int(cap or 0), meta, counts)
        n_hits, status = (int(v) for v in meta.tolist())
        status = _refuse(status, refuse, where)
        if cap is None or (status & 1):
            if cap is not None and cap >= n_hits:
                break
            cap = n_hits                              # exact: the second call cannot run out
            if cap == 0:
                return hits[:0], 0, counts
            continue
        return hits[:min(n_hits, int(cap))], n_hits, counts
    raise HmseError(-2, f"{where}: the hit list ran out twice ({n_hits} hits, {cap} entries)")


def _scan(name: str, raw, raw_off, mult, raw_bytes, hits_cap, n_counts: int, *middle, refuse=_BAD_TABLES):
    """A scan entry point hmse_<name>: the records (raw, raw_off and the optional mult), the family's own `middle` arguments, the hit list."""
    n_rec = raw_off.numel() - 1
    if n_rec < 0 or (mult is not None and mult.numel() != n_rec):
        raise HmseError(-1, f"{name}: raw_off / mult do not match")
    nb = raw.numel() if raw_bytes is None else raw_bytes
    call = lambda hits, cap, meta, counts: _call("hmse_" + name, raw, nb, raw_off, n_rec, mult, *middle, hits if cap else None, cap,
                                                 meta.data_ptr(), counts, meta.data_ptr() + 8)
    return _hit_list(call, "hmse_" + name, n_counts, hits_cap, raw_off.device, refuse)


def _chunk_map(where: str, raw_off, cuts, slot) -> int:
    """The "chunk map" arguments raw_off, cuts and slot agree in their sizes.  -> n_chunks."""
    n_chunks = slot.numel()
    if cuts.numel() != n_chunks + 1 or raw_off.numel() < 1:
        raise HmseError(-1, f"{where}: cuts / slot / raw_off do not match")
    return n_chunks


def _seams(name: str, raw, raw_off, cuts, slot, hits_cap, n_counts: int, *middle, refuse=_BAD_TABLES):
    """A seams entry point hmse_<name>: the chunk map (raw, raw_off, cuts, slot), the family's own `middle` arguments, the hit list."""
    n_chunks = _chunk_map(name, raw_off, cuts, slot)
    call = lambda hits, cap, meta, counts: _call("hmse_" + name, raw, raw.numel(), raw_off, raw_off.numel() - 1, cuts, slot, n_chunks, *middle,
                                                 hits if cap else None, cap, meta.data_ptr(), counts, meta.data_ptr() + 8)
    return _hit_list(call, "hmse_" + name, n_counts, hits_cap, cuts.device, refuse)


def find_scan(raw: torch.Tensor, raw_off: torch.Tensor, mult: torch.Tensor | None, pat: torch.Tensor, pat_off, ignore_case: bool = False,
              hits_cap: int | None = None, raw_bytes: int | None = None):
    """hmse_find_scan: every match of the patterns (`pat` uint8 on the device, `pat_off` host bounds) lying wholly inside one record
    [raw_off[r], raw_off[r + 1]) of `raw`.  -> (hits int64[n] = position in raw << 8 | pattern, any order; n_hits; counts int64[P] =
    per pattern the sum of mult[record] (int32, None: 1 each)).  hits_cap 0: count only (hits empty).  Replaces the read_store +
    host bytes.find loop."""
    bounds, n_pat = _find_bounds(pat, pat_off)
    return _scan("find_scan", raw, raw_off, mult, raw_bytes, hits_cap, n_pat, pat, bounds, n_pat, FIND_IGNORE_CASE if ignore_case else 0)


def find_seams(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, pat: torch.Tensor, pat_off,
               ignore_case: bool = False, hits_cap: int | None = None):
    """hmse_find_seams: the occurrences that start in a chunk and end behind it, read through the chunk map (`cuts` int64[n + 1],
    `slot` int64[n]: the record of every chunk).  -> (hits int64[n] = corpus offset << 8 | pattern, any order; n_hits; counts)."""
    bounds, n_pat = _find_bounds(pat, pat_off)
    return _seams("find_seams", raw, raw_off, cuts, slot, hits_cap, n_pat, pat, bounds, n_pat, FIND_IGNORE_CASE if ignore_case else 0)


def _place(name: str, hits, raw_off, cuts, slot, chunk_out, n_out: int) -> torch.Tensor:
    """hmse_find_place and hmse_findset_place: one kernel template, two widths of the hit word's low field (csrc/chunkmap.h)."""
    n_chunks = slot.numel()
    if cuts.numel() != n_chunks + 1 or chunk_out.numel() != n_chunks + 1 or raw_off.numel() < 1:
        raise HmseError(-1, f"{name}: cuts / slot / chunk_out do not match")
    out = _buf(max(int(n_out), 1), torch.int64, cuts.device)
    status = _status_word(cuts.device)
    _call("hmse_" + name, hits, hits.numel(), raw_off, raw_off.numel() - 1, cuts, slot, n_chunks, chunk_out, out if n_out else None, n_out, status)
    _refuse(status, ((2, -1, "hmse_" + name + " device status {st:#x}: inconsistent tables"),       # (the kernels set bits 0 and 1 only)
                     (1, -2, "hmse_" + name + " device status {st:#x}: chunk_out[-1] exceeds the output")))
    return out[:int(n_out)]


def find_place(hits: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, chunk_out: torch.Tensor, n_out: int) -> torch.Tensor:
    """hmse_find_place: the scan's hits, SORTED ascending, laid out at every chunk that maps to their record.  `chunk_out` int64
    [n_chunks + 1]: exclusive prefix sum of the number of hits of record slot[k]; n_out = chunk_out[-1].  -> int64[n_out] =
    corpus offset << 8 | pattern, ascending."""
    return _place("find_place", hits, raw_off, cuts, slot, chunk_out, n_out)


def _lines_tables(where: str, raw, raw_off, cuts, slot, **more) -> None:
    _chunk_map(where, raw_off, cuts, slot)
    for nm, t in dict(raw_off=raw_off, cuts=cuts, slot=slot, **more).items():
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
    _lines_tables("lines_extent", raw, raw_off, cuts, slot, pos=pos)
    n, dev = pos.numel(), cuts.device
    start, end, flags = _buf(n, torch.int64, dev), _buf(n, torch.int64, dev), _buf(n, torch.uint8, dev)
    status = _status_word(dev)
    _call("hmse_lines_extent", raw, raw.numel(), raw_off, raw_off.numel() - 1, cuts, slot, slot.numel(), pos, n, delim, before, after, reach,
          start, end, flags, status)
    return start, end, flags, _refuse(status, ((2, -1, "hmse_lines_extent device status {st:#x}: inconsistent tables"),))


def lines_gather(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, start: torch.Tensor, end: torch.Tensor,
                 out_off: torch.Tensor, n_out: int) -> torch.Tensor:
    """hmse_lines_gather: the corpus bytes [start[i], end[i]) of every range back to back.  `out_off` int64[n + 1]: exclusive prefix sum
    of end - start; n_out = out_off[-1].  -> uint8[n_out].  HmseError for an out_off[-1] above n_out (status bit 0), for inconsistent
    tables, a range that descends or leaves the corpus, or an out_off that is not the prefix sum (bit 1); nothing was written then."""
    _lines_tables("lines_gather", raw, raw_off, cuts, slot, start=start, end=end, out_off=out_off)
    n = start.numel()
    if end.numel() != n or out_off.numel() != n + 1:
        raise HmseError(-1, "lines_gather: start / end / out_off do not match")
    out = _buf(max(int(n_out), 1), torch.uint8, cuts.device)
    status = _status_word(cuts.device)
    _call("hmse_lines_gather", raw, raw.numel(), raw_off, raw_off.numel() - 1, cuts, slot, slot.numel(), start, end, out_off, n,
          out if n_out else None, n_out, status)
    _refuse(status, ((2, -1, "hmse_lines_gather device status {st:#x}: inconsistent tables, a range that descends or leaves the corpus, "
                             "or out_off is not the prefix sum of the lengths"),
                     (_ANY, -2, "hmse_lines_gather device status {st:#x}: out_off[-1] exceeds the output")))
    return out[:int(n_out)]


_BAD_TALLY = ((2, -1, "{where} device status {st:#x}: inconsistent tables, a range that descends or leaves the corpus, or a rep outside the ranges"),)


def _tally_ranges(where: str, raw, raw_off, cuts, slot, start, end, **more) -> int:
    _lines_tables(where, raw, raw_off, cuts, slot, start=start, end=end, **more)
    n = start.numel()
    if any(t.numel() != n for t in (end, *more.values())):
        raise HmseError(-1, f"{where}: start / end{''.join(' / ' + k for k in more)} do not match")
    return n


def tally_keys(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, start: torch.Tensor, end: torch.Tensor,
               ignore_case: bool = False, seed: int = 0, key_bits: int = 64) -> torch.Tensor:
    """hmse_tally_keys: the key of the (folded) corpus bytes [start[i], end[i]) of every range (include/hmse_tally.h defines it bit for
    bit).  The tables are lines_gather's; int64 tensors carry the u64 bits.  -> key int64[n].  The key only buckets ranges: tally_same
    decides equality.  HmseError for inconsistent tables or a range that descends or leaves the corpus (status bit 1)."""
    n = _tally_ranges("tally_keys", raw, raw_off, cuts, slot, start, end)
    if not 1 <= int(key_bits) <= 64:
        raise HmseError(-1, f"tally_keys: key_bits = {key_bits} lies outside 1..64")
    key = _buf(n, torch.int64, cuts.device)
    status = _status_word(cuts.device)
    _call("hmse_tally_keys", raw, raw.numel(), raw_off, raw_off.numel() - 1, cuts, slot, slot.numel(), start, end, n,
          FIND_IGNORE_CASE if ignore_case else 0, int(seed) & 0xFFFFFFFFFFFFFFFF, key_bits, key, status)
    _refuse(status, _BAD_TALLY, "hmse_tally_keys")
    return key


def tally_same(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, start: torch.Tensor, end: torch.Tensor,
               rep: torch.Tensor, ignore_case: bool = False) -> torch.Tensor:
    """hmse_tally_same: same[i] = 1 iff the ranges i and rep[i] have the same length and the same (folded) bytes.  -> uint8[n].
    HmseError for inconsistent tables, a range that descends or leaves the corpus, or a rep[i] outside [0, n) (status bit 1)."""
    n = _tally_ranges("tally_same", raw, raw_off, cuts, slot, start, end, rep=rep)
    same = _buf(n, torch.uint8, cuts.device)
    status = _status_word(cuts.device)
    _call("hmse_tally_same", raw, raw.numel(), raw_off, raw_off.numel() - 1, cuts, slot, slot.numel(), start, end, rep, n,
          FIND_IGNORE_CASE if ignore_case else 0, same, status)
    _refuse(status, _BAD_TALLY, "hmse_tally_same")
    return same


_BAD_ORDER = ((2, -1, "{where} device status {st:#x}: inconsistent tables, a range that descends or leaves the corpus, a depth beyond its text's end, "
                      "a rep outside the ranges, or a from beyond the shorter of the two texts"),)


def order_keys(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, start: torch.Tensor, end: torch.Tensor,
               depth: torch.Tensor, ignore_case: bool = False) -> torch.Tensor:
    """hmse_order_keys: seven (folded) corpus bytes of every range from text index depth[i] on and the state of its end, as one integer
    that sorts like the texts (include/hmse_order.h defines it bit for bit; below 2^60).  The tables are lines_gather's.  -> key int64[n].
    HmseError for inconsistent tables, a range that descends or leaves the corpus, or a depth[i] above the text's length (status bit 1)."""
    n = _tally_ranges("order_keys", raw, raw_off, cuts, slot, start, end, depth=depth)
    key = _buf(n, torch.int64, cuts.device)
    status = _status_word(cuts.device)
    _call("hmse_order_keys", raw, raw.numel(), raw_off, raw_off.numel() - 1, cuts, slot, slot.numel(), start, end, depth, n,
          FIND_IGNORE_CASE if ignore_case else 0, key, status)
    _refuse(status, _BAD_ORDER, "hmse_order_keys")
    return key


def order_lcp(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, start: torch.Tensor, end: torch.Tensor,
              rep: torch.Tensor, frm: torch.Tensor, ignore_case: bool = False) -> torch.Tensor:
    """hmse_order_lcp: lcp[i] = frm[i] + the number of (folded) bytes the ranges i and rep[i] share from text index frm[i] on; the caller
    promises that the bytes in front of frm[i] agree, and they are not read.  rep[i] == i gives the text's length.  -> int64[n].
    HmseError for inconsistent tables, a range that descends or leaves the corpus, a rep[i] outside [0, n) or a frm[i] beyond the
    shorter of the two texts (status bit 1)."""
    n = _tally_ranges("order_lcp", raw, raw_off, cuts, slot, start, end, rep=rep, **{"from": frm})
    lcp = _buf(n, torch.int64, cuts.device)
    status = _status_word(cuts.device)
    _call("hmse_order_lcp", raw, raw.numel(), raw_off, raw_off.numel() - 1, cuts, slot, slot.numel(), start, end, rep, frm, n,
          FIND_IGNORE_CASE if ignore_case else 0, lcp, status)
    _refuse(status, _BAD_ORDER, "hmse_order_lcp")
    return lcp


SUBST_LITERAL, SUBST_FILL = 0, 1


def subst_apply(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, start: torch.Tensor, end: torch.Tensor,
                sel: torch.Tensor, rep: torch.Tensor, rep_off: torch.Tensor, out_off: torch.Tensor, n_out: int, fill: bool = False) -> torch.Tensor:
    """hmse_subst_apply: the corpus with the ranges [start[i], end[i]) replaced (include/hmse_subst.h has the definitions).  The edits are in
    order and do not overlap; `sel` int64[n] names each edit's replacement among the packed `rep` uint8 / `rep_off` int64[n_rep + 1]; with
    `fill` every replacement is one byte, repeated over its range.  `out_off` int64[n + 1]: where each replacement begins in the output,
    and the output's length; n_out = out_off[-1].  The tables are lines_gather's.  -> uint8[n_out].  HmseError for an out_off[-1] above
    n_out (status bit 0) and for inconsistent tables, edits that break the edit rule, a sel outside the replacements, a bad rep_off, a
    fill replacement that is not one byte or an out_off that is not the definition's (bit 1); not one byte was written then."""
    _lines_tables("subst_apply", raw, raw_off, cuts, slot, start=start, end=end, sel=sel, rep_off=rep_off, out_off=out_off)
    if rep.dtype != torch.uint8:
        raise HmseError(-1, "subst_apply: rep must be torch.uint8")
    n = start.numel()
    if end.numel() != n or sel.numel() != n or out_off.numel() != n + 1 or rep_off.numel() < 1:
        raise HmseError(-1, "subst_apply: start / end / sel / out_off / rep_off do not match")
    n_rep = rep_off.numel() - 1
    if n and not n_rep:
        raise HmseError(-1, "subst_apply: there are edits and no replacement")
    out = _buf(max(int(n_out), 1), torch.uint8, cuts.device)
    status = _status_word(cuts.device)
    _call("hmse_subst_apply", raw, raw.numel(), raw_off, raw_off.numel() - 1, cuts, slot, slot.numel(), start, end, sel, n, rep, rep.numel(),
          rep_off if n_rep else None, n_rep, SUBST_FILL if fill else SUBST_LITERAL, out_off, out if n_out else None, n_out, status)
    _refuse(status, ((2, -1, "hmse_subst_apply device status {st:#x}: inconsistent tables, edits that overlap, descend or leave the corpus, a sel "
                             "outside the replacements, a bad rep_off, a fill replacement that is not one byte, or an out_off that is not the definition's"),
                     (_ANY, -2, "hmse_subst_apply device status {st:#x}: out_off[-1] exceeds the output")))
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
        return _lib.HmseFindset(C.sizeof(_lib.HmseFindset), FIND_IGNORE_CASE if self.ignore_case else 0, self.ukey.numel(), int(self.n_ids),
                                int(self.dir_bits), int(self.max_len), self.upat.numel(), _addr(self.upat), _addr(self.uoff), _addr(self.ukey),
                                _addr(self.uid), _addr(self.dir), _addr(self.bitmap))


def _findset_args(fs: FindSet):
    """-> the set's header (a host struct that names its device arrays, checked here: no parameter of the call is) and the call's flags."""
    for nm in ("upat", "uoff", "ukey", "uid", "dir", "bitmap"):
        _require_gpu(getattr(fs, nm), nm)
    n = fs.ukey.numel()
    if n and (fs.uoff.numel() != n + 1 or fs.uid.numel() != n or fs.dir.numel() != (1 << int(fs.dir_bits)) + 1
              or fs.bitmap.numel() != 1 << (FINDSET_BITMAP_BITS - 5) or any(t.element_size() != 4 for t in (fs.uoff, fs.ukey, fs.uid, fs.dir, fs.bitmap))):
        raise HmseError(-1, "findset: the set's arrays do not match its header")
    return fs.header(), FIND_IGNORE_CASE if fs.ignore_case else 0


def findset_scan(raw: torch.Tensor, raw_off: torch.Tensor, mult: torch.Tensor | None, fs: FindSet, hits_cap: int | None = None,
                 raw_bytes: int | None = None):
    """hmse_findset_scan: every match of the set's patterns lying wholly inside one record of `raw` (find_scan's contract).
    -> (hits int64[n] = position in raw << 24 | id, any order; n_hits; counts int64[n_ids] weighted by mult)."""
    return _scan("findset_scan", raw, raw_off, mult, raw_bytes, hits_cap, int(fs.n_ids), *_findset_args(fs))


def findset_seams(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, fs: FindSet, hits_cap: int | None = None):
    """hmse_findset_seams: the set's occurrences that start in a chunk and end behind it (find_seams' contract).
    -> (hits int64[n] = corpus offset << 24 | id, any order; n_hits; counts int64[n_ids])."""
    return _seams("findset_seams", raw, raw_off, cuts, slot, hits_cap, int(fs.n_ids), *_findset_args(fs))


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
        return _lib.HmseRegex(C.sizeof(_lib.HmseRegex), int(self.n_states), int(self.n_classes), int(self.reach), self.table.data_ptr(),
                              self.classmap.data_ptr())


def _regex_args(rx: Regex):
    _require_gpu(rx.table, "table")
    _require_gpu(rx.classmap, "classmap")
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
    return _scan("regex_scan", raw, raw_off, mult, raw_bytes, hits_cap, 1, _regex_args(rx), refuse=_BAD_TABLES_OR_AUTOMATON)


def regex_seams(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, rx: Regex, hits_cap: int | None = None):
    """hmse_regex_seams: the occurrence of the regex at every SEAM start o of every chunk (cuts[k + 1] - o < reach), walked through
    the chunk map.  -> (hits int64[n] = corpus offset << 8 | (length - 1), any order; n_hits; count int64[1] = n_hits)."""
    return _seams("regex_seams", raw, raw_off, cuts, slot, hits_cap, 1, _regex_args(rx), refuse=_BAD_TABLES_OR_AUTOMATON)


@dataclass
class RegexA:
    """The device arrays and the header of a regular expression compiled with assertions (include/hmse_regexa.h `hmse_regexa`; built by
    regex.Regex(assertions=True))."""
    table: torch.Tensor          # int16 [n_states * n_classes]: the bits of the u16 entries
    classmap: torch.Tensor       # uint8 [256]
    n_states: int
    n_classes: int               # the EDGE class (the last one) included
    reach: int
    start: tuple                 # the four start states, by the kind of the byte in front

    def header(self) -> "_lib.HmseRegexa":
        return _lib.HmseRegexa(C.sizeof(_lib.HmseRegexa), int(self.n_states), int(self.n_classes), int(self.reach),
                               (C.c_uint32 * 4)(*(int(v) for v in self.start)), self.table.data_ptr(), self.classmap.data_ptr())


def _regexa_args(rx: RegexA):
    if len(rx.start) != 4:
        raise HmseError(-1, "regexa: an automaton has four start states")
    return _regex_args(rx)


def regexa_scan(raw: torch.Tensor, raw_off: torch.Tensor, mult: torch.Tensor | None, rx: RegexA, hits_cap: int | None = None,
                raw_bytes: int | None = None):
    """hmse_regexa_scan: the occurrence of the asserting regex at every SCAN start p of every record (p > raw_off[r] and
    raw_off[r + 1] - p > reach: the byte in front, the match and its look-ahead byte lie in the record).  Returns what regex_scan returns."""
    return _scan("regexa_scan", raw, raw_off, mult, raw_bytes, hits_cap, 1, _regexa_args(rx), refuse=_BAD_TABLES_OR_AUTOMATON)


def regexa_seams(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, rx: RegexA, hits_cap: int | None = None):
    """hmse_regexa_seams: the occurrence of the asserting regex at every SEAM start o of every non-empty chunk k (o == cuts[k] or
    cuts[k + 1] - o <= reach), both context bytes read through the chunk map.  Returns what regex_seams returns."""
    return _seams("regexa_seams", raw, raw_off, cuts, slot, hits_cap, 1, _regexa_args(rx), refuse=_BAD_TABLES_OR_AUTOMATON)


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
    bounds, ks, n_pat = _approx_bounds(pat, pat_off, k)
    return _scan("approx_scan", raw, raw_off, mult, raw_bytes, hits_cap, n_pat, pat, bounds, ks, n_pat, FIND_IGNORE_CASE if ignore_case else 0)


def approx_seams(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, pat: torch.Tensor, pat_off, k,
                 ignore_case: bool = False, hits_cap: int | None = None):
    """hmse_approx_seams: every SEAM end of every chunk — the first m_j + k[j] - 1 ends of the chunk, walked through the chunk map from
    m_j + k[j] bytes in front.  -> (hits int64[n] = corpus offset of the match's last byte << 8 | errors << 3 | pattern, any order;
    n_hits; counts int64[P] = the seam hits per pattern)."""
    bounds, ks, n_pat = _approx_bounds(pat, pat_off, k)
    return _seams("approx_seams", raw, raw_off, cuts, slot, hits_cap, n_pat, pat, bounds, ks, n_pat, FIND_IGNORE_CASE if ignore_case else 0)


def approx_spans(raw: torch.Tensor, raw_off: torch.Tensor, cuts: torch.Tensor, slot: torch.Tensor, pat: torch.Tensor, pat_off,
                 ignore_case: bool, hits: torch.Tensor):
    """hmse_approx_spans: for every hit word (CORPUS offset of the last byte << 8 | errors << 3 | pattern; int64, any order) the start
    of its shortest best match.  -> (start int64[n], status: bit 0 = some hit lies outside the corpus, names no pattern or has errors
    that no text ending there attains; its start is offset + 1).  Inconsistent tables (status bit 1) raise HmseError."""
    _chunk_map("approx_spans", raw_off, cuts, slot)
    if hits.dtype != torch.int64:
        raise HmseError(-1, "approx_spans: hits must be torch.int64 (the bits of the u64 hit words)")
    bounds, _, n_pat = _approx_bounds(pat, pat_off)
    n, dev = hits.numel(), cuts.device
    start = _buf(max(n, 1), torch.int64, dev)
    status = _status_word(dev)
    _call("hmse_approx_spans", raw, raw.numel(), raw_off, raw_off.numel() - 1, cuts, slot, slot.numel(), pat, bounds, n_pat,
          FIND_IGNORE_CASE if ignore_case else 0, hits, n, start if n else None, status)
    return start[:n], _refuse(status, ((2, -1, "hmse_approx_spans device status {st:#x}: inconsistent tables"),))


def crc32(data: torch.Tensor, cuts: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """hmse_crc32: the zlib / gzip CRC-32 of every range data[cuts[k], cuts[k + 1]) (`cuts` int64[n + 1], ascending; ranges may be empty,
    start at any byte and have any length).  -> int32[n] (u32 bits; `out` if given).  Descending cuts or cuts[-1] > data.numel() are
    refused and `out` is left as it was."""
    n = cuts.numel() - 1
    if n < 0:
        raise HmseError(-1, "crc32: cuts is empty")
    dev = cuts.device
    if out is None:
        out = _buf(n, torch.int32, dev)
    if out.numel() != n or out.dtype != torch.int32:
        raise HmseError(-1, "crc32: out is not int32[n]")
    status = _status_word(dev)
    _call("hmse_crc32", data, data.numel(), cuts, n, out, status)
    if n:
        _refuse(status, ((_ANY, -1, "hmse_crc32: cuts descends or ends behind the data"),))
    return out


def crc32_combine(crc: torch.Tensor, lens: torch.Tensor) -> int:
    """hmse_crc32_combine: the CRC-32 of the concatenation of ranges given only their CRCs (int32[n], u32 bits) and lengths (int64[n];
    exponents only: any values whose sum stays below 2^61).  -> the CRC as a Python int (0 for n == 0)."""
    n = crc.numel()
    if lens.numel() != n or crc.dtype != torch.int32 or lens.dtype != torch.int64:
        raise HmseError(-1, "crc32_combine: crc int32[n] / lens int64[n] do not match")
    meta = _buf(2, torch.int32, crc.device, fill=0)       # [out, status]
    _call("hmse_crc32_combine", crc, lens, n, meta.data_ptr(), meta.data_ptr() + 4)
    return int(meta[0].item()) & 0xFFFFFFFF


def gzip_members(src0: torch.Tensor, src1: torch.Tensor | None, src_off: torch.Tensor, stream_len: torch.Tensor, src_sel: torch.Tensor,
                 crc: torch.Tensor, raw_off: torch.Tensor, slot: torch.Tensor, member_off: torch.Tensor, bgzf: bool = False,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """hmse_gzip_members: one gzip (or BGZF) member per chunk at member_off (int64[n_chunks + 1], the caller's prefix sum of header +
    stream + 8): header, the stream of record slot[i] — stream_len[r] bytes at src_off[r] of (src1 if src_sel[r] else src0) —, crc[r]
    and the record's raw length raw_off[r + 1] - raw_off[r].  Returns the uint8 destination (`out`, or a new tensor of member_off[-1]
    bytes).  A member outside its source or destination, or a size that is not header + stream + 8, is refused: nothing is written."""
    n_rec, n_chunks = src_off.numel(), slot.numel()
    if stream_len.numel() != n_rec or src_sel.numel() != n_rec or crc.numel() != n_rec or raw_off.numel() != n_rec + 1 or member_off.numel() != n_chunks + 1:
        raise HmseError(-1, "gzip_members: the record tables / slot / member_off do not match")
    if crc.dtype != torch.int32 or src_sel.dtype != torch.uint8 or any(t.dtype != torch.int64 for t in (src_off, stream_len, raw_off, slot, member_off)):
        raise HmseError(-1, "gzip_members: crc int32, src_sel uint8, the other tables int64")
    dev = member_off.device
    if out is None:
        out = _buf(int(member_off[-1].item()), torch.uint8, dev)
    status = _status_word(dev)
    _call("hmse_gzip_members", src0, src0.numel(), src1, 0 if src1 is None else src1.numel(), src_off, stream_len, src_sel, crc, raw_off, n_rec,
          slot, n_chunks, member_off, GZIP_BGZF if bgzf else 0, out, out.numel(), status)
    if n_chunks:
        _refuse(status, ((1, -2, "hmse_gzip_members: a member lies outside its source or the destination, or its size is not header + stream + 8"),
                         (2, -2, "hmse_gzip_members: a BGZF member above 65536 bytes")))
    return out


GZIP_VALID, GZIP_FAST, GZIP_WHY_SHIFT = 1, 2, 2
GZIP_WHY = {1: "header", 2: "stream", 3: "length", 4: "bounds"}
GZIP_MIN_MEMBER = 20


def gzip_workspace_bytes(n: int) -> int:
    return _host("hmse_gzip_workspace_bytes", int(n))


def gzip_candidates(data: torch.Tensor, cap: int, out: torch.Tensor | None = None):
    """hmse_gzip_candidates: every position of `data` (uint8) that could start a gzip member — 1f 8b 08, no reserved FLG bit, 20 bytes of
    room —, ascending.  -> (int64[cap] (`out` if given), their number as a Python int — one host sync).  Only min(number, cap) entries
    are written; the rest of the tensor is left as it was."""
    _require_gpu(data, "data")
    dev = data.device
    if out is None:
        out = _buf(cap, torch.int64, dev)
    if out.numel() != cap or out.dtype != torch.int64:
        raise HmseError(-1, "gzip_candidates: out is not int64[cap]")
    meta = _buf(2, torch.int64, dev, fill=0)               # [count, status (its low word)]
    ws = _ws(gzip_workspace_bytes(data.numel()), dev)
    _call("hmse_gzip_candidates", data, data.numel(), out, cap, meta.data_ptr(), meta.data_ptr() + 8, ws, ws.numel())
    return out, int(meta[0].item())


def gzip_measure(data: torch.Tensor, cand_off: torch.Tensor):
    """hmse_gzip_measure: one wavefront per candidate offset (int64[n]) parses the header and finds the member's end — from the BC
    subfield of a BGZF block, else by walking the DEFLATE stream for its length.  -> (stream_off int64[n], end int64[n], raw_len int64[n],
    crc int32[n] (u32 bits), flags int32[n]: GZIP_VALID | GZIP_FAST, or reason << GZIP_WHY_SHIFT (GZIP_WHY))."""
    _require_gpu(data, "data")
    dev = data.device
    n = cand_off.numel()
    if cand_off.dtype != torch.int64:
        raise HmseError(-1, "gzip_measure: cand_off is not int64")
    stream_off, end, raw_len = (_buf(n, torch.int64, dev) for _ in range(3))
    crc, flags = (_buf(n, torch.int32, dev) for _ in range(2))
    status = _status_word(dev)
    ws = _ws(gzip_workspace_bytes(data.numel()), dev)
    _call("hmse_gzip_measure", data, data.numel(), cand_off, n, stream_off, end, raw_len, crc, flags, status, ws, ws.numel())
    return stream_off, end, raw_len, crc, flags
