"""Garbage collection: drop segments from a merged store of one or more shards and collect its records on the GPU.

The ChunkIndex refcount is kept "for garbage collection" (README.md:1268, 1886); this module is what reads it back
out of the chunk map.  The unit of deletion is the SEGMENT: L2 restarts its Gear hash at every segment start, so a segment
boundary is always a cut, and the store that remains after dropping segments is defined exactly — it is, byte for byte, what
a fresh ingest writes for the concatenation R of the surviving segments (`build_manifest(ingest_shard(R, cfg, seg_off=R_seg_off))`):
  * L2  the surviving segments keep their cuts;
  * L3  digests come from the old ChunkIndex; a slot's new first occurrence is its first SURVIVING reference (hmse_gc_plan), so a
        POINTER whose stored chunk was dropped is promoted to a stored chunk;
  * L4  a signature depends only on the chunk's bytes: hmse_l4_lsh runs again over the surviving signatures in their new order;
  * L1  the record of a (chunk, dictionary) pair is deterministic: it is reused when the pair is unchanged and re-encoded by
        hmse_l1_deflate otherwise; hmse_record_gather assembles the dense streams from both sources in one launch.
The packing is the unchanged manifest.pack_manifest_device of a fresh ingest.
There is ONE body (_collect) for N >= 1 shards; a Manifest or a Store of one shard is its N = 1 case.  A store of several shards has
the same definition shard by shard — the store a fresh sharded ingest (ingest_shards_local) of every shard's surviving segments
writes — with one plan over the concatenated chunk map, L4 in the store's scope (shard-local or global, remote dictionaries
included) and stored chunks that move to the shard of their first surviving reference.  A multi-rank stream's store (pieces) and
an unmerged part are refused (manifest.merged_shards).
"""
from __future__ import annotations

import time

import numpy as np

from .config import KIND_DELTA, KIND_POINTER, LAYER_L1, LAYER_L2, LAYER_L3, LAYER_L4, IngestConfig
from .manifest import Manifest, Store, merged_shards

SUPPORTED_LAYERS = (LAYER_L1 | LAYER_L2 | LAYER_L3 | LAYER_L4, LAYER_L1 | LAYER_L2 | LAYER_L3)   # "full", "l1_cdc_dedupe"


def _sharded(m) -> bool:
    """A Store of several shards takes and returns per-shard lists; a Manifest or a Store of one shard the single items."""
    return isinstance(m, Store) and len(m.shards) > 1


def _check_layers(cfg: IngestConfig) -> None:
    if not (cfg.layers & LAYER_L1 and cfg.layers & LAYER_L3):
        raise ValueError("gc: the store needs the L1 records and the L3 index (layer masks without L1 or L3 are not collectable)")
    if cfg.layers not in SUPPORTED_LAYERS:
        raise ValueError(f"gc: layer mask {cfg.layers:#x} is not supported (full or l1_cdc_dedupe)")


def store_cuts(m: Manifest) -> np.ndarray:
    """Old chunk ends from the chunk map's raw lengths: int64[n_chunks + 1]."""
    return np.concatenate([[0], np.cumsum(m.chunk_map["raw_length"].astype(np.int64))]).astype(np.int64)


def store_seg_off(m: Manifest, cfg: IngestConfig, seg_off=None, cuts: np.ndarray | None = None) -> np.ndarray:
    """The store's segment table (None: the fixed cfg.seg_size grid), checked against its cut list: every segment boundary must
    be a cut, otherwise the store was not ingested with this seg_size / seg_off."""
    cuts = store_cuts(m) if cuts is None else cuts
    n = int(cuts[-1])
    if seg_off is None:
        k = max(1, -(-n // cfg.seg_size))
        so = np.minimum(np.arange(k + 1, dtype=np.int64) * cfg.seg_size, n)
    else:
        so = np.asarray(seg_off.cpu() if hasattr(seg_off, "cpu") else seg_off, np.int64).reshape(-1)
        if len(so) < 2 or so[0] != 0 or so[-1] != n or (np.diff(so) < 0).any():
            raise ValueError(f"gc: seg_off must run from 0 to the store's {n} bytes, ascending")
    missing = so[~np.isin(so, cuts)]
    if len(missing):
        raise ValueError(f"gc: the store's cut list misses segment boundary {int(missing[0])} (and {len(missing) - 1} more): "
                         "it was not ingested with this seg_size / seg_off")
    return so


def segments_of_ranges(seg_off: np.ndarray, ranges) -> list:
    """[(offset, len), ...] of segment-aligned byte ranges -> the sorted segment indices they cover.  A range that does not start
    and end on a segment boundary raises ValueError naming the nearest boundaries."""
    so = np.asarray(seg_off, np.int64)
    out = set()
    for off, ln in ranges:
        off, ln = int(off), int(ln)
        if off < 0 or ln < 0 or off + ln > int(so[-1]):
            raise ValueError(f"gc: range ({off}, {ln}) lies outside the store's {int(so[-1])} bytes")
        for x in (off, off + ln):
            if not (so == x).any():
                i = int(np.searchsorted(so, x))
                raise ValueError(f"gc: range ({off}, {ln}) is not segment-aligned: byte {x} lies between segment boundaries "
                                 f"{int(so[i - 1])} and {int(so[i])}")
        lo = int(np.searchsorted(so, off, side="left"))
        hi = int(np.searchsorted(so, off + ln, side="left"))
        out.update(range(lo, hi))
    return sorted(out)


def shard_segments(store: Store, cfg: IngestConfig, seg_off=None):
    """A merged store's segment tables: (per shard its own table, checked against its cut list as store_seg_off does;
    the global table — the shards' tables shifted by the shard byte offsets, shard 0's segments first; the first global segment
    index of every shard, int64[n_shards + 1]).  `seg_off`: a list of per-shard local tables (None entries or None: cfg.seg_size)."""
    return _segment_tables(merged_shards(store, "gc"), cfg, seg_off)


def _segment_tables(shards: list, cfg: IngestConfig, seg_off=None):
    if seg_off is not None and len(seg_off) != len(shards):
        raise ValueError(f"gc: seg_off must hold one segment table per shard ({len(shards)}), got {len(seg_off)}")
    sos = [store_seg_off(m, cfg, None if seg_off is None else seg_off[i]) for i, m in enumerate(shards)]
    byte_base = np.cumsum([0] + [int(so[-1]) for so in sos]).astype(np.int64)
    so_g = np.concatenate([[0]] + [so[1:] + byte_base[i] for i, so in enumerate(sos)]).astype(np.int64)
    seg_base = np.cumsum([0] + [len(so) - 1 for so in sos]).astype(np.int64)
    return sos, so_g, seg_base


def split_segments(seg_base: np.ndarray, drop) -> list:
    """Global segment indices -> per shard the sorted local segment indices they name."""
    d = np.asarray(sorted({int(x) for x in drop}), np.int64)
    if len(d) and (d[0] < 0 or d[-1] >= int(seg_base[-1])):
        raise ValueError(f"gc: segment index out of range (the store has {int(seg_base[-1])} segments)")
    sh = np.searchsorted(seg_base, d, side="right") - 1
    return [(d[sh == i] - seg_base[i]).tolist() for i in range(len(seg_base) - 1)]


def drop_ranges(m, ranges, cfg: IngestConfig, device, band_tables=None, seg_off=None, global_l4: bool = False, verify: bool = True,
                timings=None):
    """drop_segments() of the segments that the segment-aligned byte ranges [(offset, len), ...] cover (a sharded store: ranges of
    the original corpus, the shards concatenated in shard order)."""
    _check_layers(cfg)
    sos, so_g, _ = _segment_tables(merged_shards(m, "gc"), cfg, seg_off if _sharded(m) else [seg_off])
    return drop_segments(m, segments_of_ranges(so_g, ranges), cfg, device, band_tables=band_tables, seg_off=sos if _sharded(m) else sos[0],
                         global_l4=global_l4, verify=verify, timings=timings)


def drop_segments(m, drop, cfg: IngestConfig, device, band_tables=None, seg_off=None, global_l4: bool = False, verify: bool = True,
                  timings=None):
    """Drop the segments `drop` from a merged store and collect its records.  `m`: a Manifest or a Store of one shard — `drop` holds
    indices into its segment table (`seg_off`, or the fixed cfg.seg_size grid when None), `band_tables` is its band-table sidecar
    (StreamIngest.index_sidecar()) and (Manifest, sidecar bytes or None, stats) comes back — or a Store of N > 1 shards: `drop`
    holds GLOBAL segment indices (shard 0's segments first, each shard's as store_seg_off numbers them; a zero-byte shard keeps its
    one empty segment), `band_tables` one sidecar per shard or None, `seg_off` per-shard local tables or None, `global_l4` names
    the store's dictionary scope, and (Store, [N sidecars] or None, stats) comes back.  With R_i the surviving segments of shard i:
      * to_bytes() equals that of merge_manifests([build_manifest(r, i, N) for r in ingest_shards_local([R_0..], cfg,
        global_l4=global_l4, seg_offs=[..])]) — for one shard build_manifest(ingest_shard(R, cfg, seg_off=R_seg_off));
      * sidecar i equals write_band_tables(r_i.band_keys, cfg.band_bits, signatures=r_i.sig) — for one shard
        StreamIngest.index_sidecar() after ingesting R (layer mask "full"; None for "l1_cdc_dedupe").
    WITH the sidecars only the records to re-encode and their new dictionaries are decoded (one hmse_l1_inflate over their
    dictionary closure).  WITHOUT them the whole store is decoded and every stored chunk goes through hmse_l4_minhash — the cost of
    a read of the store plus the MinHash stage of an ingest.
    The old record of a stored chunk is reused iff it was made with the dictionary the new LSH picks; the old dictionaries of FULL
    records (rule 7 fallbacks do not store one) are recomputed by hmse_l4_lsh over all old signatures, and every DELTA header must
    agree with that recomputation — otherwise the store was not written under this cfg (a windowed stream, the other L4 scope,
    other LSH parameters) and ValueError is raised rather than a store that differs from a fresh ingest.  `verify` checks the
    SHA-256 of every decoded chunk.  Supported layer masks: "full" and "l1_cdc_dedupe".
    `timings` (a dict, diagnostics): filled with per-phase milliseconds (synchronising between phases)."""
    _check_layers(cfg)
    shards = merged_shards(m, "gc")
    if _sharded(m):
        return _collect(shards, drop, cfg, device, band_tables, seg_off, global_l4, verify, timings)
    # one shard: every dictionary is local, so there is no L4 scope to name — `global_l4` means nothing and is not passed on
    out, sides, stats = _collect(shards, drop, cfg, device, None if band_tables is None else [band_tables], [seg_off], False, verify, timings)
    return out.shards[0], None if sides is None else sides[0], stats


def _collect(shards: list, drop, cfg: IngestConfig, device, band_tables, seg_off, global_l4: bool, verify: bool, timings):
    """drop_segments() of the N >= 1 shards of a merged store -> (Store, [N sidecars] or None, stats).
    One hmse_gc_plan runs over the concatenated chunk map (global slot = slot base of the chunk map's shard + slot; the global chunk
    order (shard, local) is the order in which a sharded ingest picks first occurrences), so the plan's new chunk and slot numbers
    are the fresh run's global numbers; they are split per shard at the new chunk bases.  A stored chunk whose first surviving
    reference lies on another shard MIGRATES there.  L4 is recomputed per shard (shard-local) or over all shards (`global_l4`); a
    record is reused iff its dictionary (an old global slot) is unchanged — from the old blobs, back to back as StoreReader holds
    them, whatever its shard.  The sidecars are written on the GPU (hmse_band_tables_write)."""
    N = len(shards)
    sos, so_g, seg_base = _segment_tables(shards, cfg, seg_off)
    n_seg = int(seg_base[-1])
    drop = sorted({int(d) for d in drop})
    if drop and (drop[0] < 0 or drop[-1] >= n_seg):
        raise ValueError(f"gc: segment index out of range (the store has {n_seg} segments)")
    use_l4 = bool(cfg.layers & LAYER_L4)
    if use_l4 and band_tables is not None and len(band_tables) != N:
        raise ValueError(f"gc: one band-table sidecar per shard ({N}), got {len(band_tables)}")
    nc_l = [len(m.chunk_map) for m in shards]
    nu_l = [len(m.index) for m in shards]
    cbase = np.cumsum([0] + nc_l).astype(np.int64)
    sbase = np.cumsum([0] + nu_l).astype(np.int64)
    nc, nu = int(cbase[-1]), int(sbase[-1])
    own_l = []
    for i, m in enumerate(shards):
        own = np.nonzero(m.chunk_map["kind"] != KIND_POINTER)[0]
        if len(own) != nu_l[i] or not np.array_equal(m.chunk_map["slot"][own], np.arange(nu_l[i])) or (m.chunk_map["shard"][own] != i).any():
            raise ValueError(f"gc: shard {i}'s index and chunk map disagree on its stored chunks")
        if nu_l[i] and not m.index["sha256"].any():
            raise ValueError("gc: the store carries no SHA-256 digests (L3)")
        own_l.append(own + cbase[i])
    if any((m.chunk_map["shard"] >= N).any() for m in shards):
        raise ValueError("gc: a chunk map entry names a shard outside the store")
    keys_side = sig_side = None
    if use_l4 and band_tables is not None:
        from . import bandtable
        ks, ss = [], []
        for i, bt in enumerate(band_tables):
            k, sg = bandtable.read_signatures(bt)
            if sg is None or sg.shape != (nu_l[i], cfg.n_hashes) or k.shape != (nu_l[i], cfg.bands):
                raise ValueError(f"gc: band-table sidecar {i} does not belong to shard {i} of this store / configuration")
            ks.append(k); ss.append(sg)
        keys_side, sig_side = np.concatenate(ks), np.concatenate(ss)

    import torch

    from . import bandtable, ingest, manifest, ops, read
    dev = torch.device(device)
    t = lambda a, dt: read.to_device(a, dt, dev)
    clock = _Clock(timings)
    drop_mask = np.zeros(n_seg, np.uint8)
    drop_mask[drop] = 1
    stats = {"segments_dropped": len(drop), "chunks_before": nc, "stored_before": nu, "blob_bytes_before": int(sum(m.blob.size for m in shards)),
             "bytes_decoded": 0}

    # --- plan over the concatenated chunk map: global cuts, global slots, global segment table
    cuts_np = np.concatenate([[0]] + [store_cuts(m)[1:] + int(so_g[seg_base[i]]) for i, m in enumerate(shards)]).astype(np.int64)
    slot_np, _ = read.chunk_slots(shards)
    sha_np = np.concatenate([m.index["sha256"] for m in shards]).reshape(nu, 32)
    cuts_old = t(cuts_np, torch.int64)
    plan = ops.gc_plan(cuts_old, t(slot_np.astype(np.int32), torch.int32), nu, t(so_g, torch.int64), t(drop_mask, torch.uint8), t(sha_np, torch.uint8))
    n_new, u_new = plan["old_chunk"].numel(), plan["old_slot"].numel()
    old_slot, new_slot_of_old = plan["old_slot"], plan["new_slot_of_old"]
    # new chunk bases (surviving chunks per shard) and new slot bases (stored chunks per shard): one host sync
    ncb = torch.searchsorted(plan["old_chunk"], t(cbase, torch.int64))
    nub = torch.searchsorted(plan["uniq_ids"], ncb)
    b = torch.cat([ncb, nub]).tolist()
    new_cb, new_ub = b[:N + 1], b[N + 1:]
    lens_new = (cuts_old[1:] - cuts_old[:-1])[plan["old_chunk"]]
    clock.lap("plan")

    rd = read.StoreReader(Store(shards), dev)        # every shard's blob in HBM, back to back; record headers parsed (global slots)
    if not np.array_equal(rd.slot, slot_np):
        raise ValueError("gc: the store's dictionaries do not precede their records (not the store of a one-shot sharded ingest)")
    kind_old = t(rd.kind, torch.uint8)
    raw_all = raw_off_all = None

    def decode(slots=None):
        """rd.decode() of the stored slots `slots` (ascending, closed under dictionaries; None: all), counted in the stats."""
        stats["bytes_decoded"] += int((rd.raw_len if slots is None else rd.raw_len[slots]).sum())
        return rd.decode(slots, verify)

    def lsh(sig, bases):
        """Band keys and dictionaries (global slots, -1 none) of `sig`: one LSH over all rows (global L4) or one per shard."""
        if global_l4:
            return ops.l4_lsh(sig, cfg)
        ks, bs = [], []
        for i in range(N):
            k, bb = ops.l4_lsh(sig[bases[i]: bases[i + 1]], cfg)
            ks.append(k); bs.append(torch.where(bb >= 0, bb + bases[i], bb))
        return torch.cat(ks), torch.cat(bs)

    # --- L4: old signatures, the old dictionaries (recomputed in the store's scope), the new ones
    sig_new = keys_new = base_new = None
    if use_l4:
        if sig_side is not None:
            sig_old = t(sig_side.view(np.int32), torch.int32)
        else:
            raw_all, raw_off_all = decode()
            clock.lap("decode")
            sig_old = ops.l4_minhash(raw_all, raw_off_all, cfg)
            clock.lap("minhash")
        keys_old, base_old = lsh(sig_old, [int(x) for x in sbase])
        hdr_base = t(rd.base, torch.int64)
        if not bool(((kind_old != KIND_DELTA) | (hdr_base == base_old)).all()):
            raise ValueError(f"gc: a DELTA record's dictionary is not the LSH base of its chunk in the {'global' if global_l4 else 'shard-local'} "
                             "scope under this configuration (the store was written with the other L4 scope, other LSH parameters or by a "
                             "windowed stream)")
        if keys_side is not None and not torch.equal(keys_old, t(keys_side.view(np.int32), torch.int32)):
            raise ValueError("gc: the sidecars' band keys are not those of their signatures under this configuration")
        sig_new = sig_old[old_slot]
        keys_new, base_new = lsh(sig_new, new_ub)
        base_new_old = torch.where(base_new >= 0, old_slot[base_new.clamp(min=0)], base_new)
        old_base = base_old[old_slot]
        reuse = old_base == base_new_old
        clock.lap("lsh")
    else:
        base_new_old = old_base = torch.full((u_new,), -1, dtype=torch.int64, device=dev)
        reuse = torch.ones(u_new, dtype=torch.bool, device=dev)

    j_idx = torch.arange(u_new, dtype=torch.int64, device=dev)
    own_old = t(np.concatenate(own_l) if own_l else np.zeros(0, np.int64), torch.int64)
    promoted = plan["old_chunk"][plan["uniq_ids"]] != own_old[old_slot]
    shard_old = torch.searchsorted(t(sbase, torch.int64), old_slot, right=True) - 1
    shard_new = torch.searchsorted(t(np.asarray(new_ub, np.int64), torch.int64), j_idx, right=True) - 1
    migrated = shard_old != shard_new
    ob_new = torch.where(old_base >= 0, new_slot_of_old[old_base.clamp(min=0)], old_base)
    base_gone = (old_base >= 0) & ((ob_new < 0) | (ob_new > j_idx))
    redo = ~reuse
    enc = redo.nonzero().flatten()
    n_enc = int(enc.numel())

    # --- L1: re-encode (one hmse_l1_inflate over the dictionary closure across shards, hmse_l1_deflate by chunk id)
    src1 = None
    kind_e = torch.zeros(0, dtype=torch.uint8, device=dev)
    off_e = torch.zeros(1, dtype=torch.int64, device=dev)
    if n_enc:
        slots_e = old_slot[enc]
        bases_e = base_new_old[enc]
        if raw_all is not None:
            data, dcuts = raw_all, raw_off_all
            cid, bid = slots_e, bases_e
        else:
            se, be = slots_e.cpu().numpy(), bases_e.cpu().numpy()
            need = rd.closure(np.concatenate([se, be[be >= 0]]))
            data, dcuts = decode(need)
            clock.lap("decode")
            need_d = t(need, torch.int64)
            cid = torch.searchsorted(need_d, slots_e)
            bid = torch.where(bases_e >= 0, torch.searchsorted(need_d, bases_e.clamp(min=0)), bases_e)
        src1, off_e, kind_e = ops.l1_deflate(data, dcuts, cfg, cid, bid, base_is_chunk_id=True)
        del data, dcuts
        clock.lap("reencode")
    raw_all = raw_off_all = None

    # --- gather: every shard's dense streams back to back (one launch), each shard's a slice
    rec_e = torch.full((u_new,), n_enc, dtype=torch.int64, device=dev)
    rec_e[enc] = torch.arange(n_enc, dtype=torch.int64, device=dev)
    z64 = torch.zeros(1, dtype=torch.int64, device=dev)
    e_off, e_len = torch.cat([off_e[:-1], z64]), torch.cat([off_e[1:] - off_e[:-1], z64])
    e_kind = torch.cat([kind_e, torch.zeros(1, dtype=torch.uint8, device=dev)])
    s_off_old, s_len_old = t(rd.stream_off, torch.int64), t(rd.stream_len, torch.int64)
    src_off = torch.where(redo, e_off[rec_e], s_off_old[old_slot])
    s_len = torch.where(redo, e_len[rec_e], s_len_old[old_slot])
    kind_new = torch.where(redo, e_kind[rec_e], kind_old[old_slot])
    stream_off = torch.zeros(u_new + 1, dtype=torch.int64, device=dev)
    torch.cumsum(s_len, 0, out=stream_off[1:])
    streams = ops.record_gather(rd.blob, src1, src_off, redo.to(torch.uint8), stream_off)
    clock.lap("gather", nbytes=2 * int(streams.numel()))
    del rd, src1

    # --- pack: N ShardResults of the fresh sharded ingest, through the unchanged packing code
    parts = []
    for i in range(N):
        a, e, ua, ue = new_cb[i], new_cb[i + 1], new_ub[i], new_ub[i + 1]
        cuts_i = torch.zeros(e - a + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens_new[a:e], 0, out=cuts_i[1:])
        so_i = stream_off[ua: ue + 1] - stream_off[ua]
        base_i = bg = None
        if use_l4:
            bg = base_new[ua:ue]
            base_i = torch.where((bg >= ua) & (bg < ue), bg - ua, torch.full_like(bg, -1))
        res = ingest.ShardResult(int(lens_new[a:e].sum().item()) if e > a else 0, cuts_i, plan["digests"][a:e], a, n_new, plan["first_occ"][a:e],
                                 plan["refcount"][a:e], plan["uniq_ids"][ua:ue] - a, sig_new[ua:ue] if use_l4 else None,
                                 keys_new[ua:ue] if use_l4 else None, base_i, streams[int(stream_off[ua]): int(stream_off[ue])], so_i,
                                 kind_new[ua:ue], shard_bases=new_cb[:N])
        if use_l4 and global_l4:
            res.base_global, res.u_base, res.u_bases = bg, ua, new_ub[:N]
        parts.append(manifest.build_manifest(res, i, N))
    out = manifest.merge_manifests(parts)
    clock.lap("pack")
    sides = None
    if use_l4:
        sides = [bandtable.write_band_tables_device(keys_new[new_ub[i]: new_ub[i + 1]], cfg.band_bits, signatures=sig_new[new_ub[i]: new_ub[i + 1]])
                 for i in range(N)]
        clock.lap("sidecar")
    changed = redo & (kind_new != kind_old[old_slot])
    r_prom, r_gone, r_changed = int((redo & promoted).sum()), int((redo & ~promoted & base_gone).sum()), int((redo & ~promoted & ~base_gone).sum())
    stats.update({"chunks_after": n_new, "stored_after": u_new, "records_reused": u_new - n_enc, "records_reencoded": n_enc,
                  "reencoded_promoted": r_prom, "reencoded_base_dropped_or_moved": r_gone, "reencoded_base_changed": r_changed,
                  "promoted": int(promoted.sum()), "kind_changed": int(changed.sum()), "blob_bytes_after": int(sum(m.blob.size for m in out.shards)),
                  "records_migrated": int(migrated.sum()),
                  "per_shard": [{"chunks_after": new_cb[i + 1] - new_cb[i], "stored_after": new_ub[i + 1] - new_ub[i]} for i in range(N)]})
    return out, sides, stats


class _Clock:
    """Per-phase wall time with a device sync at every lap — only when the caller asked for timings."""

    def __init__(self, out):
        self.out = out
        if out is not None:
            import torch
            torch.cuda.synchronize()
            self.t = time.perf_counter()

    def lap(self, name: str, nbytes: int = 0) -> None:
        if self.out is None:
            return
        import torch
        torch.cuda.synchronize()
        now = time.perf_counter()
        ms = (now - self.t) * 1e3
        self.out[name] = self.out.get(name, 0.0) + ms
        if nbytes:
            self.out[name + "_bytes"] = nbytes
        self.t = now
