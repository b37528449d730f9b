"""Scrub a store on the GPU: which records are intact, which chunks and byte ranges of the corpus are lost, and from which damaged
record each loss comes (the reference's archive duties "Detect ... Preserve existing data ... Report degraded state clearly",
README.md:771-778, with the SHA-256 round trip as the integrity gate, README.md:1329).

scrub()   decodes every record once — hmse_scrub_records (structure, DeltaChunk headers, padding), hmse_l1_inflate with per-record
          ok flags, hmse_l3_sha256, hmse_scrub_attribute (roots by pointer doubling, chunk roots, per-root losses, damaged ranges) —
          and never raises on damage.  Only the compact report crosses to the host.
salvage() the corpus with every damaged chunk set to `fill`; every other chunk was decoded and checked by SHA-256 (when the index
          holds digests: ScrubReport.digests_checked).
repair()  a new store: damaged records copied from replicas or re-encoded from source bytes, HEADER fields rewritten from the index,
          padding zeroed.  The input store is left untouched.

Records are numbered by their global slot (shard order, then slot order), as read_store numbers them.  The metadata (header, index,
chunk map, pointer records, remote_bases, pieces) is trusted but checked: an inconsistency is METADATA, never used silently.
read_store, StoreReader, gc, similarity and resume are unchanged: they still raise on a damaged store.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np
import torch

from . import ops
from .config import KIND_DELTA, KIND_FULL, KIND_POINTER, IngestConfig
from .manifest import Manifest, Store, merged_shards
from .read import MAX_DELTA_DEPTH_LOG2, dependency_order, to_device as _t

STRUCTURE, STREAM, DIGEST, DICTIONARY, HEADER, METADATA = 1, 2, 4, 8, 16, 32
DAMAGE = STRUCTURE | STREAM | DIGEST | DICTIONARY | METADATA
FLAG_NAMES = {STRUCTURE: "STRUCTURE", STREAM: "STREAM", DIGEST: "DIGEST", DICTIONARY: "DICTIONARY", HEADER: "HEADER", METADATA: "METADATA"}
ROOT_DTYPE = np.dtype([("slot", "<i8"), ("shard", "<i8"), ("local_slot", "<i8"), ("cause", "u1"), ("records", "<i8"), ("chunks", "<i8"),
                       ("bytes", "<i8")])
SIG_OK, SIG_BAD, SIG_UNCHECKED = 0, 1, 2
MAP_BAD = -2          # chunk root of an inconsistent map entry


def flag_names(f: int) -> str:
    return "|".join(n for b, n in FLAG_NAMES.items() if f & b) or "OK"


@dataclass
class ScrubReport:
    record_status: np.ndarray            # u8 [n_records] flags
    record_root: np.ndarray              # i64 [n_records], -1 good
    chunk_root: np.ndarray               # i64 [n_chunks] in corpus (stream) order: -1 good, -2 inconsistent map entry
    ranges: np.ndarray                   # i64 [r, 2] (offset, length) of the maximal runs of damaged chunks
    roots: np.ndarray                    # ROOT_DTYPE
    padding_bytes: int
    n_bytes: int
    shard_of_record: np.ndarray = field(repr=False, default=None)
    sidecar: dict | None = None          # {"usable", "tables_ok": [per shard], "sig_status": u8[n_records], "sig_bad", "sig_unchecked"}
    digests_checked: bool = True         # False: the index holds no SHA-256 (all zero), so no record can be DIGEST and nothing was verified

    @property
    def lossless(self) -> bool:
        return not bool((self.chunk_root != -1).any())

    @property
    def sidecar_ok(self) -> bool:
        s = self.sidecar
        return s is None or (all(s["usable"]) and all(s["tables_ok"]) and s["sig_bad"] == 0)

    @property
    def clean(self) -> bool:
        return self.lossless and not bool((self.record_status & HEADER).any()) and self.padding_bytes == 0 and self.sidecar_ok

    def damaged_records(self) -> np.ndarray:
        return np.nonzero(self.record_status & DAMAGE)[0]

    def summary(self) -> str:
        lost = int(self.ranges[:, 1].sum()) if len(self.ranges) else 0
        n_dmg = int(((self.record_status & DAMAGE) != 0).sum())
        head = (f"{'clean' if self.clean else 'lossless' if self.lossless else 'DAMAGED'}: {len(self.record_status)} records, "
                f"{n_dmg} damaged in {len(self.roots)} root(s); {int((self.chunk_root != -1).sum())} of {len(self.chunk_root)} chunks, "
                f"{lost} of {self.n_bytes} bytes in {len(self.ranges)} range(s) lost; "
                f"{int(((self.record_status & HEADER) != 0).sum())} HEADER record(s), {self.padding_bytes} non-zero padding byte(s)")
        if not self.digests_checked:
            head += "; SHA-256 NOT checked (the index holds no digests)"
        if self.sidecar is not None:
            s = self.sidecar
            head += (f"; sidecar: {sum(map(bool, s['usable']))}/{len(s['usable'])} usable, tables "
                     f"{'ok' if all(s['tables_ok']) else 'DIFFER'}, {s['sig_bad']} signature(s) differ, {s['sig_unchecked']} unchecked")
        lines = [head]
        for r in self.roots[:20]:
            where = "chunk map" if r["slot"] == MAP_BAD else f"record {r['slot']} (shard {r['shard']} slot {r['local_slot']})"
            lines.append(f"  {where}: {flag_names(int(r['cause']))}, {r['records']} record(s), {r['chunks']} chunk(s), {r['bytes']} bytes")
        if len(self.roots) > 20:
            lines.append(f"  ... {len(self.roots) - 20} more")
        return "\n".join(lines)


# ---- metadata: trusted but checked -------------------------------------------------------------------------------------------
def _shards(store) -> list:
    shards = merged_shards(store, "scrub", lenient=True)
    if any(m.pieces is not None for m in shards) and not all(m.pieces is not None for m in shards):
        raise ValueError("scrub: only some shards carry stream pieces")
    return shards


@dataclass
class _Plan:
    """Host-side view of a store's metadata, every record in global slot order."""
    shards: list
    shard_slot: np.ndarray        # i64 [S+1]
    shard_blob: np.ndarray        # i64 [S+1]
    rec_shard: np.ndarray         # u32 [n]
    lba: np.ndarray               # u32 [n]
    rec_len: np.ndarray           # u32 [n]
    rec_off: np.ndarray           # i64 [n] byte offset in the concatenated blob
    kind: np.ndarray              # u8 [n] (FULL for an unknown kind: METADATA)
    raw_len: np.ndarray           # i64 [n]
    remote: np.ndarray            # i64 [n]
    meta: np.ndarray              # u8 [n] METADATA flags
    sorted_lba: np.ndarray        # u32 [n]
    sorted_slot: np.ndarray       # u32 [n]
    sha: np.ndarray               # u8 [n, 32]
    chunk_slot: np.ndarray        # i64 [n_chunks] corpus order, -1 inconsistent entry
    chunk_len: np.ndarray         # i64 [n_chunks] corpus order
    perm: np.ndarray | None       # stream order -> (shard, local) chunk list

    @property
    def n(self) -> int:
        return len(self.lba)


def plan(store) -> _Plan:
    shards = _shards(store)
    S = len(shards)
    us = [len(m.index) for m in shards]
    sb = np.cumsum([0] + us).astype(np.int64)
    bb = np.cumsum([0] + [int(m.blob.size) for m in shards]).astype(np.int64)
    n = int(sb[-1])
    rec_shard = np.repeat(np.arange(S, dtype=np.uint32), us)
    cat = lambda f, dt: np.concatenate([f(m).astype(dt) for m in shards]) if S else np.zeros(0, dt)
    lba = cat(lambda m: m.index["lba"], np.uint32)
    rec_len = cat(lambda m: m.index["length"], np.uint32)
    unit = np.array([m.lba_unit for m in shards], np.int64)
    rec_off = bb[:-1][rec_shard] + lba.astype(np.int64) * unit[rec_shard] if n else np.zeros(0, np.int64)
    kind = np.zeros(n, np.uint8)
    raw_len = np.zeros(n, np.int64)
    meta = np.zeros(n, np.uint8)
    remote = np.full(n, -1, np.int64)
    sha = cat(lambda m: m.index["sha256"].reshape(-1, 32), np.uint8).reshape(-1, 32) if S else np.zeros((0, 32), np.uint8)
    chunk_slot, chunk_len = [], []
    for i, m in enumerate(shards):
        cm, u = m.chunk_map, us[i]
        ck, cs, csh = cm["kind"].astype(np.int64), cm["slot"].astype(np.int64), cm["shard"].astype(np.int64)
        own = ck != KIND_POINTER
        ok_own = own & (csh == i) & (cs < u) & ((ck == KIND_FULL) | (ck == KIND_DELTA))
        named = np.bincount(cs[ok_own], minlength=u)[:u] if u else np.zeros(0, np.int64)
        k_loc = np.zeros(u, np.uint8)
        r_loc = np.zeros(u, np.int64)
        k_loc[cs[ok_own]] = ck[ok_own]
        r_loc[cs[ok_own]] = cm["raw_length"][ok_own]
        bad_rec = named != 1                                   # a record no own chunk names, or several do
        kind[sb[i]: sb[i + 1]] = np.where(bad_rec, KIND_FULL, k_loc)
        raw_len[sb[i]: sb[i + 1]] = np.where(bad_rec, 0, r_loc)
        meta[sb[i]: sb[i + 1]] |= np.where(bad_rec, METADATA, 0).astype(np.uint8)
        g = np.full(len(cm), -1, np.int64)
        g[ok_own] = sb[i] + cs[ok_own]
        # POINTER entries: target in range, a stored record of the target shard, lengths and the pointer record agree
        pidx = np.nonzero(~own)[0]
        ts, tsl = csh[pidx], cs[pidx]
        okp = (ts < S) & (tsl < np.array(us + [0], np.int64)[np.minimum(ts, S)])
        tg = np.where(okp, sb[np.minimum(ts, S)] + tsl, 0)
        ptrs = m.pointers
        if len(ptrs) == len(pidx) and n:
            okp &= ptrs["target_lba"].astype(np.int64) == lba[tg]
            okp &= ptrs["target_length"].astype(np.int64) == rec_len[tg]
            okp &= ptrs["flags"].astype(np.int64) == (KIND_POINTER | (ts << 4))
        else:
            okp[:] = False
        g[pidx] = np.where(okp, tg, -1)
        chunk_slot.append(g)
        chunk_len.append(cm["raw_length"].astype(np.int64))
        if m.n_remote():
            rb = m.remote_bases
            rs, rsh, rbs = rb["slot"].astype(np.int64), rb["shard"].astype(np.int64), rb["base_slot"].astype(np.int64)
            okr = (rs < u) & (rsh < S) & (rsh != i) & (rbs < np.array(us + [0], np.int64)[np.minimum(rsh, S)])
            okr &= np.bincount(np.minimum(rs, u), minlength=u + 1)[np.minimum(rs, u)] == 1
            okr &= np.where(rs < u, kind[sb[i] + np.minimum(rs, max(u - 1, 0))] == KIND_DELTA, False) if u else False
            good = rs[okr]
            remote[sb[i] + good] = sb[rsh[okr]] + rbs[okr]
            bad = rs[~okr & (rs < u)]
            meta[sb[i] + bad] |= METADATA
    # the records of a shard do not overlap (in LBA order)
    sorted_lba = np.zeros(n, np.uint32)
    sorted_slot = np.zeros(n, np.uint32)
    for i in range(S):
        a, b = sb[i], sb[i + 1]
        order = np.argsort(lba[a:b], kind="stable")
        sorted_lba[a:b] = lba[a:b][order]
        sorted_slot[a:b] = order
        st = rec_off[a:b][order]
        en = st + rec_len[a:b][order]
        ov = np.nonzero(st[1:] < en[:-1])[0]
        meta[a + order[ov]] |= METADATA
        meta[a + order[ov + 1]] |= METADATA
    slot_g = np.concatenate(chunk_slot) if S else np.zeros(0, np.int64)
    lens = np.concatenate(chunk_len) if S else np.zeros(0, np.int64)
    # a chunk's raw_length must be its record's raw length (its own entry's, for a POINTER the target's own entry's, possibly on a
    # later shard): an entry that disagrees is inconsistent.  (A chunk of a METADATA record is damaged through the record already.)
    if n:
        ok_g = slot_g >= 0
        tg = np.maximum(slot_g, 0)
        slot_g = np.where(ok_g & (meta[tg] == 0) & (lens != raw_len[tg]), -1, slot_g)
    perm = None
    if S and shards[0].pieces is not None:
        g = np.concatenate([m.global_index() for m in shards])
        perm = np.argsort(g, kind="stable")
        if len(g) != len(slot_g) or not np.array_equal(g[perm], np.arange(len(g))):
            raise ValueError("scrub: the shards' stream pieces do not tile the stream (no chunk order: refused, not reported)")
        slot_g, lens = slot_g[perm], lens[perm]
    return _Plan(shards, sb, bb, rec_shard, lba, rec_len, rec_off, kind, raw_len, remote, meta, sorted_lba, sorted_slot, sha, slot_g, lens, perm)


def cut_deep(parent: np.ndarray, max_log2: int) -> np.ndarray:
    """Records 2^max_log2 or more links below the top of their dictionary chain — a chain that long, or one that never ends (a cycle
    through remote dictionaries, or a chain behind one): a boolean mask.  Cut as METADATA, the forest that is left has chains shorter
    than 2^max_log2 records, which read.dependency_order orders and hmse_scrub_attribute's max_log2 + 1 doubling rounds resolve.
    The doubling runs on the records that still have an ancestor only, so a store of short chains costs a few small passes."""
    n = len(parent)
    anc = np.where(parent >= 0, parent, n).astype(np.int64)
    anc = np.concatenate([anc, [n]])                        # the sentinel is its own ancestor
    live = np.nonzero(anc[:n] < n)[0]
    for _ in range(max_log2):                               # after round r: anc = the 2^(r+1)-th ancestor of the live records
        if not len(live):
            break
        anc[live] = anc[anc[live]]
        live = live[anc[live] < n]
    deep = np.zeros(n, bool)
    deep[live] = True
    return deep


# ---- the device pass ------------------------------------------------------------------------------------------------------------
def _records_pass(blob, p: _Plan, device):
    t = lambda a, dt: _t(a, dt, device)
    steps = int(max(np.diff(p.shard_slot).max(initial=0), 0)).bit_length()
    return ops.scrub_records(blob, t(p.rec_shard.view(np.int32), torch.int32), t(p.shard_blob, torch.int64), t(p.shard_slot, torch.int64),
                             t(np.array([m.lba_unit for m in p.shards], np.int32), torch.int32), t(p.lba.view(np.int32), torch.int32),
                             t(p.rec_len.view(np.int32), torch.int32), t(p.kind, torch.uint8), t(p.remote, torch.int64),
                             t(p.sorted_lba.view(np.int32), torch.int32), t(p.sorted_slot.view(np.int32), torch.int32), steps,
                             t(p.meta, torch.uint8))


@dataclass
class _Pass:
    plan: _Plan
    report: ScrubReport
    raw: torch.Tensor
    raw_off: torch.Tensor
    pos: np.ndarray               # decode position of every record (global slot -> row of raw_off)
    dicts: np.ndarray             # resolved dictionary of every record (hmse_scrub_records), -1 none


def _scrub_pass(store, device, cfg=None, band_tables=None, timings=None) -> _Pass:
    from .gc import _Clock
    clock = _Clock(timings)
    p = plan(store)
    clock.lap("plan")
    n, dev = p.n, device
    t = lambda a, dt: _t(a, dt, dev)
    blobs = [t(m.blob, torch.uint8) for m in p.shards if m.blob.size]
    blob = blobs[0] if len(blobs) == 1 else torch.cat(blobs) if blobs else torch.zeros(16, dtype=torch.uint8, device=dev)
    del blobs
    clock.lap("upload", int(blob.numel()))
    status, dict_, pad = _records_pass(blob, p, dev)
    clock.lap("scrub_records")
    st_h, d_h = status.cpu().numpy(), dict_.cpu().numpy()
    bad = (st_h & (STRUCTURE | METADATA)) != 0
    parent = np.where(bad, -1, d_h)
    cyc = cut_deep(parent, MAX_DELTA_DEPTH_LOG2)
    if cyc.any():                                         # a cycle, or a chain of 2^16 or more records: METADATA, cut from the forest
        st_h = st_h | np.where(cyc, METADATA, 0).astype(np.uint8)
        status = t(st_h, torch.uint8)
        bad |= cyc
        parent = np.where(bad, -1, d_h)
    dep = dependency_order(parent)
    order = np.arange(n) if dep is None else dep[0]
    pos = np.arange(n) if dep is None else dep[1]
    delta = (p.kind == KIND_DELTA) & ~bad
    base_dec = np.where(parent >= 0, pos[np.maximum(parent, 0)], -1)
    kind_dec = np.where(bad, KIND_DELTA, p.kind).astype(np.uint8)          # DELTA without a dictionary: rejected at once
    s_off = np.where(bad, 0, p.rec_off + 8 * delta)
    s_len = np.where(bad, 0, p.rec_len.astype(np.int64) - 8 * delta)
    raw_len = np.where(bad, 0, p.raw_len)
    clock.lap("decode_order")
    raw, raw_off, ok = ops.l1_inflate(blob, t(s_off[order], torch.int64), t(kind_dec[order], torch.uint8), t(base_dec[order], torch.int64),
                                      t(raw_len[order], torch.int64), stream_len=t(s_len[order], torch.int32), check=False)
    del blob
    clock.lap("inflate", int(raw.numel()))
    got = ops.l3_sha256(raw, raw_off) if n else torch.zeros((0, 32), dtype=torch.uint8, device=dev)
    clock.lap("sha256")
    pos_d = t(pos, torch.int64)
    ok_s, got_s = (ok, got) if dep is None else (ok[pos_d], got[pos_d])
    check_digest = bool(p.sha.any())
    want = t(p.sha, torch.uint8)
    cuts = torch.zeros(len(p.chunk_len) + 1, dtype=torch.int64, device=dev)
    if len(p.chunk_len):
        torch.cumsum(t(p.chunk_len, torch.int64), 0, out=cuts[1:])
    a = ops.scrub_attribute(status, dict_ if not cyc.any() else t(d_h, torch.int64), ok_s.contiguous(), got_s.contiguous(), want, check_digest,
                        t(p.chunk_slot, torch.int64), cuts, MAX_DELTA_DEPTH_LOG2)
    clock.lap("scrub_attribute")
    counts = [int(v) for v in torch.cat([a["counts"], pad]).tolist()]           # the one host read of the sizes
    n_rng = counts[0]
    rec_status = a["status"][:n].cpu().numpy()
    rec_root = a["root"][:n].cpu().numpy()
    chunk_root = a["chunk_root"][:len(p.chunk_len)].cpu().numpy()
    ranges = a["ranges"][:2 * n_rng].cpu().numpy().reshape(-1, 2).astype(np.int64)
    roots_g = np.nonzero(rec_root == np.arange(n))[0]
    rs = torch.from_numpy(roots_g).to(dev)
    rows = torch.stack([a["root_records"][rs], a["root_chunks"][rs], a["root_bytes"][rs]]).cpu().numpy() if len(roots_g) else np.zeros((3, 0), np.int64)
    roots = np.zeros(len(roots_g) + (1 if counts[4] else 0), ROOT_DTYPE)
    roots["slot"][:len(roots_g)] = roots_g
    roots["shard"][:len(roots_g)] = p.rec_shard[roots_g]
    roots["local_slot"][:len(roots_g)] = roots_g - p.shard_slot[p.rec_shard[roots_g].astype(np.int64)]
    roots["cause"][:len(roots_g)] = rec_status[roots_g] & DAMAGE
    roots["records"][:len(roots_g)], roots["chunks"][:len(roots_g)], roots["bytes"][:len(roots_g)] = rows
    if counts[4]:
        roots[-1] = (MAP_BAD, -1, -1, METADATA, 0, counts[4], counts[5])
    rep = ScrubReport(rec_status, rec_root, chunk_root, ranges, roots, counts[8], int(p.chunk_len.sum()), p.rec_shard,
                      digests_checked=check_digest or n == 0)
    clock.lap("report")
    if band_tables is not None:
        rep.sidecar = _check_sidecars(p, band_tables, cfg, rec_status, raw, raw_off, pos, dev)
        clock.lap("sidecar")
    return _Pass(p, rep, raw, raw_off, pos, np.where(bad, -1, d_h))


def _split_sidecar(buf: bytes):
    """-> (band-table section bytes, keys u32[n][bands], signatures u32[n][h], bands, band_bits) or None when unusable."""
    from . import bandtable
    try:
        tables, band_bits, keys, sig = bandtable.split_sidecar(buf)
    except (AssertionError, ValueError, struct.error):
        return None
    if sig is None or len(buf) != len(tables) + 12 + keys.nbytes + sig.nbytes:
        return None
    return tables, keys, sig, keys.shape[1], band_bits


def _check_sidecars(p: _Plan, band_tables, cfg: IngestConfig, rec_status, raw, raw_off, pos, dev) -> dict:
    S, n = len(p.shards), p.n
    sig_status = np.full(n, SIG_UNCHECKED, np.uint8)
    usable, tables_ok = [False] * S, [False] * S
    for i in range(S):
        parsed = _split_sidecar(bytes(band_tables[i]))
        a, b = int(p.shard_slot[i]), int(p.shard_slot[i + 1])
        if parsed is None:
            continue
        tables, keys, sig, bands, band_bits = parsed
        if len(keys) != b - a or bands != cfg.bands or sig.shape[1] != cfg.n_hashes:
            continue
        usable[i] = True
        keys_d = _t(keys.view(np.int32), torch.int32, dev)
        tables_ok[i] = ops.band_tables_write(keys_d, None, cfg.band_bits).cpu().numpy().tobytes() == tables
        good = np.nonzero((rec_status[a:b] & DAMAGE) == 0)[0]
        if len(good):
            ids = _t(pos[a + good], torch.int64, dev)
            sg = ops.l4_minhash(raw, raw_off, cfg, chunk_ids=ids)
            kg, _ = ops.l4_lsh(sg, cfg)
            g = _t(good, torch.int64, dev)
            same = (sg == _t(sig.view(np.int32), torch.int32, dev)[g]).all(dim=1) & (kg == keys_d[g]).all(dim=1)
            sig_status[a + good] = np.where(same.cpu().numpy(), SIG_OK, SIG_BAD)
    return {"usable": usable, "tables_ok": tables_ok, "sig_status": sig_status, "sig_bad": int((sig_status == SIG_BAD).sum()),
            "sig_unchecked": int((sig_status == SIG_UNCHECKED).sum())}


# ---- public API ----------------------------------------------------------------------------------------------------------------
def _check_args(store, cfg, band_tables):
    shards = _shards(store)
    if band_tables is not None:
        if cfg is None:
            raise ValueError("scrub: checking a band-table sidecar needs the store's IngestConfig (cfg)")
        if any(m.pieces is not None for m in shards):
            raise ValueError("scrub: sidecars of multi-rank stream stores (pieces) are not checked")
        if len(band_tables) != len(shards):
            raise ValueError(f"scrub: one sidecar per shard ({len(shards)}), got {len(band_tables)}")
    return shards


def scrub(store, device, cfg: IngestConfig | None = None, band_tables=None, timings=None) -> ScrubReport:
    """Which records, chunks and byte ranges of `store` (a Manifest or a merged Store) are intact -> ScrubReport.  Never raises on
    damage; refuses (ValueError) unmerged parts, unresolved pointers and stream pieces that do not tile the stream (then the store has
    no chunk order to report in).  `band_tables`: one sidecar per shard, checked under `cfg`.  `timings` (a dict, diagnostics): filled
    with per-phase milliseconds (synchronising between phases)."""
    _check_args(store, cfg, band_tables)
    return _scrub_pass(store, device, cfg, band_tables, timings).report


def salvage(store, device, report: ScrubReport | None = None, fill: int = 0):
    """-> (the corpus as a uint8 tensor on `device` with every damaged chunk's bytes set to `fill`, ScrubReport).  Every chunk returned
    as good was decoded in this call and, when the index holds digests (report.digests_checked), checked by SHA-256.  A `report` of an
    earlier scrub adds its damaged chunks to this call's."""
    if not 0 <= int(fill) <= 255:
        raise ValueError("salvage: fill is a byte value")
    _check_args(store, None, None)
    ps = _scrub_pass(store, device)
    rep, p = ps.report, ps.plan
    dmg = rep.chunk_root != -1
    if report is not None:
        if report.chunk_root.shape != rep.chunk_root.shape or report.record_status.shape != rep.record_status.shape:
            raise ValueError("salvage: the report is not a scrub of this store")
        dmg |= report.chunk_root != -1
    nc = len(p.chunk_len)
    dev = device
    cuts = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    if nc:
        torch.cumsum(_t(p.chunk_len, torch.int64, dev), 0, out=cuts[1:])
    n_bytes = int(p.chunk_len.sum())
    if n_bytes == 0:
        return torch.zeros(0, dtype=torch.uint8, device=dev), rep
    # a damaged chunk takes its bytes from a fill block appended to the decoded records: one extra slot pair per damaged chunk,
    # [F, F + len) — the assembly kernel reads slot s as [raw_off[s], raw_off[s + 1])
    F = ps.raw.numel()
    maxlen = int(p.chunk_len.max())
    raw_ext = torch.cat([ps.raw, torch.full((maxlen,), int(fill), dtype=torch.uint8, device=dev)])
    d = np.nonzero(dmg)[0]
    extra = np.empty(2 * len(d), np.int64)
    extra[0::2] = F
    extra[1::2] = F + p.chunk_len[d]
    raw_off_ext = torch.cat([ps.raw_off, _t(extra, torch.int64, dev)])
    n_dec = ps.raw_off.numel() - 1
    slot = np.where(dmg, 0, ps.pos[np.maximum(p.chunk_slot, 0)] if p.n else 0).astype(np.int64)
    slot[d] = n_dec + 1 + 2 * np.arange(len(d))
    data = ops.read_assemble(cuts, _t(slot, torch.int64, dev), raw_off_ext, raw_ext)
    if report is not None and not np.array_equal(dmg, rep.chunk_root != -1):
        # the chunks an earlier report named as damaged are added; the ranges are recomputed on the host
        c = np.concatenate([[0], np.cumsum(p.chunk_len)])
        e = np.diff(np.concatenate([[0], dmg.astype(np.int8), [0]]))
        st, en = np.nonzero(e == 1)[0], np.nonzero(e == -1)[0]
        rep = ScrubReport(rep.record_status, rep.record_root, np.where(rep.chunk_root != -1, rep.chunk_root, report.chunk_root),
                          np.stack([c[st], c[en] - c[st]], 1).astype(np.int64).reshape(-1, 2), rep.roots, rep.padding_bytes, rep.n_bytes,
                          rep.shard_of_record, rep.sidecar, rep.digests_checked)
    return data, rep


def _copy_records(dst: list, p: _Plan, recs: np.ndarray, src: list) -> None:
    for k in recs:
        s = int(p.rec_shard[k])
        o = int(p.rec_off[k] - p.shard_blob[s])
        dst[s][o: o + int(p.rec_len[k])] = src[s][o: o + int(p.rec_len[k])]


def _fix_headers(blobs: list, p: _Plan, recs: np.ndarray, dict_: np.ndarray) -> None:
    """Rewrite delta_length and, where the dictionary is resolved, base_length of the DELTA records `recs` from the index."""
    for k in recs:
        s = int(p.rec_shard[k])
        o = int(p.rec_off[k] - p.shard_blob[s])
        d = int(dict_[k])
        if d >= 0:
            blobs[s][o + 4: o + 6] = np.frombuffer(struct.pack("<H", int(p.rec_len[d]) & 0xFFFF), np.uint8)
        blobs[s][o + 6: o + 8] = np.frombuffer(struct.pack("<H", (int(p.rec_len[k]) - 8) & 0xFFFF), np.uint8)


def _zero_padding(blobs: list, p: _Plan) -> None:
    for s, m in enumerate(p.shards):
        a, b = int(p.shard_slot[s]), int(p.shard_slot[s + 1])
        if b == a:
            blobs[s][:] = 0
            continue
        order = np.argsort(p.lba[a:b], kind="stable")
        st = (p.rec_off[a:b] - p.shard_blob[s])[order]
        en = st + p.rec_len[a:b][order]
        gaps = np.stack([np.concatenate([[0], en]), np.concatenate([st, [m.blob.size]])], 1)
        for g0, g1 in gaps[gaps[:, 1] > gaps[:, 0]]:
            blobs[s][max(int(g0), 0): min(int(g1), m.blob.size)] = 0


def _rebuild(p: _Plan, blobs: list) -> Store:
    return Store([Manifest(m.lba_unit, m.index, m.chunk_map, m.pointers, b, m.shard, m.n_shards, m.chunk_base, m.remote_bases, m.pieces)
                  for m, b in zip(p.shards, blobs)])


def _same_metadata(a: Manifest, b: Manifest) -> bool:
    eq = lambda x, y: (x is None and y is None) or (x is not None and y is not None and x.tobytes() == y.tobytes())
    return (a.lba_unit == b.lba_unit and a.shard == b.shard and a.n_shards == b.n_shards and a.chunk_base == b.chunk_base
            and a.blob.size == b.blob.size and eq(a.index, b.index) and eq(a.chunk_map, b.chunk_map) and eq(a.pointers, b.pointers)
            and eq(a.remote_bases, b.remote_bases) and eq(a.pieces, b.pieces))


def repair(store, device, cfg: IngestConfig | None = None, replicas=(), sources=None):
    """-> (a new Store with every repairable damaged record restored, the scrub of that store).  The input is left untouched.
    `replicas`: other copies of the store with identical metadata — a damaged record is copied from the first replica whose bytes for
    it decode and verify in the repaired store (rounds until no more are accepted).
    `sources`: [(offset, bytes)] of original corpus bytes — a damaged root (FULL, or DELTA with a good header) with a chunk inside them
    whose SHA-256 matches is re-encoded by ops.l1_deflate; only a record of exactly the stored kind and length is accepted.
    HEADER fields are rewritten from the index and padding is zeroed."""
    shards = _check_args(store, cfg, None)
    if sources is not None and cfg is None:
        raise ValueError("repair: re-encoding from sources needs the store's IngestConfig (cfg)")
    reps = []
    for r in replicas:
        rs = _shards(r)
        if len(rs) != len(shards) or not all(_same_metadata(a, b) for a, b in zip(shards, rs)):
            raise ValueError("repair: a replica's metadata differs from the store's")
        reps.append(r)
    ps = _scrub_pass(store, device)
    p, rep = ps.plan, ps.report
    blobs = [m.blob.copy() for m in p.shards]
    need = ((rep.record_status & DAMAGE) != 0) & ((rep.record_status & METADATA) == 0)
    need0 = need.copy()
    # replicas: a still-damaged record takes the first replica's bytes that decode and verify IN PLACE (its dictionary may be a record
    # that only this store holds intact); a candidate that does not verify is put back.  Rounds until nothing more is accepted.
    rsh = [_shards(r) for r in reps]
    progress = True
    while reps and need.any() and progress:
        progress = False
        for shards_r in rsh:
            cand = np.nonzero(need)[0]
            if not len(cand):
                break
            trial = [b.copy() for b in blobs]
            _copy_records(trial, p, cand, [m.blob for m in shards_r])
            good = (_scrub_pass(_rebuild(p, trial), device).report.record_status[cand] & DAMAGE) == 0
            if good.any():
                _copy_records(blobs, p, cand[good], [m.blob for m in shards_r])
                need[cand[good]] = False
                progress = True
    if sources is not None and need.any():
        _repair_from_sources(p, rep, ps, blobs, need, sources, cfg, device)
    # HEADER: rewrite base_length / delta_length from the index wherever the structure (base_lba) is good
    st2 = ps if np.array_equal(need, need0) else _scrub_pass(_rebuild(p, blobs), device)
    hdr = np.nonzero((st2.report.record_status & HEADER) != 0)[0]
    _fix_headers(blobs, p, hdr, st2.dicts)
    if st2.report.padding_bytes:
        _zero_padding(blobs, p)
    out = _rebuild(p, blobs)
    return out, scrub(out, device)


def _repair_from_sources(p: _Plan, rep: ScrubReport, ps: _Pass, blobs: list, need: np.ndarray, sources, cfg: IngestConfig, dev) -> None:
    import hashlib
    roots = np.nonzero(need & (rep.record_root == np.arange(p.n)))[0]
    if not len(roots):
        return
    cuts = np.concatenate([[0], np.cumsum(p.chunk_len)])
    src = [(int(o), np.frombuffer(bytes(b), np.uint8)) for o, b in sources]
    dicts = ps.dicts
    jobs = []                                              # (record, chunk bytes, dictionary bytes or None)
    by_slot = {}
    for c in np.nonzero(np.isin(p.chunk_slot, roots))[0]:
        by_slot.setdefault(int(p.chunk_slot[c]), []).append(int(c))
    for k in roots:
        k = int(k)
        if rep.record_status[k] & (METADATA | STRUCTURE):
            continue                                       # a DELTA root with an unreadable header is not re-encoded from sources alone
        chunk = None
        for c in by_slot.get(k, []):
            a, b = int(cuts[c]), int(cuts[c + 1])
            for o, buf in src:
                if o <= a and b <= o + buf.size:
                    cand = buf[a - o: b - o]
                    if hashlib.sha256(cand.tobytes()).digest() == p.sha[k].tobytes():
                        chunk = cand
                        break
            if chunk is not None:
                break
        if chunk is None:
            continue
        dbytes = None
        if p.kind[k] == KIND_DELTA:
            d = int(dicts[k])
            if d < 0:
                continue
            q = int(ps.pos[d])
            dbytes = ps.raw[int(ps.raw_off[q]): int(ps.raw_off[q + 1])].cpu().numpy()
        jobs.append((k, chunk, dbytes, int(dicts[k]) if dbytes is not None else -1))
    if not jobs:
        return
    parts, ids, base, run = [], [], [], 0
    bounds = [0]
    for k, chunk, dbytes, d in jobs:
        if dbytes is not None:
            parts.append(dbytes); run += dbytes.size; bounds.append(run)
            base.append(len(bounds) - 2)
        else:
            base.append(-1)
        parts.append(chunk); run += chunk.size; bounds.append(run)
        ids.append(len(bounds) - 2)
    data = _t(np.concatenate(parts), torch.uint8, dev)
    cuts_d = _t(np.array(bounds, np.int64), torch.int64, dev)
    out, off, kind = ops.l1_deflate(data, cuts_d, cfg, _t(np.array(ids, np.int64), torch.int64, dev), _t(np.array(base, np.int64), torch.int64, dev),
                                    base_is_chunk_id=True)
    out, off, kind = out.cpu().numpy(), off.cpu().numpy(), kind.cpu().numpy()
    for j, (k, chunk, dbytes, d) in enumerate(jobs):
        stream = out[off[j]: off[j + 1]]
        want_kind = int(p.kind[k])
        rec = stream if want_kind == KIND_FULL else np.concatenate(
            [np.frombuffer(struct.pack("<IHH", int(p.lba[d]), int(p.rec_len[d]) & 0xFFFF, (int(p.rec_len[k]) - 8) & 0xFFFF), np.uint8), stream])
        if int(kind[j]) != want_kind or rec.size != int(p.rec_len[k]):
            continue                                        # not the stored kind and length: left as it is (unrepairable)
        s = int(p.rec_shard[k])
        o = int(p.rec_off[k] - p.shard_blob[s])
        blobs[s][o: o + rec.size] = rec
        need[k] = False
