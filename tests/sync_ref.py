"""Plain Python + numpy restatement of replication (hmse_amd/sync.py): the CHECKER of the match kernel, of diff, of the patch plan
(a digest dictionary plus `bytes ==`) and of apply (slice assignment).  TEST INFRASTRUCTURE — the product compares and copies on the GPU."""
import dataclasses
import struct

import numpy as np

from hmse_amd.config import KIND_DELTA, KIND_POINTER
from hmse_amd.manifest import DELTA_HDR_DTYPE, Manifest, Store, stream_order


def shards_of(store):
    return list(store.shards) if isinstance(store, Store) else [store]


# ---- the match kernel -----------------------------------------------------------------------------------------------------------------
def match(a, a_off, a_len, b, b_off, b_len, cand):
    """-> (same list of 0 / 1, status): include/hmse.h hmse_sync_match, record by record."""
    a, b = bytes(a), bytes(b)
    same, status = [], 0
    for k, c in enumerate(cand):
        c = int(c)
        if c < 0:
            same.append(0)
            continue
        if c >= len(b_off):
            same.append(0); status |= 1
            continue
        ao, al, bo, bl = int(a_off[k]) & (2**64 - 1), int(a_len[k]) & (2**32 - 1), int(b_off[c]) & (2**64 - 1), int(b_len[c]) & (2**32 - 1)   # (u64 / u32 of the C-ABI)
        if ao > len(a) or al > len(a) - ao or bo > len(b) or bl > len(b) - bo:
            same.append(0); status |= 1
            continue
        same.append(int(al == bl and a[ao:ao + al] == b[bo:bo + bl]))
    return same, status


# ---- records of a store ---------------------------------------------------------------------------------------------------------------
def records(store):
    """Every record in (shard, slot) order: dicts with sha (bytes), kind, pos (the stream's byte position in the shards' blobs
    concatenated), stream (bytes), hdr (the 8 DeltaChunk header bytes or b""), raw_len."""
    out, blob_base = [], 0
    for m in shards_of(store):
        kind = np.zeros(len(m.index), np.uint8)
        raw_len = np.zeros(len(m.index), np.int64)
        for c in m.chunk_map:
            if c["kind"] != KIND_POINTER:
                kind[c["slot"]] = c["kind"]; raw_len[c["slot"]] = c["raw_length"]
        for s, e in enumerate(m.index):
            o, ln = int(e["lba"]) * m.lba_unit, int(e["length"])
            h = 8 if kind[s] == KIND_DELTA else 0
            out.append({"sha": e["sha256"].tobytes(), "kind": int(kind[s]), "pos": blob_base + o + h, "stream": m.blob[o + h:o + ln].tobytes(),
                        "hdr": m.blob[o:o + h].tobytes(), "raw_len": int(raw_len[s]), "off": o, "len": ln})
        blob_base += int(m.blob.size)
    return out


def chunks(store):
    """The chunks in corpus order: (sha, raw_length) each."""
    sh = shards_of(store)
    lst = [(sh[int(c["shard"]) if len(sh) > 1 else 0].index["sha256"][int(c["slot"])].tobytes(), int(c["raw_length"])) for m in sh for c in m.chunk_map]
    perm = stream_order(sh)
    return lst if perm is None else [lst[int(i)] for i in perm]


# ---- diff -----------------------------------------------------------------------------------------------------------------------------
def diff(have, want):
    have_sha = {r["sha"] for r in records(have)}
    ch = chunks(want)
    want_sha = {s for s, _ in ch}
    present = np.array([s in have_sha for s, _ in ch], bool)
    ranges, o = [], 0
    for (s, ln), p in zip(ch, present):
        if not p and ln:
            if ranges and ranges[-1][0] + ranges[-1][1] == o:
                ranges[-1][1] += ln
            else:
                ranges.append([o, ln])
        o += ln
    new_bytes = sum(ln for (s, ln), p in zip(ch, present) if not p)
    uniq = {}
    for (s, ln), p in zip(ch, present):
        if not p:
            uniq[s] = ln
    return {"present": present, "new_ranges": np.array(ranges, np.int64).reshape(-1, 2), "shared_bytes": o - new_bytes, "new_bytes": new_bytes,
            "new_unique_bytes": sum(uniq.values()),
            "unreferenced": np.array([i for i, r in enumerate(records(have)) if r["sha"] not in want_sha], np.int64)}


# ---- the patch plan -------------------------------------------------------------------------------------------------------------------
def plan(have, want, digest_only=False):
    """Per record of want (one shard), in slot order: src = the byte position of the first record of have with its digest whose stored
    stream is `==`, else -1; the literal streams back to back; the DeltaChunk headers in slot order.  digest_only: copy on digest
    equality alone (what a plan without the byte proof would do)."""
    by_sha = {}
    for r in records(have):
        by_sha.setdefault(r["sha"], r)
    src, lit, hdrs, cls = [], [], [], []
    for r in records(want):
        h = by_sha.get(r["sha"])
        ok = h is not None and (digest_only or h["stream"] == r["stream"])
        cls.append("absent" if h is None else "same" if h["stream"] == r["stream"] else "differs")
        src.append(h["pos"] if ok else -1)
        if not ok:
            lit.append(r["stream"])
        if r["kind"] == KIND_DELTA:
            hdrs.append(r["hdr"])
    return {"src": np.array(src, np.int64), "literals": np.frombuffer(b"".join(lit), np.uint8), "class": cls,
            "delta_hdrs": np.frombuffer(b"".join(hdrs), np.uint8).reshape(-1, 8)}


def apply(have, want_empty: Manifest, blob_size, src, literals, delta_hdrs) -> Manifest:
    """Slice assignment: want's blob from have's blobs (concatenated in shard order), the literals and the headers.  `want_empty` is
    want's manifest with an empty blob; src may copy streams that are NOT the wanted bytes (a digest-only plan): it is applied as is."""
    cat = np.concatenate([m.blob for m in shards_of(have)] + [np.zeros(0, np.uint8)])
    blob = np.zeros(int(blob_size), np.uint8)
    kind = np.zeros(len(want_empty.index), np.uint8)
    for c in want_empty.chunk_map:
        if c["kind"] != KIND_POINTER:
            kind[c["slot"]] = c["kind"]
    lo, d = 0, 0
    for s, e in enumerate(want_empty.index):
        o, ln = int(e["lba"]) * want_empty.lba_unit, int(e["length"])
        if kind[s] == KIND_DELTA:
            blob[o:o + 8] = delta_hdrs[d]; d += 1; o += 8; ln -= 8
        if src[s] < 0:
            blob[o:o + ln] = literals[lo:lo + ln]; lo += ln
        else:
            blob[o:o + ln] = cat[int(src[s]):int(src[s]) + ln]
    return dataclasses.replace(want_empty, blob=blob)


def gather(src0, src1, src_off, src_sel, dst_off):
    """hmse_record_gather in slices: the piece table of sync.plan_pieces applied on the host."""
    out = np.full(int(dst_off[-1]), 0xEE, np.uint8)                    # every byte must come from a piece
    for k in range(len(src_off)):
        n = int(dst_off[k + 1] - dst_off[k])
        s = src1 if src_sel[k] else src0
        assert 0 <= int(src_off[k]) and int(src_off[k]) + n <= len(s)
        out[int(dst_off[k]):int(dst_off[k]) + n] = s[int(src_off[k]):int(src_off[k]) + n]
    return out


# ---- the same store with padding ------------------------------------------------------------------------------------------------------
def relay(m: Manifest, unit: int = 512) -> Manifest:
    """A one-shard manifest re-laid at lba_unit = `unit`: records moved to aligned offsets (zero padding between them), index,
    DeltaChunk and pointer LBAs rewritten.  The only cheap way to a store with padding (the packer pads blobs beyond 4 GiB only)."""
    assert m.n_remote() == 0
    ln = m.index["length"].astype(np.int64)
    old = m.index["lba"].astype(np.int64) * m.lba_unit
    new = np.concatenate([[0], np.cumsum((ln + unit - 1) // unit * unit)])
    blob = np.zeros(int(new[-1]), np.uint8)
    new_lba = {int(l): int(o // unit) for l, o in zip(m.index["lba"], new[:-1])}
    kind = np.zeros(len(m.index), np.uint8)
    for c in m.chunk_map:
        if c["kind"] != KIND_POINTER:
            kind[c["slot"]] = c["kind"]
    for s in range(len(m.index)):
        rec = m.blob[int(old[s]):int(old[s] + ln[s])].copy()
        if kind[s] == KIND_DELTA:
            h = np.frombuffer(rec[:8].tobytes(), DELTA_HDR_DTYPE).copy()
            h["base_lba"] = new_lba[int(h["base_lba"][0])]
            rec[:8] = np.frombuffer(h.tobytes(), np.uint8)
        blob[int(new[s]):int(new[s] + ln[s])] = rec
    index, ptr = m.index.copy(), m.pointers.copy()
    index["lba"] = new[:-1] // unit
    ptr["target_lba"] = [new_lba[int(l)] for l in ptr["target_lba"]]
    return dataclasses.replace(m, lba_unit=unit, index=index, pointers=ptr, blob=blob)


def header_size() -> int:
    return 8 + struct.calcsize("<I32sQQQQQ")
