"""Host reference of hmse_amd.scrub (TEST INFRASTRUCTURE): DeltaChunk headers parsed tolerantly in Python, records decoded with stock
zlib (raw DEFLATE, zdict = the dictionary's bytes), SHA-256 by hashlib, the same attribution, roots and ranges by plain walks.
The metadata checks (METADATA flags, kinds, raw lengths, chunk slots, remote dictionaries, stream order, the depth cut) are written
here again as plain per-entry loops; only the record layout (offsets, lengths, digests in global slot order) comes from scrub.plan."""
import hashlib
import struct
import zlib

import numpy as np

from hmse_amd import scrub as S
from hmse_amd.config import KIND_DELTA, KIND_FULL, KIND_POINTER
from hmse_amd.read import MAX_DELTA_DEPTH_LOG2, dependency_order


def metadata(p):
    """-> (meta flags, kind, raw_len, remote, chunk_slot in corpus order, chunk_len in corpus order), one entry at a time."""
    shards, n = p.shards, p.n
    sb = [int(x) for x in p.shard_slot]
    us = [len(m.index) for m in shards]
    meta = np.zeros(n, np.int64); kind = np.zeros(n, np.uint8); raw_len = np.zeros(n, np.int64); remote = np.full(n, -1, np.int64)
    slots, lens = [], []
    named = [dict() for _ in shards]
    for i, m in enumerate(shards):
        for c in m.chunk_map:
            if int(c["kind"]) != KIND_POINTER and int(c["shard"]) == i and int(c["slot"]) < us[i] and int(c["kind"]) in (KIND_FULL, KIND_DELTA):
                named[i].setdefault(int(c["slot"]), []).append(c)
    for i in range(len(shards)):
        for j in range(us[i]):
            e = named[i].get(j, [])
            if len(e) == 1:
                kind[sb[i] + j] = int(e[0]["kind"]); raw_len[sb[i] + j] = int(e[0]["raw_length"])
            else:
                meta[sb[i] + j] |= S.METADATA
    for i, m in enumerate(shards):
        n_ptr = int((m.chunk_map["kind"] == KIND_POINTER).sum())
        q = 0
        for c in m.chunk_map:
            ck, cs, csh = int(c["kind"]), int(c["slot"]), int(c["shard"])
            g = -1
            if ck != KIND_POINTER:
                if csh == i and cs < us[i] and ck in (KIND_FULL, KIND_DELTA):
                    g = sb[i] + cs
            else:
                if csh < len(shards) and cs < us[csh] and len(m.pointers) == n_ptr:
                    t, pr = sb[csh] + cs, m.pointers[q]
                    if (int(pr["target_lba"]) == int(p.lba[t]) and int(pr["target_length"]) == int(p.rec_len[t])
                            and int(pr["flags"]) == (KIND_POINTER | (csh << 4))):
                        g = t
                q += 1
            slots.append(g); lens.append(int(c["raw_length"]))
        if m.remote_bases is not None:
            rows = [(int(r["slot"]), int(r["shard"]), int(r["base_slot"])) for r in m.remote_bases]
            for sl, sh, bs in rows:
                good = (sl < us[i] and sh < len(shards) and sh != i and bs < us[sh] and sum(1 for x in rows if x[0] == sl) == 1
                        and kind[sb[i] + sl] == KIND_DELTA)
                if good:
                    remote[sb[i] + sl] = sb[sh] + bs
                elif sl < us[i]:
                    meta[sb[i] + sl] |= S.METADATA
    for i, m in enumerate(shards):                                     # overlapping records, in LBA order
        recs = sorted(range(us[i]), key=lambda j: (int(p.lba[sb[i] + j]), j))
        for a, b in zip(recs, recs[1:]):
            if int(p.rec_off[sb[i] + b]) < int(p.rec_off[sb[i] + a]) + int(p.rec_len[sb[i] + a]):
                meta[sb[i] + a] |= S.METADATA; meta[sb[i] + b] |= S.METADATA
    for k, g in enumerate(slots):                                      # a chunk's raw_length is its record's raw length
        if g >= 0 and not meta[g] and lens[k] != raw_len[g]:
            slots[k] = -1
    slots, lens = np.array(slots, np.int64), np.array(lens, np.int64)
    if shards and shards[0].pieces is not None:
        order = {}
        pos = 0
        for m in shards:
            for pc in m.pieces:
                for x in range(int(pc["n"])):
                    order[int(pc["g0"]) + x] = pos; pos += 1
        perm = np.array([order[x] for x in range(pos)], np.int64)
        slots, lens = slots[perm], lens[perm]
    return meta, kind, raw_len, remote, slots, lens


def deep(parent: np.ndarray, limit: int) -> np.ndarray:
    """Records `limit` or more links below the top of their chain, or on / behind a cycle (iterative walk with memoised depths)."""
    n = len(parent)
    depth = np.full(n, -1, np.int64)                                   # -1 unknown; >= limit or a cycle: cut
    INF = 1 << 62
    for k in range(n):
        path = []
        j = k
        on = set()
        while j >= 0 and depth[j] < 0 and j not in on:
            on.add(j); path.append(j); j = int(parent[j])
        base = INF if (j >= 0 and j in on) else (-1 if j < 0 else int(depth[j]))
        for x in reversed(path):
            base = INF if base >= INF else base + 1
            depth[x] = base
    return depth >= limit


def _inflate(stream: bytes, raw_len: int, zdict: bytes | None):
    try:
        d = zlib.decompressobj(-15, zdict=zdict) if zdict is not None else zlib.decompressobj(-15)
        out = d.decompress(stream, raw_len + 1)
        if len(out) > raw_len or d.unconsumed_tail:
            return None
        out += d.flush()
        if not d.eof or d.unused_data or len(out) != raw_len:
            return None
        return out
    except zlib.error:
        return None


def scrub_ref(store) -> dict:
    p = S.plan(store)
    n = p.n
    meta, kind, raw_len, remote, chunk_slot, chunk_len = metadata(p)
    blob = np.concatenate([m.blob for m in p.shards]) if p.shards else np.zeros(0, np.uint8)
    status = meta.copy()
    dicts = np.full(n, -1, np.int64)
    lba_of = []
    for s in range(len(p.shards)):
        a, b = int(p.shard_slot[s]), int(p.shard_slot[s + 1])
        mp = {}
        order = np.argsort(p.lba[a:b], kind="stable")
        for j in order[::-1]:
            mp[int(p.lba[a + j])] = int(j)          # (reversed: of equal LBAs the first in stable sorted order wins)
        lba_of.append(mp)
    pad = 0
    for k in range(n):
        s = int(p.rec_shard[k])
        b1 = int(p.shard_blob[s + 1])
        o, L = int(p.rec_off[k]), int(p.rec_len[k])
        if o + L > b1:
            status[k] |= S.STRUCTURE
        elif kind[k] == KIND_DELTA and not status[k] & S.METADATA:
            if L < 8:
                status[k] |= S.STRUCTURE
                continue
            base_lba, base_len, dlen = struct.unpack("<IHH", blob[o:o + 8].tobytes())
            r = int(remote[k])
            ds = int(p.rec_shard[r]) if r >= 0 else s
            j = lba_of[ds].get(base_lba)
            g = None if j is None else int(p.shard_slot[ds]) + j
            if g is None or (g != r if r >= 0 else g >= k):
                status[k] |= S.STRUCTURE
            else:
                dicts[k] = g
                if base_len != int(p.rec_len[g]) & 0xFFFF:
                    status[k] |= S.HEADER
            if dlen != (L - 8) & 0xFFFF:
                status[k] |= S.HEADER
    for s, m in enumerate(p.shards):
        a, b = int(p.shard_slot[s]), int(p.shard_slot[s + 1])
        order = np.argsort(p.lba[a:b], kind="stable")
        st = (p.rec_off[a:b] - p.shard_blob[s])[order]
        en = st + p.rec_len[a:b][order]
        if not len(en):
            pad += int((m.blob != 0).sum())                        # a shard without records: its whole blob is padding
            continue
        edges = list(zip(np.concatenate([[0], en[:-1]]), st)) + [(int(en[-1]), m.blob.size)]
        for g0, g1 in edges:
            g0, g1 = int(g0), min(int(g1), m.blob.size)
            if g1 > g0:
                pad += int((m.blob[g0:g1] != 0).sum())
    bad = (status & (S.STRUCTURE | S.METADATA)) != 0
    parent = np.where(bad, -1, dicts)
    cyc = deep(parent, 1 << MAX_DELTA_DEPTH_LOG2)
    status |= np.where(cyc, S.METADATA, 0)
    bad |= cyc
    parent = np.where(bad, -1, dicts)
    dep = dependency_order(parent)
    order = range(n) if dep is None else dep[0]
    raw = [None] * n
    ok = np.zeros(n, bool)
    for k in order:
        k = int(k)
        if bad[k]:
            continue
        o, L = int(p.rec_off[k]), int(p.rec_len[k])
        zd = None
        if kind[k] == KIND_DELTA:
            if parent[k] < 0 or raw[parent[k]] is None:
                continue
            zd = raw[parent[k]]
            o, L = o + 8, L - 8
        raw[k] = _inflate(blob[o:o + L].tobytes(), int(raw_len[k]), zd)
        ok[k] = raw[k] is not None
    check = bool(p.sha.any())
    fault = np.zeros(n, np.int64)
    for k in range(n):
        if bad[k]:
            fault[k] = status[k] & (S.STRUCTURE | S.METADATA)
        elif not ok[k]:
            fault[k] = S.STREAM
        elif check and hashlib.sha256(raw[k]).digest() != p.sha[k].tobytes():
            fault[k] = S.DIGEST
    root = np.full(n, -1, np.int64)
    final = (status & S.HEADER).astype(np.int64)
    for k in range(n):
        far, j = -1, k
        while j >= 0:
            if fault[j]:
                far = j
            j = int(parent[j])
        root[k] = far
        if far == k:
            final[k] |= fault[k]
        elif far >= 0:
            final[k] |= S.DICTIONARY
    chunk_root = np.array([-2 if s < 0 else root[s] for s in chunk_slot], np.int64)
    cuts = np.concatenate([[0], np.cumsum(chunk_len)]).astype(np.int64)
    dmg = chunk_root != -1
    e = np.diff(np.concatenate([[0], dmg.astype(np.int8), [0]]))
    st, en = np.nonzero(e == 1)[0], np.nonzero(e == -1)[0]
    ranges = np.stack([cuts[st], cuts[en] - cuts[st]], 1).astype(np.int64).reshape(-1, 2)
    roots = {}
    for k in range(n):
        if root[k] >= 0:
            roots.setdefault(int(root[k]), [0, 0, 0])[0] += 1
    for c, r in enumerate(chunk_root):
        if r != -1:
            v = roots.setdefault(int(r), [0, 0, 0])
            v[1] += 1
            v[2] += int(cuts[c + 1] - cuts[c])
    return {"record_status": final.astype(np.uint8), "record_root": root, "chunk_root": chunk_root, "ranges": ranges, "roots": roots,
            "padding_bytes": pad, "raw": raw}


def same(rep, ref) -> list:
    """Differences between a ScrubReport and scrub_ref()'s result (empty: identical)."""
    diff = []
    for key in ("record_status", "record_root", "chunk_root", "ranges"):
        a, b = getattr(rep, key), ref[key]
        if a.shape != b.shape or not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0][:10] if a.shape == b.shape else "shape"
            diff.append((key, bad))
    got = {int(r["slot"]): (int(r["records"]), int(r["chunks"]), int(r["bytes"])) for r in rep.roots}
    want = {k: tuple(v) for k, v in ref["roots"].items()}
    if got != want:
        diff.append(("roots", sorted(set(got.items()) ^ set(want.items()), key=str)[:6]))
    if rep.padding_bytes != ref["padding_bytes"]:
        diff.append(("padding_bytes", rep.padding_bytes, ref["padding_bytes"]))
    return diff
