"""GPU: hmse_amd.scrub against the host reference (tests/scrub_ref.py), exactly — clean stores of every kind, flipped payload bytes in
FULL records, dictionaries, cross-shard POINTER targets and remote dictionaries, header damage, a zeroed run, padding, a flipped
sidecar signature, salvage, repair from replicas and from sources, both inflate decoders, and a 256 MiB store with random flips."""
import dataclasses
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MIB = 1 << 20
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _data(n=6 * MIB, seed=42):
    from hmse_amd import corpus
    a = corpus.wiki_synth(n, seed=seed)
    rng = np.random.default_rng(seed)
    for _ in range(3):                                   # near-duplicates: DELTA records, chains of them, POINTERs
        src = int(rng.integers(0, n // 2)); dst = int(rng.integers(n // 2, n - 700000))
        v = a[src: src + 600000].copy()
        v[::1500] ^= 0x20
        a[dst: dst + v.size] = v
    a[n - 400000:] = a[100000:500000]
    return a


def _copy(store):
    from hmse_amd import manifest
    st = manifest.Store.from_bytes(store.to_bytes())
    return manifest.Store([dataclasses.replace(m, blob=m.blob.copy()) for m in st.shards])


@pytest.fixture(scope="module")
def stores(dev):
    """{kind: (store, corpus, cfg, sidecars or None)}: one manifest; 3 shards with global L4 (cross-shard POINTERs, remote dictionaries);
    a 2-rank stream store (pieces)."""
    import torch
    from hmse_amd import IngestConfig, bandtable, ingest, manifest, stream_dist
    cfg = IngestConfig(seg_size=MIB)
    data = _data()
    out = {}
    r = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    out["one"] = (_copy(manifest.Store([manifest.build_manifest(r)])), data, cfg,
                  [bandtable.write_band_tables(r.band_keys.cpu().numpy(), cfg.band_bits, signatures=r.sig.cpu().numpy())])
    parts = [data[: 2 * MIB], data[2 * MIB: 4 * MIB], data[4 * MIB:]]
    rs = ingest.ingest_shards_local([torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in parts], cfg, global_l4=True)
    st = manifest.merge_manifests([manifest.build_manifest(x, i, 3) for i, x in enumerate(rs)])
    out["sharded"] = (_copy(st), data, cfg, [bandtable.write_band_tables(x.band_keys.cpu().numpy(), cfg.band_bits, signatures=x.sig.cpu().numpy())
                                              for x in rs])
    B = 2 * MIB
    res = stream_dist.stream_shards_local([torch.from_numpy(data[a: a + B].copy()) for a in range(0, data.size, B)], cfg, 2, dev)
    sr = stream_dist.store_results(res)
    st = manifest.merge_manifests([manifest.build_manifest(sr[i], i, 2) for i in range(2)])
    out["stream"] = (_copy(st), data, cfg, None)
    return out


def _check(store, dev, **kw):
    import scrub_ref
    from hmse_amd import scrub
    rep = scrub.scrub(store, dev, **kw)
    ref = scrub_ref.scrub_ref(store)
    assert scrub_ref.same(rep, ref) == [], scrub_ref.same(rep, ref)
    return rep, ref


def _rec(store, g):
    """(shard, byte offset in its blob, length, kind) of global record g."""
    from hmse_amd import scrub
    p = scrub.plan(store)
    s = int(p.rec_shard[g])
    return s, int(p.rec_off[g] - p.shard_blob[s]), int(p.rec_len[g]), int(p.kind[g]), p


def _outside_ranges_equal(got, data, ranges):
    mask = np.ones(data.size, bool)
    for o, n in ranges:
        mask[o: o + n] = False
    return np.array_equal(got[mask], data[mask])


@pytest.mark.parametrize("kind", ["one", "sharded", "stream"])
def test_clean_stores_are_clean_and_salvage_is_read_store(stores, dev, kind):
    from hmse_amd import read, scrub
    store, data, cfg, sides = stores[kind]
    rep, _ = _check(store, dev, cfg=cfg if sides else None, band_tables=sides)
    assert rep.clean and rep.lossless and len(rep.roots) == 0, rep.summary()
    if sides:
        assert rep.sidecar["sig_bad"] == 0 and rep.sidecar["sig_unchecked"] == 0 and all(rep.sidecar["tables_ok"])
    got, rep2 = scrub.salvage(store, dev)
    assert np.array_equal(got.cpu().numpy(), read.read_store(store, dev).cpu().numpy()) and np.array_equal(got.cpu().numpy(), data)


def _pick(store, want):
    """A global record of the wanted role: 'leaf' FULL nothing depends on and no POINTER names, 'dict' with DELTA dependants,
    'xptr' target of a cross-shard POINTER, 'remote' a dictionary used from another shard."""
    from hmse_amd import scrub
    p = scrub.plan(store)
    raw_dicts = _dicts(store)
    used = np.bincount(raw_dicts[raw_dicts >= 0], minlength=p.n)
    named = np.bincount(p.chunk_slot[p.chunk_slot >= 0], minlength=p.n)
    if want == "leaf":
        c = np.nonzero((p.kind == 0) & (used == 0) & (named == 1) & (p.rec_len > 64))[0]
    elif want == "dict":
        c = np.nonzero((p.kind == 0) & (used >= 1) & (p.rec_len > 64))[0]
    elif want == "remote":
        r = p.remote[p.remote >= 0]
        c = np.unique(r[p.rec_len[r] > 64])
    else:
        own_shard = np.concatenate([np.full(len(m.chunk_map), i) for i, m in enumerate(p.shards)])
        if p.perm is not None:
            own_shard = own_shard[p.perm]
        tg = p.chunk_slot
        x = (tg >= 0) & (p.rec_shard[np.maximum(tg, 0)] != own_shard)
        c = np.unique(tg[x])
        c = c[p.rec_len[c] > 64]
    assert len(c), want
    return int(c[len(c) // 2])


def _dicts(store):
    from hmse_amd import scrub
    p = scrub.plan(store)
    d = np.full(p.n, -1, np.int64)
    blob = np.concatenate([m.blob for m in p.shards])
    lba_of = [{int(v): j for j, v in enumerate(m.index["lba"])} for m in p.shards]
    for k in np.nonzero(p.kind == 2)[0]:
        lba = int(blob[p.rec_off[k]: p.rec_off[k] + 4].view("<u4")[0])
        r = int(p.remote[k])
        s = int(p.rec_shard[r]) if r >= 0 else int(p.rec_shard[k])
        j = lba_of[s].get(lba)
        if j is not None:
            d[k] = int(p.shard_slot[s]) + j
    return d


@pytest.mark.parametrize("kind,role", [("one", "leaf"), ("one", "dict"), ("sharded", "xptr"), ("sharded", "remote"), ("stream", "dict")])
def test_one_flipped_payload_byte(stores, dev, kind, role):
    from hmse_amd import read, scrub
    store0, data, cfg, sides = stores[kind]
    store = _copy(store0)
    g = _pick(store, role)
    s, o, L, k, p = _rec(store, g)
    store.shards[s].blob[o + (8 if k == 2 else 0) + L // 3] ^= 0x5A
    rep, ref = _check(store, dev)
    assert not rep.lossless and rep.record_root[g] == g and rep.record_status[g] & (scrub.STREAM | scrub.DIGEST)
    dep = np.nonzero(rep.record_root == g)[0]
    if role in ("dict", "remote"):
        assert len(dep) >= 2 and (rep.record_status[dep[dep != g]] & scrub.DICTIONARY).all()
    if role == "remote":
        assert (p.rec_shard[dep] != p.rec_shard[g]).any()
    if role == "xptr":
        assert (rep.chunk_root == g).sum() >= 2
    got, _ = scrub.salvage(store, dev, fill=0xEE)
    got = got.cpu().numpy()
    assert _outside_ranges_equal(got, data, rep.ranges)
    for o2, n2 in rep.ranges:
        assert (got[o2: o2 + n2] == 0xEE).all()
    with pytest.raises(Exception):
        read.read_store(store, dev)


def test_base_lba_damage_is_structure_and_names_the_dependants(stores, dev):
    from hmse_amd import read, scrub
    store0, data, cfg, _ = stores["one"]
    store = _copy(store0)
    p = scrub.plan(store)
    d = _dicts(store)
    used = np.bincount(d[d >= 0], minlength=p.n)
    cand = np.nonzero(p.kind == 2)[0]
    g = int(cand[np.argmax(used[cand] * 1000 + np.bincount(p.chunk_slot[p.chunk_slot >= 0], minlength=p.n)[cand])])
    s, o, L, k, _ = _rec(store, g)
    store.shards[s].blob[o: o + 4] = 0xFF
    with pytest.raises(read.ReadError):
        read.read_store(store, dev)
    rep, _ = _check(store, dev)
    assert rep.record_status[g] & scrub.STRUCTURE and rep.record_root[g] == g
    kids = np.nonzero(d == g)[0]
    assert (rep.record_root[kids] == g).all() and (rep.record_status[kids] & scrub.DICTIONARY).all()
    assert (rep.chunk_root[p.chunk_slot == g] == g).all() and int((rep.chunk_root == g).sum()) == int(rep.roots["chunks"][rep.roots["slot"] == g][0])


def test_header_length_damage_is_header_only_and_repair_restores_it(stores, dev):
    from hmse_amd import scrub
    store0, data, cfg, _ = stores["sharded"]
    store = _copy(store0)
    p = scrub.plan(store)
    ds = np.nonzero(p.kind == 2)[0]
    assert len(ds) >= 3 and (p.remote[ds] >= 0).any()                  # (remote dictionaries among them)
    for g, off in ((int(ds[0]), 4), (int(ds[-1]), 6), (int(ds[p.remote[ds] >= 0][0]) if ds[p.remote[ds] >= 0][0] not in (ds[0], ds[-1]) else int(ds[1]), 5)):
        s, o, L, k, _ = _rec(store, g)
        store.shards[s].blob[o + off] ^= 0x11
    rep, _ = _check(store, dev)
    assert rep.lossless and not rep.clean and int(((rep.record_status & scrub.HEADER) != 0).sum()) == 3
    assert not (rep.record_status & ~np.uint8(scrub.HEADER)).any()
    fixed, rep2 = scrub.repair(store, dev)
    assert rep2.clean and fixed.to_bytes() == store0.to_bytes()
    assert store.to_bytes() != store0.to_bytes()                          # the input is left as it was


def test_zeroed_run_across_records(stores, dev):
    from hmse_amd import scrub
    store0, data, cfg, _ = stores["one"]
    store = _copy(store0)
    _, o, L, _, _ = _rec(store, 40)
    store.shards[0].blob[o + 10: o + 10 + 30000] = 0
    rep, _ = _check(store, dev)
    assert len(np.unique(rep.record_root[rep.record_root >= 0])) >= 3
    got, _ = scrub.salvage(store, dev)
    assert _outside_ranges_equal(got.cpu().numpy(), data, rep.ranges)


def _relayout(m, unit):
    """The same one-shard manifest with every record on a multiple of `unit` (zero padding between records)."""
    from hmse_amd import scrub
    p = scrub.plan(m)
    new = np.zeros(p.n, np.int64)
    pos = 0
    for k in range(p.n):
        new[k] = pos
        pos += -(-int(p.rec_len[k]) // unit) * unit
    blob = np.zeros(pos, np.uint8)
    idx = m.index.copy()
    for k in range(p.n):
        blob[new[k]: new[k] + p.rec_len[k]] = m.blob[p.rec_off[k]: p.rec_off[k] + p.rec_len[k]]
    idx["lba"] = new // unit
    for k in np.nonzero(p.kind == 2)[0]:
        old = int(blob[new[k]: new[k] + 4].view("<u4")[0])
        j = int(np.nonzero(m.index["lba"] == old)[0][0])
        blob[new[k]: new[k] + 4] = np.frombuffer(np.uint32(idx["lba"][j]).tobytes(), np.uint8)
    ptr = m.pointers.copy()
    own = {int(a): int(b) for a, b in zip(m.index["lba"], idx["lba"])}
    ptr["target_lba"] = [own[int(x)] for x in ptr["target_lba"]]
    return dataclasses.replace(m, lba_unit=unit, index=idx, pointers=ptr, blob=blob)


def test_padding_only_is_lossless_not_clean_and_repair_zeroes_it(stores, dev):
    from hmse_amd import manifest, read, scrub
    store0, data, cfg, _ = stores["one"]
    m = _relayout(store0.shards[0], 16)
    pristine = manifest.Store([m])
    assert np.array_equal(read.read_store(pristine, dev).cpu().numpy(), data)
    bad = _copy(pristine)
    p = scrub.plan(bad)
    gaps = [int(p.rec_off[k] + p.rec_len[k]) for k in range(p.n) if p.rec_len[k] % 16][:5]
    for x in gaps:
        bad.shards[0].blob[x] = 0x33
    rep, _ = _check(bad, dev)
    assert rep.lossless and not rep.clean and rep.padding_bytes == len(gaps)
    fixed, rep2 = scrub.repair(bad, dev)
    assert rep2.clean and fixed.to_bytes() == pristine.to_bytes()


def test_flipped_sidecar_signature(stores, dev):
    from hmse_amd import scrub
    store, data, cfg, sides = stores["sharded"]
    bad = [bytearray(s) for s in sides]
    bad[1][-5] ^= 1                                                      # a word of the last record's signature
    rep = scrub.scrub(store, dev, cfg=cfg, band_tables=[bytes(b) for b in bad])
    assert rep.lossless and not rep.clean and rep.sidecar["sig_bad"] == 1 and all(rep.sidecar["tables_ok"])
    p = scrub.plan(store)
    assert rep.sidecar["sig_status"][int(p.shard_slot[2]) - 1] == scrub.SIG_BAD
    short = scrub.scrub(store, dev, cfg=cfg, band_tables=[sides[0], sides[1][:-4], sides[2]])
    assert short.sidecar["usable"] == [True, False, True] and not short.clean


def _damage(store, recs, rng):
    from hmse_amd import scrub
    p = scrub.plan(store)
    for g in recs:
        s = int(p.rec_shard[g]); o = int(p.rec_off[g] - p.shard_blob[s]); L = int(p.rec_len[g])
        h = 8 if p.kind[g] == 2 else 0
        store.shards[s].blob[o + h + int(rng.integers(0, L - h))] ^= 0xFF


def test_repair_from_replicas(stores, dev):
    from hmse_amd import scrub
    store0, data, cfg, _ = stores["sharded"]
    p = scrub.plan(store0)
    rng = np.random.default_rng(7)
    big = np.nonzero(p.rec_len > 32)[0]
    ra, rb = rng.choice(big, 12, replace=False).reshape(2, 6)
    a, b = _copy(store0), _copy(store0)
    _damage(a, ra, rng); _damage(b, rb, rng)
    fixed, rep = scrub.repair(a, dev, replicas=[b])
    assert rep.clean and fixed.to_bytes() == store0.to_bytes()
    # overlapping damage: exactly the overlap's roots remain
    c = _copy(store0)
    _damage(c, np.concatenate([ra[:3], rb[:2]]), np.random.default_rng(7))
    fixed, rep = scrub.repair(a, dev, replicas=[c])
    ra_rep = scrub.scrub(a, dev)
    c_rep = scrub.scrub(c, dev)
    both = ((ra_rep.record_status & scrub.DAMAGE) != 0) & ((c_rep.record_status & scrub.DAMAGE) != 0)
    assert set(rep.roots["slot"].tolist()) == set(np.unique(ra_rep.record_root[both]).tolist())


def test_repair_from_sources(stores, dev):
    from hmse_amd import scrub
    store0, data, cfg, _ = stores["one"]
    store = _copy(store0)
    p = scrub.plan(store)
    d = _dicts(store)
    full = int(np.nonzero((p.kind == 0) & (p.rec_len > 64))[0][3])
    delta = int(np.nonzero((p.kind == 2) & (p.rec_len > 64) & (d >= 0) & (d != full))[0][0])
    _damage(store, [full, delta], np.random.default_rng(3))
    rep0 = scrub.scrub(store, dev)
    assert rep0.record_root[full] == full and rep0.record_root[delta] == delta
    fixed, rep = scrub.repair(store, dev, cfg=cfg, sources=[(0, data.tobytes())])
    assert rep.clean and fixed.to_bytes() == store0.to_bytes()


def test_report_is_the_same_under_both_decoders(stores, dev):
    from hmse_amd import ops, scrub
    store0, data, cfg, _ = stores["sharded"]
    store = _copy(store0)
    p = scrub.plan(store)
    _damage(store, np.random.default_rng(11).choice(np.nonzero(p.rec_len > 32)[0], 20, replace=False), np.random.default_rng(12))
    try:
        ops.l1_inflate_mode(1)
        a = scrub.scrub(store, dev)
        ops.l1_inflate_mode(2)
        b = scrub.scrub(store, dev)
    finally:
        ops.l1_inflate_mode(0)
    for key in ("record_status", "record_root", "chunk_root", "ranges"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key
    assert a.roots.tobytes() == b.roots.tobytes()


def test_256_mib_store_with_random_flips(dev):
    import torch
    from hmse_amd import IngestConfig, corpus, ingest, manifest, scrub
    cfg = IngestConfig()
    data = corpus.wiki_synth(256 * MIB, seed=5)
    r = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    store = _copy(manifest.Store([manifest.build_manifest(r)]))
    del r
    rng = np.random.default_rng(256)
    blob = store.shards[0].blob
    for x in rng.integers(0, blob.size, 300):
        blob[x] ^= np.uint8(1 << int(rng.integers(0, 8)))
    rep, _ = _check(store, dev)
    assert 100 <= len(rep.roots) <= 300 and not rep.lossless
    got, _ = scrub.salvage(store, dev)
    assert _outside_ranges_equal(got.cpu().numpy(), data, rep.ranges)


def test_metadata_damage_is_reported_and_salvaged(stores, dev):
    """Inconsistent metadata never used silently: a cross-shard POINTER whose raw_length disagrees with its target's record, a
    pointer record with the wrong target_lba, a remote_bases row naming a record that does not exist.  Both POINTER chunks are
    METADATA (chunk root -2, one MAP_BAD row), the record of the bad row is METADATA with its dependants; salvage fills them all."""
    from hmse_amd import manifest, read, scrub
    store0, data, cfg, _ = stores["sharded"]
    st = _copy(store0)
    shards = [dataclasses.replace(m, chunk_map=m.chunk_map.copy(), pointers=m.pointers.copy(),
                                  remote_bases=None if m.remote_bases is None else m.remote_bases.copy()) for m in st.shards]
    store = manifest.Store(shards)
    m2 = shards[2]
    ptr = np.nonzero(m2.chunk_map["kind"] == 1)[0]
    cross = ptr[m2.chunk_map["shard"][ptr] != 2]
    m2.chunk_map["raw_length"][cross[0]] -= 3                          # POINTER raw_length != the target's raw length
    m2.pointers["target_lba"][len(ptr) // 2] += 1                      # pointer record disagrees with the target's index entry
    rb_shard = next(i for i, m in enumerate(shards) if m.n_remote())
    shards[rb_shard].remote_bases["base_slot"][0] = 0xFFFFFF            # names no record of that shard
    with pytest.raises(Exception):
        read.read_store(store, dev)
    rep, _ = _check(store, dev)
    p = scrub.plan(store)
    bad_rec = int(p.shard_slot[rb_shard]) + int(shards[rb_shard].remote_bases["slot"][0])
    assert rep.record_status[bad_rec] & scrub.METADATA and rep.record_root[bad_rec] == bad_rec
    assert (rep.chunk_root == scrub.MAP_BAD).sum() == 2
    row = rep.roots[rep.roots["slot"] == scrub.MAP_BAD]
    lens = p.chunk_len[rep.chunk_root == scrub.MAP_BAD]
    assert len(row) == 1 and row["cause"][0] == scrub.METADATA and row["chunks"][0] == 2 and row["bytes"][0] == int(lens.sum())
    got, _ = scrub.salvage(store, dev, fill=0x7E)
    got = got.cpu().numpy()
    assert got.size == int(p.chunk_len.sum())
    # outside the ranges the bytes are the corpus's; a chunk map whose lengths are wrong shifts what follows, so compare by chunk
    cuts = np.concatenate([[0], np.cumsum(p.chunk_len)])
    want = np.concatenate([[0], np.cumsum(np.concatenate([m.chunk_map["raw_length"] for m in store0.shards]).astype(np.int64))])
    for c in np.nonzero(rep.chunk_root == -1)[0][::97]:
        assert np.array_equal(got[cuts[c]: cuts[c + 1]], data[want[c]: want[c + 1]])
    for o2, n2 in rep.ranges:
        assert (got[o2: o2 + n2] == 0x7E).all()


def test_records_pass_counts_the_blob_of_a_shard_without_records(dev):
    """hmse_scrub_records with no record at all: the whole blob of each record-less shard is padding (shard bounds clamped to the
    blob passed)."""
    import torch
    from hmse_amd import ops
    blob = torch.tensor([0, 5, 0, 0, 7, 1, 0, 0], dtype=torch.uint8, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    e32, e64, e8 = i32([]), i64([]), torch.zeros(0, dtype=torch.uint8, device=dev)
    _, _, pad = ops.scrub_records(blob, e32, i64([0, 3, 99]), i64([0, 0, 0]), i32([1, 1]), e32, e32, e8, e64, e32, e32, 0, e8)
    assert int(pad.item()) == 3                                        # [0, 3) holds 1 non-zero byte, [3, 8) (clamped from 99) 2



@pytest.mark.parametrize("n_chunks", [255, 256, 257, 262145])
def test_attribute_ranges_of_damaged_chunk_runs_equal_a_run_length_count(dev, n_chunks):
    """ops.scrub_attribute on synthetic tables: every record good, no dictionary, chunk_slot -1 (a damaged chunk, root -2) in seeded random
    runs, the last chunk damaged (its run ends at the boundary thread n_chunks).  n_chunks = 255 / 256 / 257: that thread is the last of
    the first block, the first of a second, and inside it; 262145 = 256 x 1024 + 1 blocks of boundaries: the scan over the block counts
    takes its second trip.  ranges and counts[0, 4, 5] equal numpy's run lengths."""
    import torch
    from hmse_amd import ops
    rng = np.random.default_rng(n_chunks)
    n = 7
    runs = rng.integers(1, 9, n_chunks)                                       # lengths of alternating good / damaged runs
    bad = (np.repeat(np.arange(n_chunks) % 2, runs)[:n_chunks] == (n_chunks % 2)).copy()
    bad[-1] = True
    slot = np.where(bad, -1, rng.integers(0, n, n_chunks)).astype(np.int64)
    cuts = np.concatenate([[0], np.cumsum(rng.integers(1, 100, n_chunks))]).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sha = t(np.zeros((n, 32), np.uint8))
    r = ops.scrub_attribute(t(np.zeros(n, np.uint8)), t(np.full(n, -1, np.int64)), t(np.ones(n, np.uint8)), sha, sha, False, t(slot), t(cuts), 0)
    edge = np.diff(np.concatenate([[0], bad.astype(np.int8), [0]]))
    start, end = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    want = np.stack([cuts[start], cuts[end] - cuts[start]], axis=1).reshape(-1)
    counts = r["counts"].cpu().numpy()
    assert counts[0] == start.size and counts[4] == bad.sum() and counts[5] == (cuts[1:] - cuts[:-1])[bad].sum()
    assert np.array_equal(r["ranges"].cpu().numpy()[: want.size], want)
    assert np.array_equal(r["chunk_root"].cpu().numpy()[:n_chunks], np.where(bad, -2, -1))
