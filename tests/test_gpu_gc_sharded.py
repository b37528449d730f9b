"""GPU: garbage collection of a merged multi-shard store (hmse_amd.gc sharded path) — the collected store is, byte for byte, what a
fresh sharded ingest (ingest_shards_local) of every shard's surviving segments writes, and every sidecar is that run's; with
shard-local and global L4, with and without sidecars, with migrating stored chunks, emptied shards and remote dictionaries.
Also the band-table sidecar kernel (hmse_band_tables_write) against the numpy writer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _dataset():
    """test_gpu_gc's variants dataset: 4 MiB of wiki-synth, variants of two of its pieces (and an exact copy of the first), more
    text, then the first MiB again — 14 segments of 1 MiB, the last one partial."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import variants_dataset
    from hmse_amd import corpus
    a = corpus.wiki_synth(4 << 20, seed=42)
    v = variants_dataset(a)
    v2 = variants_dataset(a[1_400_000:])[200_000:-200_000]
    return np.concatenate([a, v, v2, corpus.wiki_synth((12 << 20) - a.size - v.size - v2.size, seed=7), a[: (1 << 20) + 12345]])


def _fixed(n, seg):
    k = max(1, -(-n // seg))
    return np.minimum(np.arange(k + 1, dtype=np.int64) * seg, n)


def _sharded(parts, cfg, dev, global_l4, seg_offs=None):
    """Fresh sharded ingest of `parts` -> (merged Store read back from its bytes, sidecars or None)."""
    import torch
    from hmse_amd import bandtable, ingest, manifest
    from hmse_amd.config import LAYER_L4
    so = None if seg_offs is None else [torch.from_numpy(np.asarray(s, np.int64)).to(dev) for s in seg_offs]
    rs = ingest.ingest_shards_local([torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in parts], cfg, global_l4=global_l4, seg_offs=so)
    n = len(rs)
    store = manifest.merge_manifests([manifest.build_manifest(r, i, n) for i, r in enumerate(rs)])
    sides = [bandtable.write_band_tables(r.band_keys.cpu().numpy(), cfg.band_bits, signatures=r.sig.cpu().numpy()) for r in rs] \
        if cfg.layers & LAYER_L4 else None
    return manifest.Store.from_bytes(store.to_bytes()), sides


def _remainders(parts, sos, drop):
    """Per shard the surviving bytes and their segment table, for GLOBAL segment indices `drop`."""
    gone = set(drop)
    out, g = [], 0
    for p, so in zip(parts, sos):
        keep = [i for i in range(len(so) - 1) if g + i not in gone]
        g += len(so) - 1
        r = np.concatenate([p[so[i]: so[i + 1]] for i in keep]) if keep else p[:0]
        r_so = np.concatenate([[0], np.cumsum([so[i + 1] - so[i] for i in keep])]).astype(np.int64) if keep else np.zeros(2, np.int64)
        out.append((r, r_so))
    return out


def _check(store, parts, sos, drop, cfg, dev, global_l4, sides=None, seg_off=None):
    import torch
    from hmse_amd import gc, read
    from hmse_amd.config import LAYER_L4
    out, out_sides, st = gc.drop_segments(store, drop, cfg, dev, band_tables=sides, seg_off=seg_off, global_l4=global_l4)
    rem = _remainders(parts, sos, drop)
    want, want_sides = _sharded([r for r, _ in rem], cfg, dev, global_l4, seg_offs=[s for _, s in rem])
    assert out.to_bytes() == want.to_bytes()
    if cfg.layers & LAYER_L4:
        assert len(out_sides) == len(parts) and out_sides == want_sides
    else:
        assert out_sides is None
    r_all = np.concatenate([r for r, _ in rem])
    assert torch.equal(read.read_store(out, dev).cpu(), torch.from_numpy(r_all))
    assert len(out.shards) == len(parts) and all(m.n_shards == len(parts) for m in out.shards)
    assert st["chunks_after"] == sum(len(m.chunk_map) for m in want.shards)
    assert st["stored_after"] == sum(len(m.index) for m in want.shards)
    assert [s["chunks_after"] for s in st["per_shard"]] == [len(m.chunk_map) for m in want.shards]
    assert [s["stored_after"] for s in st["per_shard"]] == [len(m.index) for m in want.shards]
    assert st["records_reused"] + st["records_reencoded"] == st["stored_after"]
    assert st["blob_bytes_after"] == sum(int(m.blob.size) for m in want.shards)
    return out, out_sides, st, r_all


CUTS3 = (4, 9)        # 3 shards: [0, 4) [4, 9) [9, 14) segments of 1 MiB
CUTS2 = (4,)


def _split(data, cuts_mib):
    b = [0] + [c * MIB for c in cuts_mib] + [data.size]
    return [data[b[i]: b[i + 1]] for i in range(len(b) - 1)]


@pytest.fixture(scope="module")
def three(dev):
    """The variants dataset in 3 shards, written shard-local and global: {scope: (store, sidecars)}."""
    from hmse_amd import IngestConfig
    cfg = IngestConfig(seg_size=MIB)
    data = _dataset()
    parts = _split(data, CUTS3)
    sos = [_fixed(p.size, MIB) for p in parts]
    stores = {g: _sharded(parts, cfg, dev, g) for g in (False, True)}
    return cfg, parts, sos, stores


def _n_cross_pointers(store):
    from hmse_amd.config import KIND_POINTER
    return sum(int(((m.chunk_map["kind"] == KIND_POINTER) & (m.chunk_map["shard"] != m.shard)).sum()) for m in store.shards)


DROPS3 = {"none": [], "first_of_shard0": [0], "middle_shard": list(range(4, 9)), "one_per_shard": [1, 6, 11],
          "every_other": list(range(0, 14, 2)), "everything": list(range(14))}


def test_stores_have_cross_shard_pointers_and_remote_dictionaries(three):
    cfg, parts, sos, stores = three
    for g in (False, True):
        assert _n_cross_pointers(stores[g][0]) > 20
    assert sum(m.n_remote() for m in stores[True][0].shards) > 20
    assert sum(m.n_remote() for m in stores[False][0].shards) == 0


@pytest.mark.parametrize("sidecar", [True, False])
@pytest.mark.parametrize("global_l4", [False, True])
@pytest.mark.parametrize("name", list(DROPS3))
def test_sharded_gc_equals_fresh_sharded_ingest(three, dev, name, global_l4, sidecar):
    cfg, parts, sos, stores = three
    store, sides = stores[global_l4]
    out, out_sides, st, r_all = _check(store, parts, sos, DROPS3[name], cfg, dev, global_l4, sides=sides if sidecar else None)
    if name == "first_of_shard0":
        assert st["records_migrated"] > 10, st
    if name == "middle_shard":
        assert len(out.shards[1].chunk_map) == 0 and len(out.shards[1].index) == 0 and out.shards[1].blob.size == 0
    if name == "everything":
        assert st["chunks_after"] == 0 and all(len(m.chunk_map) == 0 for m in out.shards)
    if name == "one_per_shard" and global_l4 and sidecar:
        from hmse_amd import manifest
        assert manifest.reconstruct(out) == r_all.tobytes()        # stock zlib reads the collected store
    if name == "none":
        assert out.to_bytes() == store.to_bytes() and st["records_reencoded"] == 0
        if sidecar:
            assert out_sides == sides


def test_global_l4_reencodes_and_reuses_remote_dictionaries(three, dev):
    """With global L4, some re-encoded records get a dictionary on another shard and some reused records keep one (a reused record
    keeps its old stream bytes, a re-encoded one with a new dictionary does not), over a few drop sets."""
    from hmse_amd import gc
    cfg, parts, sos, stores = three
    store, sides = stores[True]
    old_streams = set()
    for m in store.shards:
        for e in m.index:
            o = int(e["lba"]) * m.lba_unit
            old_streams.add(m.blob[o + 8: o + int(e["length"])].tobytes())
    kept = fresh = 0
    for drop in ([0], [0, 1], [0, 4], list(range(0, 14, 2))):
        out, _, st = gc.drop_segments(store, drop, cfg, dev, band_tables=sides, global_l4=True)
        assert st["records_reencoded"] > 0 and st["records_reused"] > 0
        for m in out.shards:
            for s in (m.remote_bases["slot"] if m.remote_bases is not None else []):
                e = m.index[int(s)]
                o = int(e["lba"]) * m.lba_unit
                if m.blob[o + 8: o + int(e["length"])].tobytes() in old_streams:
                    kept += 1
                else:
                    fresh += 1
    assert kept > 0 and fresh > 0, (kept, fresh)


def test_l1_cdc_dedupe_two_shards(dev):
    from hmse_amd import ABLATIONS, IngestConfig
    cfg = IngestConfig(seg_size=MIB).with_(layers=ABLATIONS["l1_cdc_dedupe"])
    parts = _split(_dataset(), CUTS2)
    sos = [_fixed(p.size, MIB) for p in parts]
    store, sides = _sharded(parts, cfg, dev, False)
    assert sides is None and _n_cross_pointers(store) > 20
    for drop in ([0], [1, 5, 9]):
        _check(store, parts, sos, drop, cfg, dev, False)


@pytest.mark.parametrize("global_l4", [False, True])
def test_document_aligned_seg_off_two_shards(dev, global_l4):
    import torch
    from hmse_amd import IngestConfig, partition
    cfg = IngestConfig(seg_size=MIB)
    parts = _split(_dataset(), CUTS2)
    sos = [partition.document_seg_off(partition.document_starts(torch.from_numpy(p).to(dev)), p.size, MIB) for p in parts]
    assert not all(np.array_equal(s, _fixed(p.size, MIB)) for s, p in zip(sos, parts))
    store, sides = _sharded(parts, cfg, dev, global_l4, seg_offs=sos)
    n0 = len(sos[0]) - 1
    for drop, sc in (([0, 1], sides), ([2, n0 + 1], None)):
        _check(store, parts, sos, drop, cfg, dev, global_l4, sides=sc, seg_off=sos)


def test_refuses_a_store_collected_in_the_other_scope(three, dev):
    import torch
    from hmse_amd import bandtable, gc, ops, read
    from hmse_amd.config import KIND_DELTA
    cfg, parts, sos, stores = three
    # written shard-local, collected as global: some DELTA header disagrees with the global LSH
    store, sides = stores[False]
    rd = read.StoreReader(store, dev)
    sig = np.concatenate([bandtable.read_signatures(s)[1] for s in sides]).view(np.int32)
    _, bg = ops.l4_lsh(torch.from_numpy(sig.copy()).to(dev), cfg)
    assert ((rd.kind == KIND_DELTA) & (rd.base != bg.cpu().numpy())).any()
    with pytest.raises(ValueError, match="LSH base"):
        gc.drop_segments(store, [0], cfg, dev, band_tables=sides, global_l4=True)
    # written global (remote dictionaries), collected shard-local
    store, sides = stores[True]
    assert sum(m.n_remote() for m in store.shards) > 0
    with pytest.raises(ValueError, match="LSH base"):
        gc.drop_segments(store, [0], cfg, dev, band_tables=sides, global_l4=False)


def test_refusals(three, dev):
    import torch
    from hmse_amd import gc, ingest, manifest
    from hmse_amd.manifest import PIECE_DTYPE, Manifest, Store
    cfg, parts, sos, stores = three
    store, sides = stores[False]
    with pytest.raises(ValueError, match="segment-aligned"):
        gc.drop_ranges(store, [(MIB, 100)], cfg, dev, band_tables=sides)
    # a two-rank stream store: the same shards with pieces that tile a stream
    ms = []
    g = 0
    for m in store.shards[:2]:
        pc = np.zeros(1, PIECE_DTYPE)
        pc["g0"], pc["n"] = g, len(m.chunk_map)
        g += len(m.chunk_map)
        ms.append(Manifest(m.lba_unit, m.index, m.chunk_map, m.pointers, m.blob, m.shard, 2, m.chunk_base, None, pc))
    with pytest.raises(ValueError, match="pieces"):
        gc.drop_segments(Store(ms), [0], cfg, dev)
    # an unmerged part
    rs = ingest.ingest_shards_local([torch.from_numpy(p).to(dev) for p in parts[:2]], cfg)
    part = manifest.build_manifest(rs[1], 1, 2)
    with pytest.raises(ValueError, match="merge_manifests"):
        gc.drop_segments(part, [0], cfg, dev)


def test_gc_twice_equals_one_gc_of_the_union(three, dev):
    from hmse_amd import gc
    cfg, parts, sos, stores = three
    for g in (False, True):
        store, sides = stores[g]
        once, once_sides, _ = gc.drop_segments(store, [0, 10], cfg, dev, band_tables=sides, global_l4=g)
        m1, s1, _ = gc.drop_segments(store, [0], cfg, dev, band_tables=sides, global_l4=g)
        rem = _remainders(parts, sos, [0])
        # original segment 10 is shard 2's second segment; after dropping segment 0 it is global segment 9
        m2, s2, _ = gc.drop_segments(m1, [9], cfg, dev, band_tables=s1, global_l4=g, seg_off=[s for _, s in rem])
        assert m2.to_bytes() == once.to_bytes() and s2 == once_sides


def test_sharded_gc_at_scale_four_shards_of_64_mib(dev):
    from hmse_amd import IngestConfig, corpus
    cfg = IngestConfig()
    data = corpus.load("wikipedia", 256 << 20, seed=42)[0]
    parts = [data[i * (64 << 20): (i + 1) * (64 << 20)] for i in range(4)]
    sos = [_fixed(p.size, cfg.seg_size) for p in parts]
    store, sides = _sharded(parts, cfg, dev, True)
    n_seg = sum(len(s) - 1 for s in sos)
    drop = list(range(1, n_seg, 4))
    _, _, st, _ = _check(store, parts, sos, drop, cfg, dev, True, sides=sides)
    assert st["chunks_after"] < st["chunks_before"] and st["records_reused"] > st["stored_after"] // 2


# ---- the sidecar kernel against the numpy writer -----------------------------------------------------------------------------

def _keys(rng, n, bands):
    return rng.integers(0, 1 << 32, (n, bands), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("with_sig", [False, True])
@pytest.mark.parametrize("band_bits", [12, 16])
@pytest.mark.parametrize("bands", [4, 8, 16])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000, 262145, 300000])   # a tile of 256 ids and one either side; 262145 = 256 x 1024 + 1: the scan of the run flags takes the second trip over its block sums
def test_band_tables_kernel_equals_numpy_writer(dev, n, bands, band_bits, with_sig):
    import torch
    from hmse_amd import bandtable
    rng = np.random.default_rng(n + bands + band_bits)
    keys = _keys(rng, n, bands)
    sig = rng.integers(0, 1 << 32, (n, 128), dtype=np.uint64).astype(np.uint32) if with_sig else None
    want = bandtable.write_band_tables(keys.view(np.int32), band_bits, signatures=None if sig is None else sig.view(np.int32))
    kd = torch.from_numpy(keys.view(np.int32)).to(dev)
    sd = None if sig is None else torch.from_numpy(sig.view(np.int32)).to(dev)
    got = bandtable.write_band_tables_device(kd, band_bits, signatures=sd)
    assert got == want


def test_band_tables_kernel_continuation_headers_and_colliding_keys(dev):
    """A bucket of 70001 ids (two headers, ids ascending across them), keys equal in the low bits but not the high ones."""
    import torch
    from hmse_amd import bandtable
    rng = np.random.default_rng(3)
    n = 200000
    keys = _keys(rng, n, 3)
    hot = rng.choice(n, 70001, replace=False)
    keys[hot, 1] = (keys[hot, 1] & np.uint32(0xFFFF0000)) | np.uint32(0x1234)      # one 16-bit bucket, many different keys
    keys[:, 2] = (keys[:, 2] & np.uint32(0xFFFFF000)) | (keys[:, 2] & np.uint32(7))  # 12 bits: only 8 buckets, all crowded
    for bits in (16, 12):
        want = bandtable.write_band_tables(keys.view(np.int32), bits)
        got = bandtable.write_band_tables_device(torch.from_numpy(keys.view(np.int32)).to(dev), bits)
        assert got == want
    _, tables = bandtable.read_band_tables(want)
    assert any(int(c) > 65535 for _, _, cnt, _ in tables for c in cnt)


def test_band_tables_kernel_refuses_too_many_ids(dev):
    import ctypes as C
    import torch
    from hmse_amd import _lib, bandtable, ops
    n = 1 << 24
    keys = torch.zeros((n, 1), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        bandtable.write_band_tables_device(keys, 16)
    with pytest.raises(ValueError):
        bandtable.write_band_tables(np.zeros((n, 1), np.int32), 16)
    # the C entry point flags it on the device (status bit 0) and writes nothing
    meta = torch.full((2,), 7, dtype=torch.int64, device=dev)
    out = torch.empty(64, dtype=torch.uint8, device=dev)
    rc = _lib.hip_lib().hmse_band_tables_write(keys.data_ptr(), n, 1, 16, None, 0, out.data_ptr(), 64, meta.data_ptr(), meta.data_ptr() + 8,
                                               None, 0, ops._stream())
    assert rc == 0
    assert meta.tolist()[0] == 0 and meta.tolist()[1] & 0xFFFFFFFF == 1
