"""GPU: garbage collection of dropped segments (hmse_amd.gc) — the collected store is, byte for byte, what a fresh ingest of the
surviving segments writes (manifest and band-table sidecar), on every path: reused records, promoted POINTERs, re-based and
re-encoded records, with and without the sidecar; the two kernels (hmse_gc_plan, hmse_record_gather) against torch."""
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
    """The variants dataset of test_gpu_stream: 4 MiB of wiki-synth, five variants and a copy of a 200 KB piece of it, more text,
    then the first MiB again — 13 MiB + 12345 bytes, 14 segments of 1 MiB, the last one partial.  Extended by five variants of a
    second piece of the first 4 MiB WITHOUT an exact copy behind them: the first piece's copy is promoted when the first segments
    go and keeps its slot (its variants keep their dictionary), the second piece's variants lose theirs — re-based records and
    DELTA -> FULL changes."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import variants_dataset
    from hmse_amd import corpus
    a = corpus.wiki_synth(4 << 20, seed=42)
    v = variants_dataset(a)
    v2 = variants_dataset(a[1_400_000:])[200_000:-200_000]
    return np.concatenate([a, v, v2, corpus.wiki_synth((12 << 20) - a.size - v.size - v2.size, seed=7), a[: (1 << 20) + 12345]])


def _sidecar(res, cfg):
    from hmse_amd import bandtable
    return bandtable.write_band_tables(res.band_keys.cpu().numpy(), cfg.band_bits, signatures=res.sig.cpu().numpy())


def _store(data, cfg, dev, seg_off=None):
    import torch
    from hmse_amd import ingest, manifest
    from hmse_amd.config import LAYER_L4
    so = None if seg_off is None else torch.from_numpy(np.asarray(seg_off, np.int64)).to(dev)
    res = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg, seg_off=so)
    m = manifest.Manifest.from_bytes(manifest.build_manifest(res).to_bytes())
    return m, (_sidecar(res, cfg) if cfg.layers & LAYER_L4 else None)


def _remainder(data, so, drop):
    keep = [i for i in range(len(so) - 1) if i not in set(drop)]
    r = np.concatenate([data[so[i]: so[i + 1]] for i in keep]) if keep else data[:0]
    r_so = np.concatenate([[0], np.cumsum([so[i + 1] - so[i] for i in keep])]).astype(np.int64)
    return r, r_so


def _fixed(n, seg):
    k = max(1, -(-n // seg))
    return np.minimum(np.arange(k + 1, dtype=np.int64) * seg, n)


def _check_identity(m, data, drop, cfg, dev, side=None, seg_off=None):
    """GC of `drop`, then the contract: manifest bytes == fresh ingest of the remainder, sidecar == its index sidecar, read-back."""
    import torch
    from hmse_amd import gc, read
    from hmse_amd.config import LAYER_L4
    so = _fixed(data.size, cfg.seg_size) if seg_off is None else np.asarray(seg_off, np.int64)
    out, out_side, st = gc.drop_segments(m, drop, cfg, dev, band_tables=side, seg_off=seg_off)
    r, r_so = _remainder(data, so, drop)
    want, want_side = _store(r, cfg, dev, seg_off=r_so)
    assert out.to_bytes() == want.to_bytes()
    if cfg.layers & LAYER_L4:
        assert out_side == want_side
    else:
        assert out_side is None
    assert torch.equal(read.read_manifest(out, dev), torch.from_numpy(r).to(dev))
    assert st["chunks_after"] == len(want.chunk_map) and st["stored_after"] == len(want.index)
    assert st["records_reused"] + st["records_reencoded"] == st["stored_after"]
    assert st["blob_bytes_before"] == m.blob.size and st["blob_bytes_after"] == want.blob.size
    return out, st, r


@pytest.fixture(scope="module")
def variants(dev):
    from hmse_amd import IngestConfig
    cfg = IngestConfig(seg_size=MIB)
    data = _dataset()
    m, side = _store(data, cfg, dev)
    assert len(_fixed(data.size, MIB)) - 1 == 14
    return data, cfg, m, side


DROPS = {"none": [], "first": [0], "first4": [0, 1, 2, 3], "middle_pair": [6, 7], "last_partial": [13], "every_other": list(range(0, 14, 2))}


@pytest.mark.parametrize("sidecar", [True, False])
@pytest.mark.parametrize("name", list(DROPS))
def test_gc_equals_fresh_ingest_of_the_remainder(variants, dev, name, sidecar):
    data, cfg, m, side = variants
    out, st, r = _check_identity(m, data, DROPS[name], cfg, dev, side=side if sidecar else None)
    if sidecar:
        assert st["bytes_decoded"] < data.size // 2          # only the re-encode set and its dictionaries were decoded
    else:
        assert st["bytes_decoded"] == sum(m.chunk_map["raw_length"][m.chunk_map["kind"] != 1].astype(np.int64))
    if name == "first4" and sidecar:
        from hmse_amd import manifest
        assert manifest.reconstruct(out) == r.tobytes()      # stock zlib reads the collected store


def test_gc_exercises_promotion_rebasing_and_kind_changes(variants, dev):
    data, cfg, m, side = variants
    _, st, _ = _check_identity(m, data, [0, 1, 2, 3], cfg, dev, side=side)
    assert st["promoted"] > 10, st
    assert st["reencoded_base_dropped_or_moved"] + st["reencoded_base_changed"] > 10, st
    assert st["kind_changed"] >= 1, st
    assert st["reencoded_promoted"] + st["reencoded_base_dropped_or_moved"] + st["reencoded_base_changed"] == st["records_reencoded"]
    assert st["records_reused"] > st["stored_after"] // 2, st


def test_gc_drop_nothing_and_drop_everything(variants, dev):
    import torch
    from hmse_amd import gc, read
    data, cfg, m, side = variants
    out, out_side, st = gc.drop_segments(m, [], cfg, dev, band_tables=side)
    assert out.to_bytes() == m.to_bytes() and out_side == side
    assert st["records_reencoded"] == 0 and st["records_reused"] == len(m.index) and st["promoted"] == 0
    out, out_side, st = gc.drop_ranges(m, [(0, data.size)], cfg, dev, band_tables=side)
    assert len(out.chunk_map) == 0 and len(out.index) == 0 and out.blob.size == 0
    assert st["chunks_after"] == 0 and st["stored_after"] == 0
    assert read.read_manifest(out, dev).numel() == 0
    assert read.read_manifest(type(out).from_bytes(out.to_bytes()), dev).numel() == 0


def test_one_shard_inputs_share_one_body(variants, dev):
    """A Manifest, a Store of that one shard, and a Manifest with global_l4=True (every dictionary of one shard is local: the scope
    names nothing) give the same Manifest, the same sidecar and the same stats."""
    from hmse_amd import gc, manifest
    data, cfg, m, side = variants
    for sc in (side, None):
        out, out_side, st = gc.drop_segments(m, [0, 1, 2, 3], cfg, dev, band_tables=sc)
        assert isinstance(out, manifest.Manifest) and isinstance(out_side, bytes)
        for o2, side2, st2 in (gc.drop_segments(manifest.Store([m]), [0, 1, 2, 3], cfg, dev, band_tables=sc),
                               gc.drop_segments(m, [0, 1, 2, 3], cfg, dev, band_tables=sc, global_l4=True)):
            assert isinstance(o2, manifest.Manifest) and o2.to_bytes() == out.to_bytes() and side2 == out_side
            shared = set(st) & set(st2)
            assert {"chunks_after", "stored_after", "records_reused", "records_reencoded", "bytes_decoded", "blob_bytes_after"} <= shared
            assert all(st[k] == st2[k] for k in shared)


def test_retention_window_then_resume(dev):
    """Write with StreamIngest, drop the first batch, resume from the collected store and its sidecar, push two more batches:
    the result equals a one-shot ingest of (remainder + new batches)."""
    import torch
    from hmse_amd import IngestConfig, gc, ingest, manifest, stream
    cfg = IngestConfig(seg_size=MIB)
    data = _dataset()[: 13 * MIB]
    st0 = stream.StreamIngest(cfg, 11 * MIB, dev)
    for a, b in ((0, 4), (4, 8), (8, 11)):
        st0.push(torch.from_numpy(data[a * MIB: b * MIB].copy()))
    m0 = manifest.Manifest.from_bytes(manifest.build_manifest(st0.finish()).to_bytes())
    side0 = st0.index_sidecar()
    del st0
    m1, side1, stats = gc.drop_ranges(m0, [(0, 4 * MIB)], cfg, dev, band_tables=side0)
    assert stats["segments_dropped"] == 4
    # the sidecar is that of a stream that ingested the remainder
    sr = stream.StreamIngest(cfg, 7 * MIB, dev)
    sr.push(torch.from_numpy(data[4 * MIB: 11 * MIB].copy()))
    sr.finish()
    assert side1 == sr.index_sidecar()
    del sr
    st = stream.StreamIngest.resume(m1, cfg, 9 * MIB, dev, band_tables=side1)
    st.push(torch.from_numpy(data[11 * MIB: 12 * MIB].copy()))
    st.push(torch.from_numpy(data[12 * MIB: 13 * MIB].copy()))
    got = manifest.build_manifest(st.finish()).to_bytes()
    want = manifest.build_manifest(ingest.ingest_shard(torch.from_numpy(data[4 * MIB:].copy()).to(dev), cfg)).to_bytes()
    assert got == want


@pytest.mark.parametrize("variant", ["l1_cdc_dedupe", "lsh_8x16", "reference_preset", "delta_gate_20", "document_seg_off"])
def test_gc_identity_across_the_config_space(dev, variant):
    import torch
    from hmse_amd import ABLATIONS, IngestConfig, partition
    data = _dataset()
    cfg = IngestConfig(seg_size=MIB)
    seg_off = None
    if variant == "l1_cdc_dedupe":
        cfg = cfg.with_(layers=ABLATIONS["l1_cdc_dedupe"])
    elif variant == "lsh_8x16":
        cfg = cfg.with_(bands=8, rows=16)
    elif variant == "reference_preset":
        cfg = IngestConfig.reference_preset().with_(seg_size=MIB)
    elif variant == "delta_gate_20":
        cfg = cfg.with_(delta_max_ratio_pct=20)
    else:
        starts = partition.document_starts(torch.from_numpy(data).to(dev))
        seg_off = partition.document_seg_off(starts, data.size, MIB)
        assert len(seg_off) > 8 and not np.array_equal(seg_off, _fixed(data.size, MIB))
    m, side = _store(data, cfg, dev, seg_off=seg_off)
    n_seg = (len(seg_off) if seg_off is not None else len(_fixed(data.size, MIB))) - 1
    for drop, sc in (([0, 1, 2, 3], side), ([1, n_seg - 3], None)):
        _check_identity(m, data, drop, cfg, dev, side=sc, seg_off=seg_off)


def test_gc_refuses_a_store_written_under_other_lsh_parameters(dev):
    from hmse_amd import IngestConfig, gc
    data = _dataset()
    cfg = IngestConfig(seg_size=MIB)
    m, side = _store(data, cfg.with_(bands=8, rows=16), dev)
    with pytest.raises(ValueError, match="LSH base"):
        gc.drop_segments(m, [0], cfg, dev)
    with pytest.raises(ValueError, match="sidecar"):
        gc.drop_segments(m, [0], cfg, dev, band_tables=side)


@pytest.mark.parametrize("n,u", [(255, 60), (256, 60), (257, 60), (5000, 1200), (300000, 40000)])   # one block of 256 chunks and one either side; 300000: the block sums need a second trip of the 1024-wide scan
def test_plan_kernel_equals_l3_dedup_over_the_surviving_digests(dev, n, u):
    import torch
    from hmse_amd import ops
    rng = np.random.default_rng(n)
    lens = rng.integers(1, 200, n)
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    so = np.unique(np.concatenate([[0], rng.choice(cuts[1:-1], 40, replace=False), [cuts[-1]]])).astype(np.int64)
    drop = (rng.random(len(so) - 1) < 0.4).astype(np.uint8)
    slot = rng.integers(0, u, n).astype(np.int32)
    dig = rng.integers(0, 256, (u, 32), dtype=np.uint8)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    p = ops.gc_plan(t(cuts, torch.int64), t(slot, torch.int32), u, t(so, torch.int64), t(drop, torch.uint8), t(dig, torch.uint8))
    seg = np.searchsorted(so, cuts[:-1], side="right") - 1
    alive = np.nonzero(drop[seg] == 0)[0]
    assert np.array_equal(p["old_chunk"].cpu().numpy(), alive)
    surv = t(dig[slot[alive]], torch.uint8)
    fo, rc = ops.l3_dedup(surv)
    assert torch.equal(p["first_occ"], fo) and torch.equal(p["refcount"], rc) and torch.equal(p["digests"], surv)
    uniq = (fo == torch.arange(alive.size, device=dev)).nonzero().flatten()
    assert torch.equal(p["uniq_ids"], uniq)
    old_slot = slot[alive][uniq.cpu().numpy()]
    assert np.array_equal(p["old_slot"].cpu().numpy(), old_slot)
    inv = np.full(u, -1, np.int64)
    inv[old_slot] = np.arange(old_slot.size)
    assert np.array_equal(p["new_slot_of_old"].cpu().numpy(), inv)


def test_gather_kernel_equals_a_torch_copy(dev):
    import torch
    from hmse_amd import ops
    rng = np.random.default_rng(7)
    k = 3000
    lens = np.where(rng.random(k) < 0.1, 0, rng.integers(1, 65537, k))
    lens[:6] = [0, 1, 15, 16, 17, 65536]
    src0 = torch.from_numpy(rng.integers(0, 256, 40 << 20, dtype=np.uint8)).to(dev)
    src1 = torch.from_numpy(rng.integers(0, 256, 30 << 20, dtype=np.uint8)).to(dev)
    sel = rng.integers(0, 2, k).astype(np.uint8)
    cap = np.where(sel == 1, src1.numel(), src0.numel())
    off = (rng.integers(0, cap - lens) | 1).astype(np.int64)        # odd source offsets
    off = np.minimum(off, cap - lens)
    dst_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    got = ops.record_gather(src0, src1, t(off, torch.int64), t(sel, torch.uint8), t(dst_off, torch.int64))
    lt = t(lens, torch.int64)
    pos = torch.arange(int(dst_off[-1]), device=dev) - torch.repeat_interleave(t(dst_off[:-1], torch.int64), lt) + \
        torch.repeat_interleave(t(off, torch.int64), lt)
    which = torch.repeat_interleave(t(sel, torch.bool), lt)
    want = torch.where(which, src1[pos.clamp(max=src1.numel() - 1)], src0[pos])
    assert torch.equal(got, want)
    # an odd destination start (a record after a 3-byte one): unaligned heads and tails on the store side too
    got3 = ops.record_gather(src0, src1, t(np.r_[0, off], torch.int64), t(np.r_[0, sel], torch.uint8), t(np.r_[0, dst_off + 3], torch.int64))
    assert torch.equal(got3[3:], want) and torch.equal(got3[:3], src0[:3])
    with pytest.raises(ops.HmseError):
        ops.record_gather(src0, None, t([src0.numel() - 4], torch.int64), t([0], torch.uint8), t([0, 5], torch.int64))


def test_gc_at_scale_256_mib_drops_a_quarter(dev):
    from hmse_amd import IngestConfig, corpus
    cfg = IngestConfig()
    data = corpus.load("wikipedia", 256 << 20, seed=42)[0]
    m, side = _store(data, cfg, dev)
    drop = list(range(0, 64, 4))                              # 16 of 64 segments of 4 MiB, spread out
    _, st, _ = _check_identity(m, data, drop, cfg, dev, side=side)
    assert st["chunks_after"] < st["chunks_before"] and st["records_reused"] > st["stored_after"] // 2
