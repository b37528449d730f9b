"""CPU: garbage collection (hmse_amd.gc) refuses what it does not support before any device work, and maps segment-aligned byte
ranges to the segments they cover."""
import numpy as np
import pytest

from hmse_amd import IngestConfig
from hmse_amd.config import ABLATIONS, KIND_FULL
from hmse_amd.manifest import CHUNK_INDEX_DTYPE, MAP_DTYPE, PIECE_DTYPE, POINTER_DTYPE, REMOTE_BASE_DTYPE, Manifest, Store

SEG = 10240
DEV = "cuda:0"          # never touched: every refusal comes first


def _store(n_chunks=35, chunk=1024):
    """A one-shard store of n_chunks FULL records of `chunk` bytes (3.5 segments of SEG bytes at the default)."""
    idx = np.zeros(n_chunks, CHUNK_INDEX_DTYPE)
    idx["sha256"][:, 0] = np.arange(n_chunks) + 1
    idx["lba"] = np.arange(n_chunks) * 4
    idx["length"] = 4
    idx["refcount"] = 1
    cmap = np.zeros(n_chunks, MAP_DTYPE)
    cmap["slot"] = np.arange(n_chunks)
    cmap["raw_length"] = chunk
    cmap["kind"] = KIND_FULL
    return Manifest(1, idx, cmap, np.zeros(0, POINTER_DTYPE), np.zeros(4 * n_chunks, np.uint8))


def _cfg(**kw):
    return IngestConfig(seg_size=SEG, **kw)


def test_refuses_multi_shard_stores():
    from hmse_amd import gc
    m = _store()
    with pytest.raises(ValueError, match="shard"):
        gc.drop_segments(Store([m, m]), [0], _cfg(), DEV)
    m2 = Manifest(m.lba_unit, m.index, m.chunk_map, m.pointers, m.blob, shard=1, n_shards=2, chunk_base=35)
    with pytest.raises(ValueError, match="shard"):
        gc.drop_segments(m2, [0], _cfg(), DEV)
    rb = np.zeros(1, REMOTE_BASE_DTYPE)
    m3 = Manifest(m.lba_unit, m.index, m.chunk_map, m.pointers, m.blob, remote_bases=rb)
    with pytest.raises(ValueError, match="remote_bases"):
        gc.drop_segments(m3, [0], _cfg(), DEV)
    pc = np.zeros(1, PIECE_DTYPE)
    pc["n"] = 35
    m4 = Manifest(m.lba_unit, m.index, m.chunk_map, m.pointers, m.blob, pieces=pc)
    with pytest.raises(ValueError, match="pieces"):
        gc.drop_segments(m4, [0], _cfg(), DEV)
    # a Store of one shard is fine up to the device work; its shard's refusals still apply
    with pytest.raises(ValueError, match="layer"):
        gc.drop_segments(Store([m]), [0], _cfg(layers=ABLATIONS["cdc_dedupe"]), DEV)


@pytest.mark.parametrize("name", ["l1_only", "l1_cdc", "l4_only", "cdc_dedupe"])
def test_refuses_layer_masks_without_l1_l3_or_unsupported(name):
    from hmse_amd import gc
    with pytest.raises(ValueError, match="layer"):
        gc.drop_segments(_store(), [1], _cfg(layers=ABLATIONS[name]), DEV)
    with pytest.raises(ValueError, match="layer"):
        gc.drop_ranges(_store(), [(0, SEG)], _cfg(layers=ABLATIONS[name]), DEV)


def test_refuses_a_cut_list_that_misses_a_segment_boundary():
    from hmse_amd import gc
    with pytest.raises(ValueError, match="misses segment boundary 10000"):
        gc.drop_segments(_store(), [0], IngestConfig(seg_size=10000), DEV)
    with pytest.raises(ValueError, match="misses segment boundary"):
        gc.drop_segments(_store(), [0], _cfg(), DEV, seg_off=np.array([0, 5000, 35840]))
    with pytest.raises(ValueError, match="seg_off"):
        gc.drop_segments(_store(), [0], _cfg(), DEV, seg_off=np.array([0, 10240]))
    with pytest.raises(ValueError, match="out of range"):
        gc.drop_segments(_store(), [4], _cfg(), DEV)


def test_refuses_ranges_that_are_not_segment_aligned():
    from hmse_amd import gc
    with pytest.raises(ValueError, match="byte 20580 lies between segment boundaries 20480 and 30720"):
        gc.drop_ranges(_store(), [(SEG, SEG + 100)], _cfg(), DEV)
    with pytest.raises(ValueError, match="between segment boundaries 0 and 10240"):
        gc.drop_ranges(_store(), [(5, SEG - 5)], _cfg(), DEV)
    with pytest.raises(ValueError, match="outside"):
        gc.drop_ranges(_store(), [(0, 40000)], _cfg(), DEV)


def test_drop_ranges_maps_aligned_ranges_to_segments(monkeypatch):
    from hmse_amd import gc
    so = gc.store_seg_off(_store(), _cfg())
    assert so.tolist() == [0, 10240, 20480, 30720, 35840]
    assert gc.segments_of_ranges(so, [(0, SEG)]) == [0]
    assert gc.segments_of_ranges(so, [(SEG, 2 * SEG), (30720, 5120)]) == [1, 2, 3]
    assert gc.segments_of_ranges(so, [(0, 35840)]) == [0, 1, 2, 3]
    assert gc.segments_of_ranges(so, [(SEG, 0), (20480, SEG), (20480, SEG)]) == [2]
    seen = {}

    def fake(m, drop, cfg, device, band_tables=None, seg_off=None, global_l4=False, verify=True, timings=None):
        seen.update(drop=drop, seg_off=np.asarray(seg_off).tolist())
        return "ok"
    monkeypatch.setattr(gc, "drop_segments", fake)
    assert gc.drop_ranges(_store(), [(30720, 5120), (0, SEG)], _cfg(), DEV) == "ok"
    assert seen == {"drop": [0, 3], "seg_off": [0, 10240, 20480, 30720, 35840]}
    # a document-aligned table: ranges follow its boundaries, not the fixed grid
    doc = np.array([0, 4096, 20480, 35840])
    assert gc.drop_ranges(_store(), [(4096, 16384)], _cfg(), DEV, seg_off=doc) == "ok"
    assert seen == {"drop": [1], "seg_off": doc.tolist()}
