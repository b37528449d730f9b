"""CPU: the host side of sharded garbage collection (hmse_amd.gc) — global segment numbering across shards (empty shards
included), corpus ranges -> (shard, local segment), and the refusals that come before any device work."""
import numpy as np
import pytest

from hmse_amd import IngestConfig
from hmse_amd.config import KIND_FULL, KIND_POINTER
from hmse_amd.manifest import CHUNK_INDEX_DTYPE, MAP_DTYPE, PIECE_DTYPE, POINTER_DTYPE, Manifest, Store

SEG = 10240
DEV = "cuda:0"          # never touched: every result here comes before device work


def _shard(n_chunks, shard, n_shards, chunk_base, chunk=1024):
    """A shard of n_chunks FULL records of `chunk` bytes."""
    idx = np.zeros(n_chunks, CHUNK_INDEX_DTYPE)
    idx["sha256"][:, 0] = np.arange(n_chunks) + 1
    idx["sha256"][:, 1] = shard
    idx["lba"] = np.arange(n_chunks) * 4
    idx["length"] = 4
    idx["refcount"] = 1
    cmap = np.zeros(n_chunks, MAP_DTYPE)
    cmap["slot"] = np.arange(n_chunks)
    cmap["raw_length"] = chunk
    cmap["kind"] = KIND_FULL
    cmap["shard"] = shard
    return Manifest(1, idx, cmap, np.zeros(0, POINTER_DTYPE), np.zeros(4 * n_chunks, np.uint8), shard, n_shards, chunk_base)


def _store(sizes=(35, 0, 20)):
    """Shards of 35, 0 and 20 chunks of 1 KiB: 4 + 1 (empty) + 2 segments of SEG bytes."""
    out, base = [], 0
    for i, n in enumerate(sizes):
        out.append(_shard(n, i, len(sizes), base))
        base += n
    return Store(out)


def _cfg(**kw):
    return IngestConfig(seg_size=SEG, **kw)


def test_global_segment_table_and_split():
    from hmse_amd import gc
    sos, so_g, seg_base = gc.shard_segments(_store(), _cfg())
    assert [len(s) - 1 for s in sos] == [4, 1, 2]
    assert np.array_equal(sos[1], [0, 0])                                           # the empty shard keeps one empty segment
    assert np.array_equal(seg_base, [0, 4, 5, 7])
    assert np.array_equal(so_g, [0, 10240, 20480, 30720, 35840, 35840, 46080, 56320])
    assert gc.split_segments(seg_base, [0, 3, 4, 5, 6]) == [[0, 3], [0], [0, 1]]
    assert gc.split_segments(seg_base, []) == [[], [], []]
    with pytest.raises(ValueError, match="out of range"):
        gc.split_segments(seg_base, [7])
    with pytest.raises(ValueError, match="out of range"):
        gc.split_segments(seg_base, [-1])


def test_corpus_ranges_map_to_shard_segments():
    from hmse_amd import gc
    _, so_g, seg_base = gc.shard_segments(_store(), _cfg())
    # shard 2 starts at byte 35840: its second segment is global segment 6
    segs = gc.segments_of_ranges(so_g, [(35840 + SEG, 20480 - SEG)])
    assert segs == [6] and gc.split_segments(seg_base, segs) == [[], [], [1]]
    # the last partial segment of shard 0 and the first of shard 2, in one range across the empty shard
    segs = gc.segments_of_ranges(so_g, [(30720, 35840 + SEG - 30720)])
    assert gc.split_segments(seg_base, segs)[0] == [3] and gc.split_segments(seg_base, segs)[2] == [0]
    with pytest.raises(ValueError, match="between segment boundaries 35840 and 46080"):
        gc.segments_of_ranges(so_g, [(35840, 100)])


def test_per_shard_seg_off():
    from hmse_amd import gc
    st = _store()
    sos, so_g, seg_base = gc.shard_segments(st, _cfg(), seg_off=[np.array([0, 5120, 35840]), None, np.array([0, 20480])])
    assert np.array_equal(seg_base, [0, 2, 3, 4]) and np.array_equal(so_g, [0, 5120, 35840, 35840, 56320])
    with pytest.raises(ValueError, match="one segment table per shard"):
        gc.shard_segments(st, _cfg(), seg_off=[None, None])
    with pytest.raises(ValueError, match="misses segment boundary"):
        gc.shard_segments(st, _cfg(), seg_off=[np.array([0, 5000, 35840]), None, None])


def test_refusals_before_device_work():
    from hmse_amd import gc
    st = _store()
    with pytest.raises(ValueError, match="out of range"):
        gc.drop_segments(st, [7], _cfg(), DEV)
    with pytest.raises(ValueError, match="segment-aligned"):
        gc.drop_ranges(st, [(100, SEG)], _cfg(), DEV)
    with pytest.raises(ValueError, match="one band-table sidecar per shard"):
        gc.drop_segments(st, [0], _cfg(), DEV, band_tables=[b"", b""])
    with pytest.raises(ValueError, match="layer"):
        gc.drop_segments(st, [0], _cfg(layers=0x6), DEV)
    # a multi-rank stream store
    ms = []
    for m in st.shards:
        pc = np.zeros(1, PIECE_DTYPE)
        pc["g0"], pc["n"] = m.chunk_base, len(m.chunk_map)
        ms.append(Manifest(m.lba_unit, m.index, m.chunk_map, m.pointers, m.blob, m.shard, m.n_shards, m.chunk_base, None, pc))
    with pytest.raises(ValueError, match="pieces"):
        gc.drop_segments(Store(ms), [0], _cfg(), DEV)
    # one unmerged part
    with pytest.raises(ValueError, match="merge_manifests"):
        gc.drop_segments(st.shards[2], [0], _cfg(), DEV)
    # shards out of order / wrong chunk bases
    with pytest.raises(ValueError, match="merge_manifests"):
        gc.drop_segments(Store([st.shards[0], st.shards[2], st.shards[1]]), [0], _cfg(), DEV)
    bad = Manifest(1, st.shards[2].index, st.shards[2].chunk_map, st.shards[2].pointers, st.shards[2].blob, 2, 3, 7)
    with pytest.raises(ValueError, match="starts at chunk 7"):
        gc.drop_segments(Store([st.shards[0], st.shards[1], bad]), [0], _cfg(), DEV)


def test_refuses_a_shard_whose_map_disagrees_with_its_index():
    from hmse_amd import gc
    st = _store()
    m = st.shards[2]
    cmap = m.chunk_map.copy()
    cmap["kind"][3] = KIND_POINTER                        # a stored slot without its own chunk
    st.shards[2] = Manifest(1, m.index, cmap, m.pointers, m.blob, 2, 3, m.chunk_base)
    with pytest.raises(ValueError, match="shard 2's index and chunk map disagree"):
        gc.drop_segments(st, [0], _cfg(), DEV)
    cmap = m.chunk_map.copy()
    cmap["shard"][0] = 9
    st.shards[2] = Manifest(1, m.index, cmap, m.pointers, m.blob, 2, 3, m.chunk_base)
    with pytest.raises(ValueError, match="disagree|outside"):
        gc.drop_segments(st, [0], _cfg(), DEV)


def test_merged_shards_is_the_one_store_check():
    """manifest.merged_shards: what GC and near-duplicate search refuse, what scrub (lenient) leaves to its report, and the prefix."""
    import dataclasses
    from hmse_amd.manifest import PTR_UNRESOLVED, REMOTE_BASE_DTYPE, merged_shards
    st = _store()
    lone = _shard(5, 0, 1, 0)
    for lenient in (False, True):
        assert merged_shards(st, "x", lenient) == st.shards and merged_shards(lone, "x", lenient) == [lone]
        with pytest.raises(ValueError, match="^who: shard 2 of 3 is one part of a sharded store: merge_manifests"):
            merged_shards(st.shards[2], "who", lenient)
        with pytest.raises(ValueError, match="^who: a Manifest or a Store, not bytes"):
            merged_shards(b"", "who", lenient)
        with pytest.raises(ValueError, match="shard 1 is manifest shard 2 of 3: not a merged store of 3 shards"):
            merged_shards(Store([st.shards[0], st.shards[2], st.shards[1]]), "x", lenient)
        with pytest.raises(ValueError, match="remote_bases"):
            merged_shards(dataclasses.replace(lone, remote_bases=np.zeros(1, REMOTE_BASE_DTYPE)), "x", lenient)
        ptr = np.zeros(1, POINTER_DTYPE)
        ptr["flags"] = PTR_UNRESOLVED
        with pytest.raises(ValueError, match="^who: the store has unresolved cross-shard pointers"):
            merged_shards(Store([st.shards[0], dataclasses.replace(st.shards[1], pointers=ptr), st.shards[2]]), "who", lenient)
    # only the readers of the (shard, local) chunk order refuse these three
    moved = Store([st.shards[0], st.shards[1], dataclasses.replace(st.shards[2], chunk_base=7)])
    pc = np.zeros(1, PIECE_DTYPE)
    streamed = Store([dataclasses.replace(m, pieces=pc) for m in st.shards])
    remote = Store([dataclasses.replace(lone, remote_bases=np.zeros(1, REMOTE_BASE_DTYPE))])
    for bad, what in ((moved, "starts at chunk 7, not 35"), (streamed, "pieces"), (remote, "remote_bases")):
        with pytest.raises(ValueError, match=what):
            merged_shards(bad, "x")
        assert merged_shards(bad, "x", lenient=True) == bad.shards
