"""CPU: hmse_amd.scrub's refusals, its host-side metadata plan and report plumbing, and the host reference (tests/scrub_ref.py) on tiny
hand-written manifests (stock zlib records: FULL, DELTA chains, POINTERs)."""
import hashlib
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _deflate(raw: bytes, zdict: bytes | None = None) -> bytes:
    c = zlib.compressobj(9, zlib.DEFLATED, -15, zdict=zdict) if zdict else zlib.compressobj(9, zlib.DEFLATED, -15)
    return c.compress(raw) + c.flush()


def tiny(unit: int = 1):
    """A one-shard manifest: records 0 (FULL), 1 (DELTA on 0), 2 (DELTA on 1), 3 (FULL); chunks 0, 1, 2, POINTER->0, 3, POINTER->2."""
    from hmse_amd.config import KIND_DELTA, KIND_FULL, KIND_POINTER
    from hmse_amd.manifest import CHUNK_INDEX_DTYPE, MAP_DTYPE, POINTER_DTYPE, Manifest
    rng = np.random.default_rng(1)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 8), dtype=np.uint8)) for _ in range(60)]
    base = b" ".join(words[i] for i in rng.integers(0, 60, 700))[:3000]
    v1 = base[:1000] + b"EDIT" + base[1004:]
    v2 = v1[:2000] + b"MORE" + v1[2004:]
    other = bytes(rng.integers(0, 256, 1500, dtype=np.uint8))
    raws = [base, v1, v2, other]
    kinds = [KIND_FULL, KIND_DELTA, KIND_DELTA, KIND_FULL]
    dic = [-1, 0, 1, -1]
    recs, off = [], 0
    lba, ln = [], []
    for k, r in enumerate(raws):
        s = _deflate(r, raws[dic[k]] if dic[k] >= 0 else None)
        rec = s if kinds[k] == KIND_FULL else b"\0" * 8 + s
        lba.append(off // unit); ln.append(len(rec))
        recs.append(rec)
        off += -(-len(rec) // unit) * unit
    blob = np.zeros(off, np.uint8)
    for k, rec in enumerate(recs):
        if kinds[k] == KIND_DELTA:
            rec = struct.pack("<IHH", lba[dic[k]], ln[dic[k]], ln[k] - 8) + rec[8:]
        blob[lba[k] * unit: lba[k] * unit + len(rec)] = np.frombuffer(rec, np.uint8)
    idx = np.zeros(4, CHUNK_INDEX_DTYPE)
    idx["lba"], idx["length"], idx["refcount"] = lba, ln, 1
    idx["sha256"] = [np.frombuffer(hashlib.sha256(r).digest(), np.uint8) for r in raws]
    order = [0, 1, 2, 0, 3, 2]
    cm = np.zeros(6, MAP_DTYPE)
    cm["slot"] = order
    cm["raw_length"] = [len(raws[s]) for s in order]
    cm["kind"] = [kinds[0], kinds[1], kinds[2], KIND_POINTER, kinds[3], KIND_POINTER]
    ptr = np.zeros(2, POINTER_DTYPE)
    ptr["target_lba"] = [lba[0], lba[2]]; ptr["target_length"] = [ln[0], ln[2]]; ptr["flags"] = KIND_POINTER
    m = Manifest(unit, idx, cm, ptr, blob)
    return m, b"".join(raws[s] for s in order)


def test_reference_on_a_clean_tiny_manifest():
    import scrub_ref
    from hmse_amd import manifest
    m, data = tiny()
    assert manifest.reconstruct(m) == data
    ref = scrub_ref.scrub_ref(m)
    assert not ref["record_status"].any() and (ref["record_root"] == -1).all() and (ref["chunk_root"] == -1).all()
    assert ref["ranges"].shape == (0, 2) and ref["padding_bytes"] == 0 and ref["roots"] == {}


def test_reference_attributes_a_dictionary_chain_to_its_root():
    import scrub_ref
    from hmse_amd import scrub as S
    m, data = tiny()
    m.blob[int(m.index["lba"][0]) + 40] ^= 0x55                         # the head of the chain 0 <- 1 <- 2
    ref = scrub_ref.scrub_ref(m)
    st = ref["record_status"]
    assert st[0] & (S.STREAM | S.DIGEST) and st[1] == S.DICTIONARY and st[2] == S.DICTIONARY and st[3] == 0
    assert list(ref["record_root"]) == [0, 0, 0, -1]
    assert list(ref["chunk_root"]) == [0, 0, 0, 0, -1, 0]
    lens = m.chunk_map["raw_length"].astype(np.int64)
    assert ref["ranges"].tolist() == [[0, int(lens[:4].sum())], [int(lens[:5].sum()), int(lens[5])]]
    assert ref["roots"] == {0: [3, 5, int(lens.sum() - lens[4])]}


def test_reference_flags_headers_and_padding():
    import scrub_ref
    from hmse_amd import manifest, scrub as S
    m, data = tiny(unit=16)
    assert manifest.reconstruct(m) == data
    o = int(m.index["lba"][1]) * 16
    m.blob[o + 6] ^= 1                                                   # delta_length
    m.blob[int(m.index["lba"][0]) * 16 + int(m.index["length"][0])] = 7  # padding behind record 0 (unit 16: there is some)
    ref = scrub_ref.scrub_ref(m)
    assert list(ref["record_status"]) == [0, S.HEADER, 0, 0] and ref["padding_bytes"] == 1
    assert (ref["chunk_root"] == -1).all()
    m.blob[o] ^= 1                                                       # base_lba: no index entry
    ref = scrub_ref.scrub_ref(m)
    assert ref["record_status"][1] & S.STRUCTURE and ref["record_status"][2] == S.DICTIONARY and list(ref["record_root"]) == [-1, 1, 1, -1]


def test_plan_reports_inconsistent_metadata():
    from hmse_amd import scrub as S
    m, _ = tiny()
    m.pointers["target_lba"][1] += 1                                     # pointer record disagrees with the index
    m.chunk_map["slot"][4] = 9                                           # an own chunk names no record; record 3 is named by nobody
    p = S.plan(m)
    assert p.chunk_slot.tolist() == [0, 1, 2, 0, -1, -1]
    assert p.meta.tolist() == [0, 0, 0, S.METADATA]


def test_refusals():
    import dataclasses
    import torch
    from hmse_amd import IngestConfig, manifest, scrub
    m, _ = tiny()
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="merge_manifests"):
        scrub.scrub(dataclasses.replace(m, n_shards=2), dev)
    p2 = dataclasses.replace(m, pointers=m.pointers.copy())
    p2.pointers["flags"][0] |= manifest.PTR_UNRESOLVED
    with pytest.raises(ValueError, match="unresolved"):
        scrub.scrub(p2, dev)
    with pytest.raises(ValueError, match="Manifest or a Store"):
        scrub.scrub(b"bytes", dev)
    with pytest.raises(ValueError, match="cfg"):
        scrub.scrub(m, dev, band_tables=[b""])
    st = manifest.Store([m])
    with pytest.raises(ValueError, match="one sidecar per shard"):
        scrub.scrub(st, dev, cfg=IngestConfig(), band_tables=[b"", b""])
    pieces = np.zeros(1, manifest.PIECE_DTYPE); pieces["n"] = len(m.chunk_map)
    with pytest.raises(ValueError, match="pieces"):
        scrub.scrub(manifest.Store([dataclasses.replace(m, pieces=pieces)]), dev, cfg=IngestConfig(), band_tables=[b""])
    with pytest.raises(ValueError, match="cfg"):
        scrub.repair(m, dev, sources=[(0, b"")])
    other = dataclasses.replace(m, index=m.index.copy())
    other.index["refcount"][0] += 1
    with pytest.raises(ValueError, match="metadata"):
        scrub.repair(m, dev, replicas=[other])
    with pytest.raises(ValueError, match="fill"):
        scrub.salvage(m, dev, fill=256)


def test_sidecar_parsing_and_report_plumbing():
    from hmse_amd import bandtable, scrub as S
    keys = np.arange(12, dtype=np.uint32).reshape(3, 4)
    sig = np.arange(3 * 128, dtype=np.uint32).reshape(3, 128)
    buf = bandtable.write_band_tables(keys, 16, signatures=sig)
    tables, k2, s2, bands, bits = S._split_sidecar(buf)
    assert np.array_equal(k2, keys) and np.array_equal(s2, sig) and bands == 4 and bits == 16 and buf.startswith(tables)
    assert S._split_sidecar(buf[:-4]) is None and S._split_sidecar(bandtable.write_band_tables(keys, 16)) is None
    assert S._split_sidecar(b"junk") is None
    rep = S.ScrubReport(np.array([0, S.DIGEST, S.DICTIONARY, S.HEADER], np.uint8), np.array([-1, 1, 1, -1]), np.array([-1, 1, 1, -2]),
                        np.array([[10, 30]]), np.zeros(2, S.ROOT_DTYPE), 0, 100)
    assert rep.digests_checked and "NOT checked" not in rep.summary()
    rep.roots[0] = (1, 0, 1, S.DIGEST, 2, 2, 20); rep.roots[1] = (S.MAP_BAD, -1, -1, S.METADATA, 0, 1, 10)
    assert not rep.lossless and not rep.clean and rep.damaged_records().tolist() == [1, 2]
    s = rep.summary()
    assert "DAMAGED" in s and "DIGEST" in s and "chunk map" in s and "30 of 100 bytes" in s
    ok = S.ScrubReport(np.array([S.HEADER], np.uint8), np.array([-1]), np.array([-1]), np.zeros((0, 2), np.int64), np.zeros(0, S.ROOT_DTYPE), 0, 5)
    assert "NOT checked" in S.ScrubReport(ok.record_status, ok.record_root, ok.chunk_root, ok.ranges, ok.roots, 0, 5,
                                          digests_checked=False).summary()
    assert ok.lossless and not ok.clean
    ok.record_status[0] = 0
    assert ok.clean
    ok.sidecar = {"usable": [True], "tables_ok": [True], "sig_bad": 1, "sig_unchecked": 0, "sig_status": np.ones(1, np.uint8)}
    assert not ok.clean
    assert S.flag_names(S.STREAM | S.HEADER) == "STREAM|HEADER" and S.flag_names(0) == "OK"


def test_cut_deep_is_one_limit_always_applied():
    """Cycles, chains behind them and records 2^16 or more links down are cut, whether or not every dictionary precedes its
    dependant; what is left is ordered by read.dependency_order without a ReadError, and the reference's plain walk agrees."""
    import scrub_ref
    from hmse_amd import scrub as S
    from hmse_amd.read import MAX_DELTA_DEPTH_LOG2, dependency_order
    assert not S.cut_deep(np.array([-1, 0, 1]), 16).any()
    assert S.cut_deep(np.array([2, 0, 1, -1, 3, 0]), 16).tolist() == [True, True, True, False, False, True]
    L = 1 << MAX_DELTA_DEPTH_LOG2
    chain = np.arange(-1, 70000 - 1)                                   # every dictionary precedes: no reordering needed, still cut
    d = S.cut_deep(chain, MAX_DELTA_DEPTH_LOG2)
    assert d.sum() == 70000 - L and not d[:L].any() and d[L:].all()
    fwd = chain.copy()
    fwd[0], fwd[69999] = 69999, -1                                     # one forward link: the chain's top is the last record
    d = S.cut_deep(fwd, MAX_DELTA_DEPTH_LOG2)
    assert np.array_equal(d, scrub_ref.deep(fwd, L)) and d.sum() == 70000 - L
    dependency_order(np.where(d, -1, fwd))                             # no ReadError once the deep records are cut
    with pytest.raises(Exception):
        dependency_order(fwd)


def test_pointer_raw_length_disagreeing_with_its_target_is_metadata():
    import scrub_ref
    from hmse_amd import scrub as S
    m, data = tiny()
    m.chunk_map["raw_length"][3] -= 5                                  # the POINTER to record 0
    p = S.plan(m)
    assert p.chunk_slot.tolist() == [0, 1, 2, -1, 3, 2] and not p.meta.any()
    ref = scrub_ref.scrub_ref(m)
    assert ref["chunk_root"].tolist() == [-1, -1, -1, -2, -1, -1] and not ref["record_status"].any()
    lens = m.chunk_map["raw_length"].astype(np.int64)
    assert ref["ranges"].tolist() == [[int(lens[:3].sum()), int(lens[3])]] and ref["roots"] == {-2: [0, 1, int(lens[3])]}


def test_reference_metadata_is_its_own_and_agrees_with_the_plan():
    import scrub_ref
    from hmse_amd import scrub as S
    m, _ = tiny()
    m.pointers["target_length"][0] += 1
    m.chunk_map["slot"][1] = 3                                         # record 1 unnamed, record 3 named twice
    m.chunk_map["raw_length"][5] += 2
    p = S.plan(m)
    meta, kind, raw_len, remote, slots, lens = scrub_ref.metadata(p)
    assert np.array_equal(meta, p.meta) and np.array_equal(kind, p.kind) and np.array_equal(raw_len, p.raw_len)
    assert np.array_equal(slots, p.chunk_slot) and np.array_equal(lens, p.chunk_len) and np.array_equal(remote, p.remote)
    assert slots.tolist() == [0, 3, 2, -1, 3, -1] and meta.tolist() == [0, S.METADATA, 0, S.METADATA]


def test_reference_counts_the_blob_of_a_shard_without_records_as_padding():
    import scrub_ref
    from hmse_amd.manifest import CHUNK_INDEX_DTYPE, MAP_DTYPE, POINTER_DTYPE, Manifest
    m = Manifest(1, np.zeros(0, CHUNK_INDEX_DTYPE), np.zeros(0, MAP_DTYPE), np.zeros(0, POINTER_DTYPE), np.array([0, 3, 0, 9], np.uint8))
    assert scrub_ref.scrub_ref(m)["padding_bytes"] == 2


def test_stream_pieces_that_do_not_tile_are_refused():
    import dataclasses
    from hmse_amd import manifest, scrub as S
    m, _ = tiny()
    pieces = np.zeros(1, manifest.PIECE_DTYPE); pieces["g0"] = 1; pieces["n"] = len(m.chunk_map)
    with pytest.raises(ValueError, match="refused"):
        S.plan(manifest.Store([dataclasses.replace(m, pieces=pieces)]))


def test_ops_wrappers_refuse_host_tensors():
    import torch
    from hmse_amd import ops
    x = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ops.HmseError):
        ops.scrub_records(torch.zeros(16, dtype=torch.uint8), x, x, x, x, x, x, x, x, x, x, 1, x)
    with pytest.raises(ops.HmseError):
        ops.scrub_attribute(x, x, x, x, x, False, x, x, 16)
    from hmse_amd import IngestConfig
    assert ops.workspace_bytes(ops.STAGE_SCRUB_ATTRIBUTE, 1000, IngestConfig()) > 4 * 4 * 1000
    assert ops.workspace_bytes(ops.STAGE_SCRUB_RECORDS, 1000, IngestConfig()) == 0          # the records pass takes no workspace
