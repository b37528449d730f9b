"""GPU: multi-member gzip / BGZF imported (hmse_amd.gunzip; hmse_gzip_candidates, hmse_gzip_measure).  The oracle is stock zlib — the
chain of zlib.decompressobj(wbits=31) of tests/gunzip_ref.py — and the pure-Python byte filter: the same members, the same bytes,
accepted if and only if the chain accepts.  Per kernel on synthetic buffers, on poisoned / misaligned / guarded memory (tests/arena.py),
on members of every level, strategy, size class and header, on damaged files, and round the loop with hmse_amd.export on the stores of
tests/test_gpu_export.py."""
import gzip
import io
import os
import sys
import zlib

import numpy as np
import pytest

import arena as A
import gunzip_ref as ref

pytestmark = pytest.mark.gpu

KIB = 1 << 10
SEG = 256 * KIB
TILE = 16384                    # positions per workgroup of the candidate passes; a thread tests 16, a trip of the workgroup 4096


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev, dt=None):
    import torch
    a = np.ascontiguousarray(np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else a)
    t = torch.from_numpy(a.copy())
    return (t if dt is None else t.to(dt)).to(dev)


def _cands(blob, dev, cap=None):
    """-> (written entries, count, the whole output tensor) of ops.gzip_candidates into a poisoned int64[cap + 2]"""
    import torch
    from hmse_amd import ops
    want = ref.candidates(blob)
    cap = len(want) if cap is None else cap
    out = torch.full((cap + 2,), -7, dtype=torch.int64, device=dev)
    got, count = ops.gzip_candidates(_t(blob, dev), cap, out=out[:cap])
    return out.tolist(), count


# ---- hmse_gzip_candidates -------------------------------------------------------------------------------------------------------------------
def _planted(n, at, seed):
    d = bytearray(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes().replace(b"\x1f\x8b", b".."))
    for p, flg in at:
        d[p: p + 4] = b"\x1f\x8b\x08" + bytes([flg])
    return bytes(d[:n])


@pytest.mark.parametrize("boundary", [16, 4096, TILE, 2 * TILE], ids=["thread", "trip", "tile", "tile2"])
def test_the_magic_straddles_a_boundary_at_each_split_point(boundary, dev):
    n = 3 * TILE + 777
    for split in (0, 1, 2, 3, 4):                                                      # bytes of the four in front of the boundary
        blob = _planted(n, [(boundary - split, 0x08), (5, 0), (n - 20, 0x1F)], seed=boundary + split)
        want = ref.candidates(blob)
        assert boundary - split in want and n - 20 in want
        out, count = _cands(blob, dev)
        assert count == len(want) and out == want + [-7, -7]


@pytest.mark.parametrize("n", [0, 1, 19, 20, 21, 35, 36, 37, TILE + 19, TILE + 20])
def test_the_last_position_with_room_and_tiny_buffers(n, dev):
    blob = (b"\x1f\x8b\x08\x00" * (n // 4 + 1))[:n]
    want = ref.candidates(blob)
    assert len(want) == (0 if n < 20 else (n - 20) // 4 + 1)
    out, count = _cands(blob, dev)
    assert count == len(want) and out == want + [-7, -7]
    if n >= 20:                                                                        # n - 20 is a candidate, n - 19 is not
        for p, there in ((n - 20, [n - 20]), (n - 19, [])):
            one = _planted(n, [(p, 0)], seed=n)
            assert ref.candidates(one) == there and _cands(one, dev, 3) == (there + [-7] * (5 - len(there)), len(there))


def test_nothing_but_magic_with_cap_below_and_at_the_count(dev):
    import torch
    from hmse_amd import ops
    n = 2 * TILE + 4 * 100 + 3
    blob = (b"\x1f\x8b\x08\x00" * (n // 4 + 1))[:n]
    want = ref.candidates(blob)
    assert len(want) == (n - 20) // 4 + 1 > 2 * TILE // 4
    for cap in (len(want), len(want) - 1, 5000, 1, 0):
        out, count = _cands(blob, dev, cap)
        assert count == len(want) and out == want[:cap] + [-7, -7], cap                # the total, the first cap, nothing behind them
    status = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)              # the status bit: the entry point clears the word itself
    meta = torch.full((1,), -1, dtype=torch.int64, device=dev)
    d, ws = _t(blob, dev), torch.empty(ops.gzip_workspace_bytes(n), dtype=torch.uint8, device=dev)
    for cap, bit in ((len(want), 0), (len(want) - 1, 1)):
        ops._call("hmse_gzip_candidates", d, n, torch.empty(cap, dtype=torch.int64, device=dev), cap, meta, status, ws, ws.numel())
        assert status.tolist() == [bit, 0x5A5A5A5A] and meta.tolist() == [len(want)]
    # reserved FLG bits and the other method bytes are no candidates
    blob = b"".join(b"\x1f\x8b" + bytes([m, f]) for m in (7, 8, 9) for f in range(256)) + bytes(20)
    assert _cands(blob, dev)[0][:-2] == ref.candidates(blob) == [4 * (256 + f) for f in range(32)]


# ---- measure + chain against zlib ------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 70, 32767, 32768, 32769, 65536, 200_000]
LEVELS = [0, 1, 6, 9]
STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE]


@pytest.fixture(scope="module")
def corpus():
    return ref.text(100, (1 << 20) + 5)


def _same(imp, blob, raws):
    """the import equals the zlib chain: members, bytes, cuts, offsets, CRC"""
    members = ref.chain(blob)
    assert [r for _, _, r in members] == raws
    assert imp.n_members == len(members) and imp.raw.cpu().numpy().tobytes() == b"".join(raws)
    assert imp.cuts.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.int64).tolist()
    assert imp.member_off.tolist() == [o for o, _, _ in members] + [len(blob)]
    assert imp.crc32 == zlib.crc32(b"".join(raws)) and imp.n_candidates >= imp.n_members


@pytest.mark.parametrize("level", LEVELS)
def test_members_of_every_strategy_and_size(level, corpus, dev):
    import torch
    from hmse_amd import gunzip
    raws, parts = [], []
    for si, strategy in enumerate(STRATEGIES):
        for k, n in enumerate(SIZES):
            a = (7919 * (si * 8 + k + level)) % 50_000
            raws.append(corpus[a: a + n])
            parts.append(ref.member(raws[-1], level, strategy, mtime=k))
    if level == 6:                                                                     # and one of 1 MiB
        raws.append(corpus[: 1 << 20])
        parts.append(ref.member(raws[-1], 6))
    blob = b"".join(parts)
    imp = gunzip.from_gzip(blob, dev)
    _same(imp, blob, raws)
    assert imp.raw.is_cuda and imp.raw.dtype == torch.uint8 and imp.cuts.dtype == torch.int64 and imp.n_bgzf == 0
    if level == 0:                                                                     # stored blocks show the corpus: it holds no magic
        assert imp.n_candidates == imp.n_members
    # the same through the other kinds of source
    if level == 1:
        for src in (np.frombuffer(blob, np.uint8), _t(blob, dev), torch.from_numpy(np.frombuffer(blob, np.uint8).copy())):
            assert torch.equal(gunzip.from_gzip(src, dev).raw, imp.raw)


def test_headers_of_every_combination_and_a_path(corpus, dev, tmp_path):
    from hmse_amd import gunzip, ops
    raws, parts = [], []
    for extra in (None, b"", b"AB\x03\x00xyzCD\x00\x00", b"BD\x02\x00\x05\x00" + b"Q" * 300):     # none, XLEN 0, subfields that are no BC
        for name in (None, b"name of a file.txt"):
            for comment in (None, b"", b"a comment " * 30):
                for hcrc in (False, True):
                    raws.append(corpus[len(parts) * 100: len(parts) * 100 + 500 + len(parts)])
                    parts.append(ref.member(raws[-1], 6, extra=extra, name=name, comment=comment, hcrc=hcrc, mtime=len(parts)))
    blob = b"".join(parts)
    (tmp_path / "many.gz").write_bytes(blob)
    imp = gunzip.from_gzip(tmp_path / "many.gz", dev)
    _same(imp, blob, raws)
    assert imp.n_members == 48 and gzip.decompress(blob) == b"".join(raws)
    # the measure kernel by itself against the reference, candidate by candidate — also at offsets that are no members
    offs = sorted(set(imp.member_off.tolist()[:-1] + [3, len(blob) - 19, len(blob) - 20, len(blob), len(blob) + 5]))
    so, end, rl, crc, fl = (v.tolist() for v in ops.gzip_measure(_t(blob, dev), _t(np.array(offs, np.int64), dev)))
    for k, p in enumerate(offs):
        m = ref.measure(blob, p)
        assert (fl[k] & 3) == (m["flags"] & 3) and (end[k], rl[k], crc[k] & 0xFFFFFFFF) == (m["end"], m["raw_len"], m["crc"]), (k, p)
        if m["valid"]:
            assert so[k] == m["stream_off"]
        else:
            assert fl[k] >> 2 in (1, 2, 3, 4) and (m["why"] not in (ref.WHY_HEADER, ref.WHY_LENGTH) or fl[k] >> 2 == m["why"]), (k, p, fl[k])


def test_the_nested_file(dev):
    from hmse_amd import gunzip
    blob, raws = ref.nested_case()
    imp = gunzip.from_gzip(blob, dev)
    _same(imp, blob, raws)
    assert imp.n_candidates == len(ref.candidates(blob)) > imp.n_members == 4


def test_bgzf_blocks_take_the_fast_path(corpus, dev):
    from hmse_amd import gunzip
    import export_ref
    raws = [corpus[i * 60_000: i * 60_000 + n] for i, n in enumerate((65536, 1, 0, 40_000, 65535))]
    blob = b"".join(ref.bgzf_member(r) for r in raws) + export_ref.BGZF_EOF
    imp = gunzip.from_gzip(blob, dev)
    _same(imp, blob, raws + [b""])
    assert imp.n_bgzf == imp.n_members == 6
    mixed = ref.member(raws[3], 9) + ref.bgzf_member(raws[1]) + ref.bgzf_member(raws[3], bsize=20) + ref.member(b"")      # BSIZE + 1 < header + 10: ignored
    imp = gunzip.from_gzip(mixed, dev)
    _same(imp, mixed, [raws[3], raws[1], raws[3], b""])
    assert imp.n_bgzf == 1


# ---- refusals that name the offset -----------------------------------------------------------------------------------------------------------
def test_refusals_name_member_and_offset(corpus, dev):
    from hmse_amd import gunzip
    raws = [corpus[:3000], corpus[3000: 3070], corpus[5000: 45_000]]
    mem = [ref.member(raws[0], 6, name=b"one", hcrc=True), ref.member(raws[1], 1), ref.member(raws[2], 9)]
    good = b"".join(mem)
    o1, o2 = len(mem[0]), len(mem[0]) + len(mem[1])
    _same(gunzip.from_gzip(good, dev), good, raws)

    def refused(blob, member, offset, match, zlib_too=True):
        assert (ref.outcome(blob) is None) == zlib_too                                 # zlib refuses it too (all but the lying BSIZE)
        with pytest.raises(gunzip.GunzipError, match=match) as e:
            gunzip.from_gzip(blob, dev)
        assert (e.value.member, e.value.offset) == (member, offset), str(e.value)

    refused(b"junk" + good, 0, 0, "does not start with a gzip member")
    refused(b"\0" * 40, 0, 0, "does not start with a gzip member")
    refused(good + b"\0", 3, len(good), "1 bytes behind member 2")
    refused(good + b"trailing junk, longer than a member", 3, len(good), "bytes behind member 2")
    refused(good[:-1], 2, o2, "not a valid member")
    refused(good[:o2 + 200], 2, o2, "not a valid member")
    reserved = bytearray(good); reserved[o1 + 3] |= 0x20
    refused(bytes(reserved), 1, o1, "bytes behind member 0")                           # no candidate there: zlib's "unknown header flags set"
    fhcrc = bytearray(good); fhcrc[4] ^= 1                                              # MTIME lies under the header CRC
    refused(bytes(fhcrc), 0, 0, r"not a valid member \(header\)")
    isize = bytearray(good); isize[o2 - 4] ^= 1
    refused(bytes(isize), 1, o1, r"not a valid member \(length\)")
    stream = bytearray(good); stream[o2 + 10] = 0x07                                   # block type 3
    refused(bytes(stream), 2, o2, r"not a valid member \(stream\)")
    crc = bytearray(good); crc[o2 - 8] ^= 0x80
    refused(bytes(crc), 1, o1, "CRC-32 mismatch")
    assert ref.outcome(bytes(crc)) is None
    imp = gunzip.from_gzip(bytes(crc), dev, verify=False)                              # accepted as recorded
    assert imp.raw.cpu().numpy().tobytes() == b"".join(raws) and imp.crc32 != zlib.crc32(b"".join(raws))
    # a BSIZE that disagrees with its stream: believed by the chain, refused when the block is decoded (zlib does not look at it)
    z = [ref.bgzf_member(raws[1]), ref.bgzf_member(raws[0]), ref.bgzf_member(raws[1])]
    lie = z[0] + ref.bgzf_member(raws[0], bsize=len(z[1]) + len(z[2]) - 1)[:len(z[1])] + z[2]       # block 1 claims block 2 as well
    assert ref.outcome(lie) == [raws[1], raws[0], raws[1]]
    refused(lie, 1, len(z[0]), "BSIZE disagrees", zlib_too=False)
    # the limits: ValueError, nothing decoded
    with pytest.raises(ValueError, match=f"decode to {sum(map(len, raws))} bytes, max_bytes is {sum(map(len, raws)) - 1}") as e:
        gunzip.from_gzip(good, dev, max_bytes=sum(map(len, raws)) - 1)
    assert not isinstance(e.value, gunzip.GunzipError)
    assert gunzip.from_gzip(good, dev, max_bytes=sum(map(len, raws))).n_members == 3
    with pytest.raises(ValueError, match="3 positions carry the gzip magic, max_candidates is 2"):
        gunzip.from_gzip(good, dev, max_candidates=2)
    assert gunzip.from_gzip(good, dev, max_candidates=3).n_candidates == 3
    assert gunzip.from_gzip(b"", dev).n_members == 0


# ---- mutation parity -------------------------------------------------------------------------------------------------------------------------
def test_two_hundred_mutations_end_as_zlib_ends_them(dev):
    from hmse_amd import gunzip
    accepted = refused = 0
    for blob, at in ref.mutations():
        want = ref.outcome(blob)
        try:
            imp = gunzip.from_gzip(blob, dev)
            got = [imp.raw[a:b].cpu().numpy().tobytes() for a, b in zip(imp.cuts.tolist()[:-1], imp.cuts.tolist()[1:])]
        except gunzip.GunzipError:
            got = None
        assert got == want, (at, blob[at])
        accepted += want is not None
        refused += want is None
    assert accepted >= 10 and refused >= 10 and accepted + refused == 200


# ---- round trip with export ------------------------------------------------------------------------------------------------------------------
def _store_input():
    """the recipe of tests/test_gpu_export.py::_store_input"""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import variants_dataset
    from hmse_amd import corpus
    w = corpus.wiki_synth(1 << 20, seed=42)
    return np.concatenate([w[: 640 * KIB], w[100_000: 450_000], variants_dataset(w)[:300_000], np.full(100_000, ord("e"), np.uint8)])


def _ragged_seg_off(n, dev):
    import torch
    off = [0]
    for s in [SEG, 1, 2, 3, 70, SEG, 1, 70, 3, 2]:
        off.append(off[-1] + s)
    while off[-1] < n:
        off.append(min(off[-1] + SEG, n))
    return torch.tensor(off, dtype=torch.int64, device=dev)


@pytest.fixture(scope="module")
def store(dev):
    import torch
    from hmse_amd import IngestConfig, ingest, manifest
    cfg = IngestConfig(seg_size=SEG)
    data = _store_input()
    res = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg, _ragged_seg_off(data.size, dev))
    packed = manifest.build_manifest(res).to_bytes()
    return cfg, data, manifest.Manifest.from_bytes(packed), packed


@pytest.mark.parametrize("bgzf", [False, True], ids=["gzip", "bgzf"])
def test_round_trip_with_export(store, dev, bgzf):
    import torch
    from hmse_amd import KIND_DELTA, KIND_POINTER, export, gunzip, ingest, manifest
    cfg, data, m, packed = store
    kinds, lens = m.chunk_map["kind"], m.chunk_map["raw_length"]
    assert (kinds == KIND_POINTER).sum() > 0 and (kinds == KIND_DELTA).sum() > 0 and {1, 2, 3, 70} <= set(lens.tolist())
    x = export.to_gzip(m, dev, cfg, bgzf=bgzf)
    imp = gunzip.from_gzip(x.data, dev)                                                # the device tensor where it is
    assert imp.raw.cpu().numpy().tobytes() == data.tobytes() and imp.crc32 == x.crc32 == zlib.crc32(data.tobytes())
    n_chunks = x.member_off.numel() - 1
    if bgzf:                                                                           # the EOF block is one more, empty member
        assert imp.n_members == n_chunks + 1 == imp.n_bgzf and imp.cuts.tolist() == x.cuts.tolist() + [data.size]
        assert imp.member_off.tolist() == x.member_off.tolist() + [x.data.numel()]
    else:
        assert imp.n_members == n_chunks and imp.n_bgzf == 0 and torch.equal(imp.cuts, x.cuts) and torch.equal(imp.member_off, x.member_off)
    # the imported bytes feed the ingest as the corpus does
    res = ingest.ingest_shard(imp.raw, cfg, _ragged_seg_off(data.size, dev))
    assert manifest.build_manifest(res).to_bytes() == packed


def test_a_two_shard_store_and_a_file_python_appended_to(dev):
    import torch
    from hmse_amd import IngestConfig, corpus, export, gunzip, ingest, manifest
    cfg = IngestConfig(seg_size=SEG)
    data = corpus.wiki_synth(1 << 20, seed=42).copy()
    data[640 * KIB + 5000: 900 * KIB + 5000] = data[5000: 260 * KIB + 5000]        # the second shard repeats bytes of the first
    shards = [torch.from_numpy(data[: 512 * KIB]).to(dev), torch.from_numpy(data[512 * KIB:]).to(dev)]
    parts = [manifest.build_manifest(r, i, 2) for i, r in enumerate(ingest.ingest_shards_local(shards, cfg))]
    st = manifest.Store.from_bytes(manifest.merge_manifests(parts).to_bytes())
    for bgzf in (False, True):
        x = export.to_gzip(st, dev, bgzf=bgzf)
        imp = gunzip.from_gzip(x.data, dev)
        assert imp.raw.cpu().numpy().tobytes() == data.tobytes() and imp.crc32 == x.crc32
        assert imp.cuts.tolist()[: x.cuts.numel()] == x.cuts.tolist() and imp.n_members == x.member_off.numel() - 1 + int(bgzf)
    buf, pieces = io.BytesIO(), [data[:300_000].tobytes(), data[300_000: 300_007].tobytes(), data[400_000: 1_000_000].tobytes()]
    for i, p in enumerate(pieces):                                                     # written once, appended to twice
        with gzip.GzipFile(filename="rotation.log", fileobj=buf, mode="ab", compresslevel=(6, 9, 1)[i], mtime=1_700_000_000 + i) as f:
            f.write(p)
    imp = gunzip.from_gzip(buf.getvalue(), dev)
    _same(imp, buf.getvalue(), pieces)


# ---- dispatch --------------------------------------------------------------------------------------------------------------------------------
def test_enough_tiny_members_for_the_lane_per_stream_decoder(corpus, dev):
    from hmse_amd import gunzip
    n_mem = 49_152 + 300                                                               # hmse_l1_inflate goes wide by itself from 49 152 streams on
    lens = np.random.default_rng(31).integers(0, 48, n_mem)
    lens[:5] = [0, 1, 47, 0, 2]
    starts = np.concatenate([[0], np.cumsum(lens)])
    raws = [corpus[a: a + l] for a, l in zip(starts[:-1].tolist(), lens.tolist())]
    blob = b"".join(ref.member(r, (1, 6, 9, 0)[k & 3], zlib.Z_FIXED if k % 7 == 0 else zlib.Z_DEFAULT_STRATEGY) for k, r in enumerate(raws))
    imp = gunzip.from_gzip(blob, dev)
    _same(imp, blob, raws)
    assert imp.n_members == n_mem >= 49_152


# ---- on poisoned, misaligned, guarded memory -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,mis", [("random", 3), ("ones", 0), ("zero", 13)])
def test_kernels_read_their_data_and_write_their_declared_outputs_only(pattern, mis, corpus, dev, monkeypatch):
    import torch
    from hmse_amd import gunzip, ops
    ar = A.Arena(dev, pattern, seed=41).install(monkeypatch, distrust_zeros=True, byte_misalign=mis)
    raws = [corpus[:20_000], b"", corpus[500: 570], corpus[30_000: 65_000]]
    last = ref.member(corpus[7000: 9000], 6, name=b"cut")
    blob = ref.member(raws[0], 6, name=b"n", hcrc=True) + ref.bgzf_member(raws[1]) + ref.member(raws[2], 0) + ref.bgzf_member(raws[3]) + last[:-30]
    # behind the declared end: the rest of the cut member, a whole member, magic at every offset of the last 19 positions
    tail = last[-30:] + ref.member(b"behind the end") + b"\x1f\x8b\x08\x00" * 8
    data, both = ar.place_with_tail(np.frombuffer(blob, np.uint8).copy(), np.frombuffer(tail, np.uint8).copy(), misalign=mis)
    n = len(blob)
    want = ref.candidates(blob)
    assert len(want) == 5 and len(ref.candidates(blob + tail)) > 6
    cand, count = ops.gzip_candidates(data, 8)
    assert count == 5 and cand[:5].tolist() == want
    so, end, rl, crc, fl = ops.gzip_measure(data, cand[:5].contiguous())
    ms = [ref.measure(blob, p) for p in want]
    assert [f & 3 for f in fl.tolist()] == [1, 3, 1, 3, 0] == [m["flags"] & 3 for m in ms] and fl.tolist()[4] >> 2 in (2, 4)
    assert end.tolist() == [m["end"] for m in ms] and rl.tolist() == [m["raw_len"] for m in ms]
    assert [c & 0xFFFFFFFF for c in crc.tolist()] == [m["crc"] for m in ms] and so.tolist()[:4] == [m["stream_off"] for m in ms[:4]]
    with pytest.raises(gunzip.GunzipError, match="not a valid member") as e:           # the cut member ends the chain, whatever lies behind n
        gunzip.from_gzip(data, dev)
    assert (e.value.member, e.value.offset) == (4, want[4])
    whole = ar.place(np.frombuffer(blob[: want[4]], np.uint8).copy(), misalign=mis)
    imp = gunzip.from_gzip(whole, dev)
    assert imp.raw.cpu().numpy().tobytes() == b"".join(raws) and imp.n_bgzf == 2 and imp.raw.data_ptr() % 16 == mis
    ar.check()
