"""GPU: a store exported as multi-member gzip / BGZF (hmse_amd.export; hmse_crc32, hmse_crc32_combine, hmse_gzip_members).  The oracle is
the standard library — zlib.crc32, gzip.decompress, zlib.decompress(wbits=31) — and tests/export_ref.py where no data can exist (lengths
above 2^32).  Per kernel on synthetic ranges and tables, on poisoned / misaligned / guarded memory (tests/arena.py), and on stores built
by the recipe of tests/test_gpu_approx.py: POINTER and DELTA records, tiny chunks of ragged segments, a two-shard merged store."""
import gzip
import os
import sys
import zlib
from dataclasses import asdict

import numpy as np
import pytest

import arena as A
import export_ref as ref

pytestmark = pytest.mark.gpu

KIB = 1 << 10
SEG = 256 * KIB
LENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 32767, 32768, 100_000, 1_000_003]
LENS += [1023, 1024, 1025, 8191, 8192, 8193, 16384, 16385]      # the kernel's own boundaries: the smallest strip (64 x 16 bytes), one and two tiles


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


def u32(t):
    return [int(v) & 0xFFFFFFFF for v in t.tolist()]


# ---- hmse_crc32 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ranges():
    """every length three times — random, 0x00, 0xFF — back to back behind 3 junk bytes, junk behind; zlib's CRCs, computed once"""
    rng = np.random.default_rng(11)
    parts, cuts = [rng.integers(1, 255, 3, dtype=np.uint8)], [3]
    for fill in ("random", 0x00, 0xFF):
        for n in LENS:
            parts.append(rng.integers(0, 256, n, dtype=np.uint8) if fill == "random" else np.full(n, fill, np.uint8))
            cuts.append(cuts[-1] + n)
    parts.append(rng.integers(1, 255, 5, dtype=np.uint8))
    data = np.concatenate(parts)
    want = [zlib.crc32(data[a:b].tobytes()) for a, b in zip(cuts[:-1], cuts[1:])]
    return data, np.array(cuts, np.int64), want


def test_crc32_of_many_ranges_equals_zlib(ranges, dev):
    import torch
    from hmse_amd import ops
    data, cuts, want = ranges
    assert cuts[0] % 4 == 3 and len(want) == 3 * len(LENS)
    got = ops.crc32(_t(data, dev), _t(cuts, dev))
    assert got.dtype == torch.int32 and u32(got) == want
    # one range over everything: hundreds of tiles
    whole = ops.crc32(_t(data, dev), _t(np.array([0, data.size], np.int64), dev))
    assert u32(whole) == [zlib.crc32(data.tobytes())]


def test_crc32_no_ranges_and_refused_cuts(ranges, dev):
    import torch
    from hmse_amd import ops
    data, cuts, want = ranges
    d = _t(data, dev)
    assert ops.crc32(d, _t(np.array([7], np.int64), dev)).numel() == 0                  # n_chunks = 0
    assert ops.crc32(d[:0], _t(np.array([0, 0, 0], np.int64), dev)).tolist() == [0, 0]    # no data, empty ranges
    for bad in (np.array([0, 10, 9, 20], np.int64), np.array([0, 10, data.size + 1], np.int64), np.array([5, 4], np.int64)):
        out = torch.full((bad.size - 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        with pytest.raises(ops.HmseError, match="descends or ends behind"):
            ops.crc32(d, _t(bad, dev), out=out)
        assert out.tolist() == [0x5A5A5A5A] * (bad.size - 1)                           # outputs untouched
    assert u32(ops.crc32(d, _t(np.array([0, 10, 10, data.size], np.int64), dev))) == [zlib.crc32(data[:10].tobytes()), 0, zlib.crc32(data[10:].tobytes())]


# ---- hmse_crc32_combine -------------------------------------------------------------------------------------------------------------------
def test_crc32_combine(dev):
    from hmse_amd import ops
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 3000, 1000)
    lens[rng.integers(0, 1000, 150)] = 0                                               # empty ranges, also first and last
    lens[0] = lens[-1] = 0
    data = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    crcs = np.array([zlib.crc32(data[a:b].tobytes()) for a, b in zip(cuts[:-1], cuts[1:])], np.uint32)
    got = ops.crc32_combine(_t(crcs.view(np.int32), dev), _t(lens.astype(np.int64), dev))
    assert got == zlib.crc32(data.tobytes())
    assert ops.crc32_combine(_t(crcs[:0].view(np.int32), dev), _t(lens[:0].astype(np.int64), dev)) == 0
    assert ops.crc32_combine(_t(crcs[:1].view(np.int32), dev), _t(lens[:1].astype(np.int64), dev)) == int(crcs[0])
    # lengths above 2^32 are exponents only: no such data is needed
    big = rng.integers(0, 1 << 45, 1000).astype(np.int64)
    big[::7] = 0
    big[5] = (1 << 32) - 1
    big[6] = 1 << 32
    c = rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
    assert ops.crc32_combine(_t(c.view(np.int32), dev), _t(big, dev)) == ref.combine(c.tolist(), big.tolist())
    # and the CRCs of hmse_crc32 themselves
    both = ops.crc32_combine(ops.crc32(_t(data, dev), _t(cuts, dev)), _t(lens.astype(np.int64), dev))
    assert both == zlib.crc32(data.tobytes())


# ---- hmse_gzip_members on poisoned, misaligned, guarded memory -----------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,mis", [("random", 3), ("ones", 0), ("zero", 13)])
def test_kernels_write_their_declared_outputs_only(pattern, mis, dev, monkeypatch):
    import torch
    from hmse_amd import ops
    ar = A.Arena(dev, pattern, seed=21).install(monkeypatch, distrust_zeros=True, byte_misalign=mis)
    rng = np.random.default_rng(22)
    raws = [rng.integers(97, 101, n, dtype=np.uint8).tobytes() for n in (0, 1, 70, 5000, 32768, 9000)]
    streams = []
    for r in raws:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        streams.append(co.compress(r) + co.flush())
    sel = [0, 1, 0, 1, 0, 1]
    srcs, src_off = [bytearray(b"\x11" * 5), bytearray(b"\x22" * 2)], []
    for s, w in zip(streams, sel):
        src_off.append(len(srcs[w]))
        srcs[w] += s + b"\x33" * 3                                                     # junk between the records
    raw_off = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.int64)
    raw_all, tail = ar.place_with_tail(np.frombuffer(b"".join(raws), np.uint8).copy(), rng.integers(0, 256, 64, dtype=np.uint8), misalign=mis)
    crc = ops.crc32(raw_all, ar.place(raw_off))
    assert u32(crc) == [zlib.crc32(r) for r in raws]
    slot = [2, 0, 5, 2, 1, 4, 3, 0, 2]
    for bgzf in (False, True):
        H = 18 if bgzf else 10
        member_off = np.concatenate([[0], np.cumsum([H + len(streams[r]) + 8 for r in slot])]).astype(np.int64)
        out = ops.gzip_members(ar.place(np.frombuffer(bytes(srcs[0]), np.uint8).copy(), misalign=mis), ar.place(np.frombuffer(bytes(srcs[1]), np.uint8).copy(), misalign=(mis + 5) % 16),
                               ar.place(np.array(src_off, np.int64)), ar.place(np.array([len(s) for s in streams], np.int64)), ar.place(np.array(sel, np.uint8)),
                               crc, ar.place(raw_off), ar.place(np.array(slot, np.int64)), ar.place(member_off), bgzf=bgzf)
        assert out.data_ptr() % 16 == mis
        assert out.cpu().numpy().tobytes() == b"".join(ref.member(streams[r], raws[r], bgzf) for r in slot)
        assert gzip.decompress(out.cpu().numpy().tobytes()) == b"".join(raws[r] for r in slot)
        # refused: a size that is not header + stream + 8; a record that does not exist — nothing is written
        for what in ("size", "slot"):
            mo, sl = member_off.copy(), np.array(slot, np.int64)
            if what == "size":
                mo[4:] += 1
            else:
                sl[3] = len(raws)
            dst = ar.empty(int(mo[-1]), torch.uint8, misalign=mis)
            before = dst.clone()
            with pytest.raises(ops.HmseError, match="outside its source or the destination"):
                ops.gzip_members(_t(bytes(srcs[0]), dev), _t(bytes(srcs[1]), dev), _t(np.array(src_off, np.int64), dev), _t(np.array([len(s) for s in streams], np.int64), dev),
                                 _t(np.array(sel, np.uint8), dev), crc, _t(raw_off, dev), _t(sl, dev), _t(mo, dev), bgzf=bgzf, out=dst)
            assert torch.equal(dst, before)
    assert ops.crc32_combine(crc[torch.tensor(slot, device=dev)].contiguous(), ar.place(np.array([len(raws[r]) for r in slot], np.int64))) == \
        zlib.crc32(b"".join(raws[r] for r in slot))
    ar.check()


def test_a_bgzf_member_above_64_kib_is_refused(dev):
    import torch
    from hmse_amd import ops
    i64 = lambda *v: _t(np.array(v, np.int64), dev)
    src = torch.zeros(70000, dtype=torch.uint8, device=dev)
    args = lambda n, H=18: (src, None, i64(0), i64(n), _t(np.zeros(1, np.uint8), dev), _t(np.zeros(1, np.int32), dev), i64(0, 5), i64(0), i64(0, H + n + 8))
    assert ops.gzip_members(*args(65536 - 26), bgzf=True).numel() == 65536
    with pytest.raises(ops.HmseError, match="above 65536"):
        ops.gzip_members(*args(65536 - 25), bgzf=True)
    assert ops.gzip_members(*args(65536 - 25 + 8, 10), bgzf=False).numel() == 65537         # plain gzip has no such bound


# ---- stores -------------------------------------------------------------------------------------------------------------------------------
def _store_input():
    """the recipe of tests/test_gpu_approx.py::_store_input: 1.6 MB with a repeated stretch, a near-duplicate family and a run of one byte"""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import variants_dataset
    from hmse_amd import corpus
    w = corpus.wiki_synth(1 << 20, seed=42)
    return np.concatenate([w[: 640 * KIB], w[100_000: 450_000],                       # a repeated 350 000-byte stretch: POINTER chunks
                           variants_dataset(w)[:300_000],                            # a near-duplicate family: DELTA records
                           np.full(100_000, ord("e"), np.uint8)])                    # many POINTERs to one record


def _ragged_seg_off(n, dev):
    import torch
    off = [0]
    for s in [SEG, 1, 2, 3, 70, SEG, 1, 70, 3, 2]:
        off.append(off[-1] + s)
    while off[-1] < n:
        off.append(min(off[-1] + SEG, n))
    return torch.tensor(off, dtype=torch.int64, device=dev)


@pytest.fixture(scope="module")
def stores(dev):
    import torch
    from hmse_amd import IngestConfig, ingest, manifest
    cfg = IngestConfig(seg_size=SEG)
    data = _store_input()
    d = torch.from_numpy(data).to(dev)
    out = {}
    for name, seg_off in (("plain", None), ("ragged", _ragged_seg_off(data.size, dev))):
        res = ingest.ingest_shard(d, cfg, seg_off)
        out[name] = manifest.Manifest.from_bytes(manifest.build_manifest(res).to_bytes())
    return cfg, data, out


@pytest.mark.parametrize("bgzf", [False, True], ids=["gzip", "bgzf"])
@pytest.mark.parametrize("name", ["plain", "ragged"])
def test_export_of_a_store(stores, orc, dev, name, bgzf):
    import torch
    from hmse_amd import KIND_DELTA, KIND_FULL, KIND_POINTER, export, ops, read
    cfg, data, out = stores
    m = out[name]
    corpus = data.tobytes()
    kinds, lens = m.chunk_map["kind"], m.chunk_map["raw_length"]
    assert (kinds == KIND_POINTER).sum() > 0 and (kinds == KIND_DELTA).sum() > 0 and (kinds == KIND_FULL).sum() > 0
    if name == "ragged":
        assert {1, 2, 3, 70} <= set(lens.tolist())
    rd = read.StoreReader(m, dev)
    n_chunks, n_rec = len(rd.slot), len(rd.kind)
    x = export.to_gzip(m, dev, cfg, bgzf=bgzf)
    blob = x.tobytes()
    H = 18 if bgzf else 10
    assert x.data.is_cuda and x.data.dtype == torch.uint8 and x.member_off.dtype == torch.int64
    assert gzip.decompress(blob) == corpus
    assert x.cuts.tolist() == rd.cuts.tolist() and x.crc32 == zlib.crc32(corpus)
    assert export.crc32(m, dev) == x.crc32
    members = ref.parse_members(blob)
    if bgzf:
        assert blob.endswith(ref.BGZF_EOF) and members[-1] == (len(blob) - 28, 28)
        members = members[:-1]
    assert len(members) == n_chunks == x.member_off.numel() - 1
    mo, cuts = x.member_off.tolist(), rd.cuts.tolist()
    assert [o for o, _ in members] == mo[:-1] and mo[-1] == len(blob) - (28 if bgzf else 0)
    assert [export.read_member(x, k) for k in (0, n_chunks - 1)] == [members[0], members[-1]]
    # the DELTA records: encoded again without their dictionaries, as ops.l1_deflate and the CPU oracle encode them
    raw, raw_off = rd.decode()
    delta_ids = np.nonzero(rd.kind == KIND_DELTA)[0]
    s1, off1, kind1 = ops.l1_deflate(raw, raw_off, cfg, chunk_ids=_t(delta_ids.astype(np.int64), dev), base=None)
    s1, off1 = s1.cpu().numpy(), off1.cpu().numpy()
    w_out, w_off, w_kind = orc.deflate_chunks(raw.cpu().numpy(), raw_off.cpu().numpy().astype(np.uint64), orc.default_cfg(**asdict(cfg)), delta_ids.astype(np.uint64))
    assert np.array_equal(s1, w_out) and np.array_equal(off1.astype(np.uint64), w_off) and not w_kind.any() and not kind1.any()
    again = {int(r): s1[off1[i]: off1[i + 1]].tobytes() for i, r in enumerate(delta_ids)}
    assert x.n_reencoded == len(delta_ids) > 0 and x.n_copied + x.n_reencoded == n_rec
    copies = 0
    for k, (o, size) in enumerate(members):
        mem, part = blob[o: o + size], corpus[cuts[k]: cuts[k + 1]]
        assert zlib.decompress(mem, wbits=31) == part, k
        assert mem[-8:] == zlib.crc32(part).to_bytes(4, "little") + len(part).to_bytes(4, "little"), k
        r = int(rd.slot[k])
        stream = mem[H:-8]
        if bgzf:                                                                       # every block parses by the layout
            assert mem[:16] == ref.BGZF_HEADER and int.from_bytes(mem[16:18], "little") + 1 == size <= 65536, k
        else:
            assert mem[:10] == ref.GZIP_HEADER, k
        if rd.kind[r] == KIND_FULL:                                                    # a copy of the blob's record
            a = int(rd.stream_off[r])
            assert stream == m.blob[a: a + int(rd.stream_len[r])].tobytes(), k
            copies += 1
        else:
            assert rd.kind[r] == KIND_DELTA and stream == again[r], k
    assert copies > n_chunks // 2 and copies > x.n_copied                              # POINTER chunks are members too: copies of copies


def test_two_shard_store_and_an_unmerged_one(dev):
    """built as tests/test_gpu_read_ranges.py builds one: the second shard repeats bytes of the first"""
    import torch
    from hmse_amd import IngestConfig, corpus, export, ingest, manifest, read
    cfg = IngestConfig(seg_size=SEG)
    data = corpus.wiki_synth(1 << 20, seed=42).copy()
    data[640 * KIB + 5000: 900 * KIB + 5000] = data[5000: 260 * KIB + 5000]        # the second shard repeats bytes of the first
    shards = [torch.from_numpy(data[: 512 * KIB]).to(dev), torch.from_numpy(data[512 * KIB:]).to(dev)]
    res = ingest.ingest_shards_local(shards, cfg)
    parts = [manifest.build_manifest(r, i, 2) for i, r in enumerate(res)]
    assert ((parts[1].pointers["flags"] & manifest.PTR_UNRESOLVED) != 0).sum() > 10     # cross-shard pointers
    with pytest.raises(read.ReadError):
        export.to_gzip(manifest.Store(parts), dev)
    with pytest.raises(read.ReadError):
        export.crc32(manifest.Store(parts), dev)
    store = manifest.Store.from_bytes(manifest.merge_manifests(parts).to_bytes())
    want = read.read_store(store, dev).cpu().numpy().tobytes()
    assert want == data.tobytes()
    for bgzf in (False, True):
        x = export.to_gzip(store, dev, bgzf=bgzf)
        assert gzip.decompress(x.tobytes()) == want and x.crc32 == zlib.crc32(want)
        assert x.member_off.numel() - 1 == sum(len(m.chunk_map) for m in store.shards)
    assert export.crc32(store, dev) == zlib.crc32(want)


def test_max_bytes_and_an_empty_store(stores, dev, monkeypatch, tmp_path):
    from hmse_amd import export, manifest, ops
    cfg, data, out = stores
    m = out["plain"]
    x = export.to_gzip(m, dev, cfg)
    total = x.data.numel()
    assert x.write(tmp_path / "corpus.gz") == total and gzip.open(tmp_path / "corpus.gz").read() == data.tobytes()
    assert export.to_gzip(m, dev, cfg, max_bytes=total).data.numel() == total
    written = []
    real = ops.gzip_members
    monkeypatch.setattr(ops, "gzip_members", lambda *a, **k: written.append(1) or real(*a, **k))
    with pytest.raises(ValueError, match=f"needs {total} bytes, max_bytes is {total - 1}"):    # the exact size: after the DELTA records were encoded
        export.to_gzip(m, dev, cfg, max_bytes=total - 1)
    with pytest.raises(ValueError, match="needs at least .* max_bytes is 1000"):              # the copied streams alone: before any work
        export.to_gzip(m, dev, cfg, max_bytes=1000)
    assert not written
    empty = manifest.Store([])
    e = export.to_gzip(empty, dev)
    assert e.data.numel() == 0 and e.crc32 == 0 and e.member_off.tolist() == [0] and e.cuts.tolist() == [0] and e.n_copied == e.n_reencoded == 0
    z = export.to_gzip(empty, dev, bgzf=True)
    assert z.tobytes() == ref.BGZF_EOF and z.crc32 == 0 and gzip.decompress(z.tobytes()) == b""
    assert export.crc32(empty, dev) == 0 and not written
