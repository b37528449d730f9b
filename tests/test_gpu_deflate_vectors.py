"""GPU: the three DEFLATE walkers — ifl::l1_inflate_kernel (one stream per wavefront), ifl::l1_inflate_lanes_kernel (one per lane) and
gz::measure_kernel — on streams zlib's encoder never writes (tests/deflate_vectors.py: code-length runs across the alphabet boundary,
one-code and empty distance sets, 15-bit codes, the longest possible header at every bit offset, dictionary edges, and what zlib refuses
beside them), on every single-bit flip and truncation of six headers, and on members of hundreds of KiB.  The reference is stock zlib:
accepted if and only if zlib.decompressobj(-15[, zdict]) reaches eof with nothing unused, same bytes (tests/gunzip_ref.py for members)."""
import zlib

import numpy as np
import pytest

import deflate_vectors as dv
import gunzip_ref as ref
from test_gpu_gunzip import _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def inflate(dev, recs):
    """one hmse_l1_inflate call -> (ok flags, [raw bytes of every record])"""
    from hmse_amd import ops
    streams, off, kind, base, raw_len = dv.pack(recs)
    raw, raw_off, ok = ops.l1_inflate(to_dev(streams, dev), to_dev(off, dev), to_dev(kind, dev), to_dev(base, dev), to_dev(raw_len, dev), check=False)
    raw, cuts = raw.cpu().numpy().tobytes(), raw_off.tolist()
    assert cuts == np.concatenate([[0], np.cumsum(raw_len)]).tolist()
    return ok.cpu().numpy().astype(bool), [raw[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def as_zlib(dev, vectors, raws, claimed=()):
    """(with `claimed`: every stream zlib refuses once more per claimed raw length, deflate_vectors.records — refused at each)"""
    recs, first = dv.records(vectors, raws, claimed)
    ok, got = inflate(dev, recs)
    want = np.array([True] * first + [r is not None for r in raws] + [False] * (len(recs) - first - len(raws)))
    refused = [v[0] for v, r in zip(vectors, raws) if r is None]
    name = lambda i: vectors[i - first][0] if i < first + len(raws) else (refused[(i - first - len(raws)) % len(refused)], recs[i][1])
    assert np.array_equal(ok, want), [(name(i), bool(ok[i])) for i in np.nonzero(ok != want)[0][:10]]
    assert got[:first] == list(dv.DICTS.values())
    wrong = [v[0] for v, raw, g in zip(vectors, raws, got[first:]) if raw is not None and g != raw]
    assert not wrong, wrong[:10]


class TestBothDecoders:
    @pytest.fixture(autouse=True, params=[1, 2], ids=["wave-per-stream", "lane-per-stream"])
    def decoder(self, request, dev):
        """Every test of this class runs under both decoders of hmse_l1_inflate (include/hmse.h hmse_l1_inflate_mode)."""
        from hmse_amd import ops
        ops.l1_inflate_mode(request.param)
        yield request.param
        ops.l1_inflate_mode(0)

    def test_the_catalogue(self, dev):
        """The whole catalogue in one call.  The lane kernel stages 288 stream bytes in LDS for a dynamic header where that many lie in front
        of the end of `streams`, and goes back to global memory in the middle of a header that is longer: the longest-header vectors in the
        middle of the call take that path at every bit offset.  The last record's header begins within the last 288 bytes: read unstaged."""
        cat, raws = dv.catalogue(), dv.catalogue_raws()
        order = [i for i, e in enumerate(cat) if "header-short" not in e[0]] + [i for i, e in enumerate(cat) if "header-short" in e[0]]
        vectors, answers = [cat[i] for i in order], [raws[i] for i in order]
        recs, first = dv.records(vectors, answers)
        total, starts = sum(len(r[0]) for r in recs), np.cumsum([0] + [len(r[0]) for r in recs])
        longs = [first + i for i, v in enumerate(vectors) if v[0].startswith(("longest-header@", "longest-header-all-7-bit@"))]
        assert len(longs) == 16 and all(starts[i + 1] + 288 <= total for i in longs)                # staged: 288 bytes and more behind the stream
        b0 = starts[-2] + ((dv.long_header(7, short=True)[2] + 17) >> 3)                           # the byte behind HLIT, HDIST and HCLEN
        assert "header-short@7" in vectors[-1][0] and b0 + 288 > total                             # unstaged
        as_zlib(dev, vectors, answers, dv.CLAIMED)

    @pytest.mark.parametrize("k", range(8))
    def test_the_longest_header_read_unstaged_at_each_bit_offset(self, dev, k):
        cat, raws = dv.catalogue(), dv.catalogue_raws()
        i = next(i for i, e in enumerate(cat) if e[0].startswith(f"longest-header-short@{k}"))
        as_zlib(dev, [cat[0], cat[i]], [raws[0], raws[i]])

    def test_the_flip_family(self, dev):
        as_zlib(dev, dv.flip_family(), dv.family_raws(), (1, 2, 3, 4, 8))

    def test_large_members(self, dev, large):
        """members of 100 to 300 KiB in one call: 65 535-byte stored blocks, windows that slide many times, distance 32 768 throughout"""
        ok, got = inflate(dev, [(s, len(t), -1) for t, s in large])
        assert ok.all() and got == [t for t, _ in large]


@pytest.fixture(scope="module")
def large():
    """[(raw, zlib's stream)]: text and random bytes, levels 0 / 1 / 6 / 9, memLevel 1 and 9, Z_FILTERED and Z_RLE beside the default, one
    stream with a Z_SYNC_FLUSH every 1000 bytes, one 200 KiB input made of a 40 000-byte block (matches keep a distance near 32 768)"""
    text = ref.text(77, 400_000)
    rnd = np.random.default_rng(78).integers(0, 256, 400_000, dtype=np.uint8).tobytes()
    out, k = [], 0

    def one(t, level, mem, strategy):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
        out.append((t, c.compress(t) + c.flush()))

    for level in (0, 1, 6, 9):
        for mem in (1, 9):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_RLE):
                n = 100_000 + (k * 37_501) % 200_001; k += 1
                one(text[(k * 9973) % 90_000:][:n], level, mem, strategy)
            n = 100_000 + (k * 37_501) % 200_001; k += 1
            one(rnd[(k * 9973) % 90_000:][:n], level, mem, zlib.Z_DEFAULT_STRATEGY)
    one(text[:150_000], 9, 9, zlib.Z_HUFFMAN_ONLY)
    one(text[:150_000], 9, 9, zlib.Z_FIXED)
    c, parts, t = zlib.compressobj(6, zlib.DEFLATED, -15), [], text[5000: 125_000]
    for a in range(0, len(t), 1000):
        parts.append(c.compress(t[a: a + 1000]) + c.flush(zlib.Z_SYNC_FLUSH))
    out.append((t, b"".join(parts) + c.flush()))
    block = rnd[:20_000] + text[:20_000]
    one((block * 6)[:200 * 1024], 9, 9, zlib.Z_DEFAULT_STRATEGY)
    assert 36 <= len(out) <= 44 and all(100_000 <= len(t) <= 300 * 1024 and dv.verdict(s) == t for t, s in out)
    return out


@pytest.fixture(scope="module")
def members():
    """-> (the catalogue and the flip family wrapped as gzip members, the accepted dictionary-free catalogue entries as (name, member, raw))"""
    cat, raws = dv.catalogue(), dv.catalogue_raws()
    every = dv.wrapped([(e[1], r) for e, r in zip(cat, raws)] + [(e[1], r) for e, r in zip(dv.flip_family(), dv.family_raws())])
    good = [(e[0], m, r) for e, r, m in zip(cat, raws, every) if r is not None and e[2] is None]
    return every, good


def test_measure_walks_them_as_zlib_does(dev, members):
    from hmse_amd import ops
    blob = b"".join(members[0])
    offs = np.concatenate([[0], np.cumsum([len(m) for m in members[0]])[:-1]]).astype(np.int64)
    so, end, rl, crc, fl = (v.tolist() for v in ops.gzip_measure(to_dev(np.frombuffer(blob, np.uint8).copy(), dev), to_dev(offs, dev)))
    valid = 0
    for k, p in enumerate(offs.tolist()):
        m = ref.measure(blob, p)
        assert (fl[k] & 3) == (m["flags"] & 3) and (end[k], rl[k], crc[k] & 0xFFFFFFFF) == (m["end"], m["raw_len"], m["crc"]), (k, p)
        if m["valid"]:
            assert so[k] == m["stream_off"]
            valid += 1
        else:
            assert fl[k] >> 2 in (1, 2, 3, 4) and (m["why"] not in (ref.WHY_HEADER, ref.WHY_LENGTH) or fl[k] >> 2 == m["why"]), (k, p, fl[k])
    assert 500 < valid < len(offs) - 2000


def test_import_of_the_accepted_members_and_a_refused_one_spliced_in(dev, members):
    from hmse_amd import gunzip
    good = members[1]
    blob, raws = b"".join(m for _, m, _ in good), [r for _, _, r in good]
    _same(gunzip.from_gzip(blob, dev), blob, raws)
    cat = {e[0]: e[1] for e in dv.catalogue()}
    for k, name in ((0, "fixed-distance-symbol-30"), (7, "unused-code-of-one-distance-code"), (31, "run-past-the-end-by-1"), (len(good), "no-end-of-block-code")):
        offset = sum(len(m) for _, m, _ in good[:k])
        spliced = blob[:offset] + ref.member(b"", stream=cat[name]) + blob[offset:]
        with pytest.raises(ref.Refused) as z:
            ref.chain(spliced)
        assert (z.value.member, z.value.offset) == (k, offset)
        with pytest.raises(gunzip.GunzipError) as e:
            gunzip.from_gzip(spliced, dev)
        assert (e.value.member, e.value.offset) == (k, offset), (name, str(e.value))


def test_automatic_dispatch_hands_the_lane_decoder_dynamic_headers(dev, members):
    """49 152 members and more, so that hmse_l1_inflate goes wide by itself: a cycle through the accepted dictionary-free catalogue members.
    Left out of the cycle to keep the file at a few MiB: the 65 535-byte stored block, the 300-block stream and the entry that opens with a
    32 768-byte stored block (its distances are in the catalogue runs of both decoders above)."""
    from hmse_amd import gunzip, ops
    cycle = [(m, r) for name, m, r in members[1] if name not in dv.SLOW and len(m) < 4096]
    assert len(cycle) >= len(members[1]) - 3 and sum("longest-header" in n for n, m, _ in members[1] if len(m) < 4096) == 24
    n_mem = 49_152 + 300
    ops.l1_inflate_mode(0)
    blob = b"".join(cycle[k % len(cycle)][0] for k in range(n_mem))
    imp = gunzip.from_gzip(blob, dev)
    _same(imp, blob, [cycle[k % len(cycle)][1] for k in range(n_mem)])
    assert imp.n_members == n_mem >= 49_152 and len(blob) < 8 << 20
