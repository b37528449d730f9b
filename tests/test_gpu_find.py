"""GPU: exact byte-pattern search (hmse_amd.find; hmse_find_scan / hmse_find_seams / hmse_find_place) against the plain-Python
reference of tests/find_ref.py — per kernel on synthetic tables, on poisoned / misaligned / guarded memory (tests/arena.py), and on
stores: POINTER and DELTA records, tiny chunks of ragged segments, a two-shard merged store, the densest chunking.  All results are
compared bit for bit."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import arena as A
import find_ref as ref

pytestmark = pytest.mark.gpu

MIB = 1 << 20
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc", "find.hip")).read()
S = int(re.search(r"constexpr int FIND_STRIP = (\d+);", _SRC).group(1))                  # the scan's strip: bytes per lane
T = S * int(re.search(r"constexpr int FIND_NT = (\d+);", _SRC).group(1))                # its tile: bytes per workgroup and trip
LENGTHS = (1, 2, 3, 4, 5, 16, 17, 255, 256)


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


def _pairs(hits):
    return sorted((int(h) >> 8, int(h) & 255) for h in hits.tolist())


def scan(dev, raw, raw_off, pats, ic=False, mult=None, hits_cap=None):
    """ops.find_scan on host inputs -> (sorted (position, pattern) pairs, n_hits, counts)."""
    import torch
    from hmse_amd import find, ops
    flat, off = find.pack_patterns(pats)
    h, n, c = ops.find_scan(_t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), None if mult is None else _t(np.asarray(mult, np.int32), dev),
                            _t(flat, dev), off, ic, hits_cap)
    assert h.dtype == torch.int64 and c.dtype == torch.int64
    return _pairs(h), n, c.tolist()


def check_scan(dev, raw, raw_off, pats, ic=False, mult=None):
    want_hits, want_counts = ref.scan_hits(raw, raw_off, pats, ic, mult)
    got, n, counts = scan(dev, raw, raw_off, pats, ic, mult)
    assert got == want_hits and n == len(want_hits) and counts == want_counts
    _, n0, counts0 = scan(dev, raw, raw_off, pats, ic, mult, hits_cap=0)              # count-only mode: the same counts, no list
    assert n0 == n and counts0 == counts
    return got


def tables(corpus, cuts):
    """A chunk map over `corpus`: exact dedupe of the chunks in order of first appearance -> (raw, raw_off, slot)."""
    chunks = [bytes(corpus[cuts[k]: cuts[k + 1]]) for k in range(len(cuts) - 1)]
    recs, slot = [], []
    for c in chunks:
        if c not in recs:
            recs.append(c)
        slot.append(recs.index(c))
    return b"".join(recs), [0] + [int(v) for v in np.cumsum([len(r) for r in recs])], slot


def pipeline(dev, corpus, cuts, pats, ic=False):
    """scan -> sort -> place and the seams over a synthetic chunk map, each against the partition rule of the reference."""
    import torch
    from hmse_amd import find, ops
    raw, raw_off, slot = tables(corpus, cuts)
    flat, off = find.pack_patterns(pats)
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    raw_d, ro, cu, sl, pat = _t(raw if raw else np.zeros(0, np.uint8), dev), d(raw_off), d(cuts), d(slot), _t(flat, dev)
    want_in, want_seam = ref.split(corpus, pats, cuts, ic)
    mult = torch.bincount(sl, minlength=len(raw_off) - 1).to(torch.int32)
    hits, n, counts = ops.find_scan(raw_d, ro, mult, pat, off, ic)
    hits = torch.sort(hits)[0]
    lo = torch.searchsorted(hits, ro << 8)
    chunk_out = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((lo[1:] - lo[:-1])[sl], 0)])
    placed = ops.find_place(hits, ro, cu, sl, chunk_out, int(chunk_out[-1]))
    assert [(int(h) >> 8, int(h) & 255) for h in placed.tolist()] == want_in          # as laid out: ascending by offset, then pattern
    assert counts.tolist() == [sum(1 for _, j in want_in if j == q) for q in range(len(pats))]
    sh, sn, sc = ops.find_seams(raw_d, ro, cu, sl, pat, off, ic)
    assert _pairs(sh) == want_seam and sn == len(want_seam)
    assert sc.tolist() == [sum(1 for _, j in want_seam if j == q) for q in range(len(pats))]
    assert ops.find_seams(raw_d, ro, cu, sl, pat, off, ic, hits_cap=0)[1] == sn
    return want_in, want_seam


# ---- 1. per kernel, synthetic tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", LENGTHS)
def test_scan_around_tile_and_strip_boundaries(dev, m):
    """One record of 3T bytes with matches starting at EVERY offset of [T - m, T + 1] and [S - m, S + 1] (a run of one byte), then a
    pattern of distinct bytes planted at each of those distances from a strip's and a tile's first byte."""
    rec = np.full(3 * T, ord("."), np.uint8)
    rec[T - m: T + 1 + m] = ord("q")
    rec[S - m if S >= m else 0: S + 1 + m] = ord("q")
    got = check_scan(dev, rec.tobytes(), [0, 3 * T], [b"q" * m])
    starts = {p for p, _ in got}
    assert set(range(T - m, T + 2)) <= starts and set(range(max(S - m, 0), S + 2)) <= starts
    rng = np.random.default_rng(m)
    pat = bytes(rng.permutation(np.arange(65, 91, dtype=np.uint8))[:min(m, 26)]) * (m // 26 + 1)
    pat = pat[:m - 1] + b"!" if m > 1 else b"!"                                        # (ends differently: no self-overlap to lean on)
    rels = list(range(-m, 2)) if m <= 17 else [-m, -m + 1, -S - 1, -S, -S + 1, -1, 0, 1]
    n_tiles = len(rels) + 2
    rec = np.full(n_tiles * T, ord("."), np.uint8)
    want = []
    for i, r in enumerate(rels):
        for o in ((i + 1) * T + r, (i + 1) * T + 8 * S * 4 + r):                      # a tile's first byte; a strip's inside the tile
            rec[o: o + m] = np.frombuffer(pat, np.uint8)
            want.append(o)
    got = check_scan(dev, rec.tobytes(), [0, rec.size], [pat, pat[:1]])
    assert sorted(p for p, j in got if j == 0) == sorted(want)


def test_scan_clips_matches_to_their_record(dev):
    for m in (1, 2, 5, 17, 256):
        pat = (b"ab" * 200)[:m - 1] + b"Z"
        recs = [b"", pat[:1], pat[:m - 1], pat, pat + b"x", b"y" + pat, b"", pat + pat, pat[:m - 1], pat[m - 1:], b"filler" * 100 + pat]
        raw = b"".join(recs)
        raw_off = [0] + [int(v) for v in np.cumsum([len(r) for r in recs])]
        got = check_scan(dev, raw, raw_off, [pat])
        # a match at a record's first byte (record 3) and at its last m bytes (the last record); none across a boundary (records 8 | 9)
        assert (raw_off[3], 0) in got and (raw_off[-1] - m, 0) in got
        assert not [p for p, _ in got if raw_off[8] <= p < raw_off[10]] or m == 1
    assert check_scan(dev, b"abcd", [0, 2, 4], [b"abcd", b"ab", b"cd", b"bc"]) == [(0, 1), (2, 2)]       # "ab" | "cd": abcd is no hit
    assert check_scan(dev, b"abcd", [0, 4], [b"abcd"]) == [(0, 0)]
    # records that do not start at raw's first byte nor end at its last: the bytes outside belong to no record
    assert check_scan(dev, b"abcdabcdabcd", [2, 7, 10], [b"ab", b"cd", b"d"]) == [(2, 1), (3, 2), (4, 0), (7, 2), (8, 0)]


def test_scan_counts_runs_multiplicities_and_count_only(dev):
    raw = b"a" * 100000
    pats = [b"a", b"aa", b"a" * 256]
    got, n, counts = scan(dev, raw, [0, 100000], pats)
    assert counts == [100000, 99999, 99745] and n == sum(counts) and len(got) == n
    assert got == ref.scan_hits(raw, [0, 100000], pats)[0]
    assert scan(dev, raw, [0, 100000], pats, hits_cap=0)[1:] == (n, counts)
    raw_off = [0, 10, 10, 5000, 100000]
    check_scan(dev, raw, raw_off, pats)
    check_scan(dev, raw, raw_off, pats, mult=[3, 7, 0, 1000])
    assert scan(dev, raw, raw_off, pats, mult=[3, 7, 0, 1000], hits_cap=0)[2] == [30 + 95000 * 1000, 27 + 94999 * 1000, 94745 * 1000]


def _raw_scan(dev, raw, raw_off, pats, cap, sentinel=-7, flags=0):
    """hmse_find_scan called directly: -> (rc, hits tensor of cap + 64 entries prefilled with the sentinel, n_hits, counts, status)."""
    import torch
    from hmse_amd import _lib, find
    flat, off = find.pack_patterns(pats)
    raw_d, ro, pat = _t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), _t(flat, dev)
    hits = torch.full((cap + 64,), sentinel, dtype=torch.int64, device=dev)
    nh = torch.full((1,), sentinel, dtype=torch.int64, device=dev)
    counts = torch.full((len(pats),), sentinel, dtype=torch.int64, device=dev)
    status = torch.full((1,), sentinel, dtype=torch.int32, device=dev)
    rc = _lib.hip_lib().hmse_find_scan(raw_d.data_ptr(), raw_d.numel(), ro.data_ptr(), len(raw_off) - 1, None, pat.data_ptr(),
                                       (C.c_uint32 * len(off))(*off), len(pats), flags, hits.data_ptr(), cap, nh.data_ptr(), counts.data_ptr(),
                                       status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, hits, int(nh.item()), counts.tolist(), int(status.item())


def test_scan_hit_list_that_runs_out(dev):
    rng = np.random.default_rng(3)
    raw = bytes(rng.integers(97, 101, 3 * T + 77, dtype=np.uint8))
    raw_off, pats = [0, T + 5, 3 * T + 77], [b"ab", b"c"]
    want, want_counts = ref.scan_hits(raw, raw_off, pats)
    assert len(want) > 3000
    rc, hits, n, counts, status = _raw_scan(dev, raw, raw_off, pats, 16)
    assert rc == 0 and status == 1 and n == len(want) and counts == want_counts       # bit 0; n_hits and counts exact all the same
    assert (hits[16:] == -7).all()                                                   # nothing behind hits[16]
    first = [(int(h) >> 8, int(h) & 255) for h in hits[:16].tolist()]
    assert len(set(first)) == 16 and set(first) <= set(want)
    got, n2, counts2 = scan(dev, raw, raw_off, pats, hits_cap=16)                     # the wrapper's second call, with hits_cap = n_hits
    assert got == want and n2 == n and counts2 == want_counts
    rc, hits, n, counts, status = _raw_scan(dev, raw, raw_off, pats, len(want))       # an exact list does not run out
    assert status == 0 and sorted((int(h) >> 8, int(h) & 255) for h in hits[:n].tolist()) == want and (hits[n:] == -7).all()


def test_scan_many_patterns_and_case(dev):
    rng = np.random.default_rng(5)
    words = [b"th" + bytes(rng.integers(97, 123, int(rng.integers(0, 9)), dtype=np.uint8)) for _ in range(31)] + [b"th"]
    assert len(words) == 32 and all(w[:2] == b"th" for w in words)                   # one bitmap entry: the verify path tells them apart
    body = bytearray(rng.integers(97, 123, 2 * T + 1000, dtype=np.uint8).tobytes())
    for i in range(400):
        w = words[i % 32]
        o = int(rng.integers(0, len(body) - 16))
        body[o: o + len(w)] = w
    raw_off = [0, T - 3, T - 3, 2 * T + 1000]
    check_scan(dev, bytes(body), raw_off, words)
    check_scan(dev, bytes(body), raw_off, words[:5] + [b"x", b"q"])                   # one-byte patterns in the bitmap path
    # patterns that differ only in case
    text = b"The THE the tHe ThE. " * 3000 + b"Th"
    pats = [b"the", b"The", b"THE", b"tHe", b"e", b"E"]
    for group in (pats, pats[:3]):                                                   # the bitmap path and the head-compare path
        got = check_scan(dev, text, [0, len(text)], group)
        folded = check_scan(dev, text, [0, len(text)], group, ic=True)
        assert len({j for _, j in got}) == len(group) and len(folded) > len(got)
    # 0xC1 / 0xE1 are not folded, A-Z next to their neighbours @ [ ` { are
    odd = bytes([0xC1, 0xE1, 0x41, 0x61, 0x40, 0x60, 0x5B, 0x7B, 0x5A, 0x7A]) * 500
    for group in ([b"\xc1", b"\xe1", b"a", b"A", b"@", b"`", b"[", b"{", b"Z", b"z"], [b"\xc1\xe1A", b"\xe1"], [b"\xc1\xe1a@`", b"[{Zz\xc1"]):
        for ic in (False, True):
            check_scan(dev, odd, [0, len(odd)], group, ic=ic)
    c = scan(dev, odd, [0, len(odd)], [b"\xc1", b"\xe1", b"a"], ic=True)[2]
    assert c == [500, 500, 1000]


SEAM_CASES = {
    "tiny chunks between normal ones": (b"abcdefghijklmnopqrstuvwxyz" * 40, [0, 300, 301, 303, 306, 306, 700, 701, 701, 701, 702, 1040]),
    "one chunk": (b"abcabcabc", [0, 9]),
    "empty chunks only around one": (b"abcabcabc", [0, 0, 9, 9]),
    "every byte its own chunk": (b"abcabcabcabc", list(range(13))),
}


@pytest.mark.parametrize("name", sorted(SEAM_CASES))
def test_seams_and_place_on_synthetic_chunk_maps(dev, name):
    corpus, cuts = SEAM_CASES[name]
    pats = [corpus[o: o + m] for o, m in ((0, 1), (1, 2), (2, 3), (5, 4), (3, 9))] + [b"zab", b"c", corpus[-3:], corpus[-2:] + b"\x00"]
    pats += [corpus[c - 3: c + 5] for c in cuts if 3 <= c <= len(corpus) - 5][:8]
    for ic in (False, True):
        want_in, want_seam = pipeline(dev, corpus, cuts, [p.upper() if ic else p for p in pats], ic)
    if name.startswith(("tiny", "every")):
        assert want_seam
    # a match ending exactly at N is found, one that would need a byte past N is not (pattern 7 / pattern 8)
    assert (len(corpus) - 3, 7) in want_in + want_seam and not [1 for _, j in want_in + want_seam if j == 8]


def test_seams_long_patterns_and_duplicate_chunks(dev):
    rng = np.random.default_rng(11)
    block = bytes(rng.integers(97, 123, 300, dtype=np.uint8))
    corpus = block + b"X" * 5 + block + block + b"YZ" + block[:100]
    # a 256-byte pattern running over five chunks (100 | 60 | 0 | 1 | 80 | ...), duplicate chunks (one record, three places), the last chunk
    cuts = [0, 100, 160, 160, 161, 241, 300, 305, 405, 465, 465, 466, 546, 605, 705, 765, 766, 846, 905, 907, 1007]
    assert cuts[-1] == len(corpus)
    pats = [corpus[50: 306], corpus[40: 295], block[90:110], block[:100], b"X" * 5, block[299:] + b"X", corpus[-100:], corpus[-101:], b"YZ" + block[:3]]
    assert len(pats[0]) == 256 and len(pats[1]) == 255
    want_in, want_seam = pipeline(dev, corpus, cuts, pats)
    assert (50, 0) in want_seam and (0, 3) in want_in and (305, 3) in want_in and (605, 3) in want_in and (907, 6) in want_in and (906, 7) in want_seam
    pipeline(dev, corpus, cuts, [p.swapcase() for p in pats], ic=True)


def test_seams_of_an_empty_chunk_map(dev):
    import torch
    from hmse_amd import ops
    z = lambda n, dt=torch.int64: torch.zeros(n, dtype=dt, device=dev)
    pat = _t(b"ab", dev)
    h, n, c = ops.find_seams(z(0, torch.uint8), z(1), z(1), z(0), pat, [0, 2])
    assert h.numel() == 0 and n == 0 and c.tolist() == [0]
    assert ops.find_place(z(0), z(1), z(1), z(0), z(1), 0).numel() == 0
    h, n, c = ops.find_scan(z(0, torch.uint8), z(1), None, pat, [0, 1, 2])
    assert h.numel() == 0 and n == 0 and c.tolist() == [0, 0]


def test_place_lays_a_record_s_hits_out_at_every_chunk_that_names_it(dev):
    import torch
    from hmse_amd import ops
    # records: 0 "abcab" (1 chunk), 1 "bcb" (2 chunks), 2 "xyz" (no hit), 3 "cc" (1000 chunks), 4 "ab" (named by no chunk)
    recs = [b"abcab", b"bcb", b"xyz", b"cc", b"ab"]
    slot = [0, 1, 2, 1] + [3] * 1000 + [2]
    raw = b"".join(recs)
    raw_off = [0] + [int(v) for v in np.cumsum([len(r) for r in recs])]
    lens = [len(recs[s]) for s in slot]
    cuts = [0] + [int(v) for v in np.cumsum(lens)]
    corpus = b"".join(recs[s] for s in slot)
    pats = [b"b", b"ab", b"c", b"cc"]
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    hits = torch.sort(ops.find_scan(_t(raw, dev), d(raw_off), None, _t(b"".join(pats), dev), [0, 1, 3, 4, 6])[0])[0]
    lo = torch.searchsorted(hits, d(raw_off) << 8)
    per = (lo[1:] - lo[:-1])[d(slot)]
    chunk_out = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(per, 0)])
    out = ops.find_place(hits, d(raw_off), d(cuts), d(slot), chunk_out, int(chunk_out[-1]))
    want = ref.split(corpus, pats, cuts)[0]
    assert [(int(h) >> 8, int(h) & 255) for h in out.tolist()] == want and len(want) == 5 + 3 + 3 + 3 * 1000
    assert per.tolist()[:5] == [5, 3, 0, 3, 3]


def test_inconsistent_tables_set_bit_1_and_leave_the_outputs_alone(dev):
    import torch
    from hmse_amd import _lib, ops
    lib = _lib.hip_lib()
    raw = b"abcdabcdabcdabcd"
    for raw_off in ([0, 8, 4, 16], [0, 8, 17], [9, 8, 16]):                            # descending; records beyond raw_bytes
        rc, hits, n, counts, status = _raw_scan(dev, raw, raw_off, [b"ab", b"d"], 32)
        assert rc == 0 and status == 2 and n == 0 and counts == [0, 0] and (hits == -7).all()
        with pytest.raises(ops.HmseError, match="inconsistent"):
            scan(dev, raw, raw_off, [b"ab"])
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    stream = torch.cuda.current_stream().cuda_stream
    pat, off = _t(b"abcd", dev), (C.c_uint32 * 3)(0, 2, 4)
    raw_d, good_ro, good_cu, good_sl = _t(raw, dev), [0, 8, 16], [0, 8, 16, 24], [0, 1, 0]
    for ro, cu, sl in (([0, 8, 16], [0, 8, 16, 24], [0, 2, 0]), (good_ro, [0, 8, 7, 15], good_sl), ([0, 9, 16], good_cu, good_sl),
                       (good_ro, [0, 8, 16, 25], good_sl), ([0, 8, 16], good_cu, [0, 1, -1])):
        hits = torch.full((64,), -7, dtype=torch.int64, device=dev)
        nh, counts, status = torch.full((1,), -7, dtype=torch.int64, device=dev), torch.full((2,), -7, dtype=torch.int64, device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev)
        ro_d, cu_d, sl_d = d(ro), d(cu), d(sl)
        rc = lib.hmse_find_seams(raw_d.data_ptr(), 16, ro_d.data_ptr(), 2, cu_d.data_ptr(), sl_d.data_ptr(), 3, pat.data_ptr(), off, 2, 0,
                                 hits.data_ptr(), 64, nh.data_ptr(), counts.data_ptr(), status.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0 and int(status.item()) == 2 and int(nh.item()) == 0 and counts.tolist() == [0, 0] and (hits == -7).all(), (ro, cu, sl)
        out = torch.full((64,), -7, dtype=torch.int64, device=dev)
        sorted_hits, chunk_out = d([0 << 8, 4 << 8, 8 << 8]), d([0, 2, 3, 5])
        rc = lib.hmse_find_place(sorted_hits.data_ptr(), 3, ro_d.data_ptr(), 2, cu_d.data_ptr(), sl_d.data_ptr(), 3, chunk_out.data_ptr(),
                                 out.data_ptr(), 64, status.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0 and int(status.item()) == 2 and (out == -7).all(), (ro, cu, sl)
    # the same calls with consistent tables go through; a chunk_out that is not the records' hit counts is bit 1, a short output bit 0
    ro_d, cu_d, sl_d = d(good_ro), d(good_cu), d(good_sl)
    sorted_hits = d([0 << 8, 4 << 8, 8 << 8, 12 << 8])
    assert [int(h) >> 8 for h in ops.find_place(sorted_hits, ro_d, cu_d, sl_d, d([0, 2, 4, 6]), 6).tolist()] == [0, 4, 8, 12, 16, 20]
    with pytest.raises(ops.HmseError, match="inconsistent"):
        ops.find_place(sorted_hits, ro_d, cu_d, sl_d, d([0, 2, 5, 7]), 7)
    with pytest.raises(ops.HmseError, match="inconsistent"):
        ops.find_place(sorted_hits, ro_d, cu_d, sl_d, d([0, 2, 1, 3]), 3)
    with pytest.raises(ops.HmseError, match="exceeds"):
        ops.find_place(sorted_hits, ro_d, cu_d, sl_d, d([0, 2, 4, 6]), 4)


# ---- 2. memory ---------------------------------------------------------------------------------------------------------------------------
def _memory_case():
    rng = np.random.default_rng(21)
    block = bytes(rng.integers(97, 101, 700, dtype=np.uint8))
    corpus = block + b"abcd" + block + bytes(rng.integers(97, 101, T + 300, dtype=np.uint8)) + block[:350]
    cuts = [0, 350, 700, 702, 704, 1054, 1404, 1404 + T, 1404 + T + 300, 1404 + T + 650]
    assert cuts[-1] == len(corpus)
    pats = [b"ab", b"abcd", b"ABC", corpus[340:360], corpus[698:708], b"d"]
    return corpus, cuts, pats


MEMORY = [("zero", 0, False), ("ones", 0, False), ("random", 0, False), ("random", 1, False), ("random", 2, False), ("random", 3, False),
          ("random", 13, False), ("random", 0, True)]


@pytest.mark.parametrize("pattern,misalign,distrust", MEMORY)
def test_entry_points_depend_on_their_arguments_only(dev, monkeypatch, pattern, misalign, distrust):
    """Each of the three entry points on poisoned memory (outputs, status words and counts included: distrust = the wrapper's own fills
    are poisoned, too), with raw and pat off their alignment, between guard bands."""
    import torch
    from hmse_amd import find, ops
    corpus, cuts, pats = _memory_case()
    raw, raw_off, slot = tables(corpus, cuts)
    flat, off = find.pack_patterns(pats)
    ar = A.Arena(dev, pattern, seed=17).install(monkeypatch, distrust_zeros=distrust, byte_misalign=misalign)
    i64 = lambda a: ar.place(np.asarray(a, np.int64))
    raw_d, pat = ar.place(np.frombuffer(raw, np.uint8).copy(), misalign=misalign), ar.place(flat.copy(), misalign=misalign)
    ro, cu, sl = i64(raw_off), i64(cuts), i64(slot)
    mult = ar.place(np.bincount(slot, minlength=len(raw_off) - 1).astype(np.int32))
    for ic in (False, True):
        want_in, want_seam = ref.split(corpus, pats, cuts, ic)
        want_scan, want_counts = ref.scan_hits(raw, raw_off, pats, ic, mult.tolist())
        hits, n, counts = ops.find_scan(raw_d, ro, mult, pat, off, ic)
        assert _pairs(hits) == want_scan and n == len(want_scan) and counts.tolist() == want_counts
        assert ops.find_scan(raw_d, ro, mult, pat, off, ic, hits_cap=0)[2].tolist() == want_counts
        assert _pairs(ops.find_scan(raw_d, ro, None, pat, off, ic, hits_cap=5)[0]) == want_scan
        sh, sn, sc = ops.find_seams(raw_d, ro, cu, sl, pat, off, ic)
        assert _pairs(sh) == want_seam and sn == len(want_seam) and int(sc.sum()) == sn
        hs = ar.place(torch.sort(hits)[0])
        lo = torch.searchsorted(hs, ro << 8)
        chunk_out = ar.place(torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((lo[1:] - lo[:-1])[sl], 0)]))
        placed = ops.find_place(hs, ro, cu, sl, chunk_out, len(want_in))
        assert [(int(h) >> 8, int(h) & 255) for h in placed.tolist()] == want_in
    ar.check()


@pytest.mark.parametrize("misalign", [0, 3])
def test_nothing_behind_raw_bytes_is_a_match(dev, monkeypatch, misalign):
    """raw_bytes ends inside the buffer after "...ab", with "cd" lying right behind it: no hit, and no guard band changes."""
    from hmse_amd import ops
    ar = A.Arena(dev, "random", seed=23).install(monkeypatch)
    for n in (T + 2, 3 * S + 2, 2, 13):
        body = np.full(n, ord("."), np.uint8)
        body[-2:] = np.frombuffer(b"ab", np.uint8)
        raw, both = ar.place_with_tail(body, np.frombuffer(b"cd" * 40, np.uint8).copy(), misalign=misalign)
        assert both[n - 2: n + 2].cpu().numpy().tobytes() == b"abcd"
        ro = ar.place(np.array([0, n], np.int64))
        for pats, off, want in ((b"abcdbc", [0, 4, 6], []), (b"abcdcdbcbab", [0, 4, 6, 8, 9, 11], [(n - 2, 4), (n - 1, 3)])):
            pat = ar.place(np.frombuffer(pats, np.uint8).copy(), misalign=misalign)
            hits, nh, counts = ops.find_scan(raw, ro, None, pat, off)
            assert _pairs(hits) == want and nh == len(want) and counts.tolist() == [0] * (len(off) - 1 - len(want)) + [1] * len(want)
    # the seams read raw through the chunk map only: a last chunk that ends at raw_bytes, "cd" behind it
    body = np.frombuffer(b"....ab", np.uint8).copy()
    raw, both = ar.place_with_tail(body, np.frombuffer(b"cd" * 40, np.uint8), misalign=misalign)
    ro, cu, sl = ar.place(np.array([0, 5, 6], np.int64)), ar.place(np.array([0, 5, 6], np.int64)), ar.place(np.array([0, 1], np.int64))
    pat = ar.place(np.frombuffer(b"abcdab", np.uint8).copy(), misalign=misalign)
    sh, sn, sc = ops.find_seams(raw, ro, cu, sl, pat, [0, 4, 6])
    assert _pairs(sh) == [(4, 1)] and sc.tolist() == [0, 1]
    ar.check()


# ---- 3. store level ----------------------------------------------------------------------------------------------------------------------
def _store_input():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import variants_dataset
    from hmse_amd import corpus
    w = corpus.wiki_synth(2 * MIB, seed=42)
    return np.concatenate([w[: MIB + 300_000], w[200_000: 900_000],                   # a repeated 700 000-byte stretch: POINTER chunks
                           variants_dataset(w)[:600_000],                            # a near-duplicate family: DELTA records
                           np.full(200_000, ord("e"), np.uint8)])                    # many POINTERs to one record, every boundary a seam


def _ragged_seg_off(n, dev):
    import torch
    sizes = [MIB, 1, 2, 3, 70, MIB, 1, 70, 3, 2]
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    while off[-1] < n:
        off.append(min(off[-1] + MIB, n))
    return torch.tensor(off, dtype=torch.int64, device=dev)


@pytest.fixture(scope="module")
def stores(dev):
    import torch
    from hmse_amd import IngestConfig, find, ingest, manifest
    cfg = IngestConfig(seg_size=MIB)
    data = _store_input()
    d = torch.from_numpy(data).to(dev)
    out = {}
    for name, seg_off in (("plain", None), ("ragged", _ragged_seg_off(data.size, dev))):
        res = ingest.ingest_shard(d, cfg, seg_off)
        m = manifest.Manifest.from_bytes(manifest.build_manifest(res).to_bytes())
        out[name] = (m, find.StoreFinder(m, dev))
    return cfg, data, out


def _store_patterns(data, cuts):
    rng = np.random.default_rng(9)
    b = data.tobytes()
    pats = [b[o: o + m] for m in LENGTHS for o in (int(rng.integers(0, len(b) - 256)),)]           # 9: every boundary length
    pats += [b[c - 3: c + 5] for c in cuts[1:-1: max(1, (len(cuts) - 2) // 12)][:12]]                 # 12: straddling a cut
    pats += [b[MIB + 300_000 + o: MIB + 300_000 + o + m] for o, m in ((5, 7), (350_000, 33), (699_900, 100), (12_345, 256))]   # in the repeated stretch
    pats += [b"e", b"ee", b"e" * 256, b"e" * 255 + b"x", b" the ", b"The", b"of", b"\n"]             # frequent ones; the run of one byte
    pats += [b[o: o + int(m)] for o, m in zip(rng.integers(0, len(b) - 256, 7), rng.integers(1, 257, 7))]
    assert len(pats) == 40 and {len(p) for p in pats} >= set(LENGTHS)
    return pats


@pytest.mark.parametrize("name", ["plain", "ragged"])
def test_store_finder_equals_the_reference(stores, dev, name):
    from hmse_amd import KIND_DELTA, KIND_POINTER, read
    cfg, data, out = stores
    m, fd = out[name]
    kinds, lens = m.chunk_map["kind"], m.chunk_map["raw_length"]
    assert (kinds == KIND_POINTER).sum() > 50 and (kinds == KIND_DELTA).sum() > 5
    if name == "ragged":
        assert (lens < cfg.min_size).sum() >= 8 and {1, 2, 3, 70} <= set(lens.tolist())
    assert fd.n_bytes == data.size and 0 < fd.n_records < len(kinds) and fd.resident_bytes > int(fd.raw.numel())
    assert int(fd.raw.numel()) < data.size - 700_000                                  # the scan reads unique bytes only
    b = data.tobytes()
    pats = _store_patterns(data, fd.cuts.tolist())
    for ic in (False, True):
        q = [p.swapcase() for p in pats] if ic else pats
        want = ref.find(b, q, ic)
        got = fd.find(q, ignore_case=ic)
        assert got.counts.tolist() == want[0] and got.ptr.tolist() == want[1]
        assert got.offsets.tolist() == want[2]
        assert fd.count(q, ignore_case=ic).tolist() == want[0]
    one = fd.find([pats[0]])
    assert one.counts.tolist() == [len(ref.occurrences(b, pats[0]))]


def test_store_finder_limits_and_edges(stores, dev):
    import torch
    from hmse_amd import find, manifest
    cfg, data, out = stores
    m, fd = out["plain"]
    with pytest.raises(ValueError, match=r"counts per pattern: \[\d+, \d+\]"):
        fd.find([b"e", b"th"], max_hits=10)
    n_e = int(fd.count([b"e"])[0])
    assert fd.find([b"e"], max_hits=n_e).offsets.numel() == n_e
    z = fd.find([])
    assert z.ptr.tolist() == [0] and z.offsets.numel() == 0 and z.counts.numel() == 0 and fd.count([]).numel() == 0
    assert z.ptr.dtype == torch.int64 and z.offsets.dtype == torch.int64 and z.offsets.device.type == "cuda"
    for bad in (["e"], [b""], [b"x" * 257]):
        with pytest.raises(ValueError):
            fd.find(bad)
    empty = find.StoreFinder(manifest.Store([]), dev)
    assert empty.n_bytes == 0 and empty.n_records == 0
    f = empty.find([b"a", b"bc"])
    assert f.counts.tolist() == [0, 0] and f.ptr.tolist() == [0, 0, 0] and f.offsets.numel() == 0 and empty.count([b"a"]).tolist() == [0]
    got = find.find(m, [b" the "], dev, ignore_case=True)                              # the one-off form
    assert got.counts.tolist() == [len(ref.occurrences(data.tobytes(), b" the ", True))]


# ---- 4. a two-shard merged store ---------------------------------------------------------------------------------------------------------
def test_two_shard_store_gives_the_one_shard_results(stores, dev):
    import torch
    from hmse_amd import find, ingest, manifest, read
    cfg, data, out = stores
    half = MIB + 300_000 + 350_000                                                   # inside the repeated stretch: POINTERs across shards
    rs = ingest.ingest_shards_local([torch.from_numpy(p).to(dev) for p in (data[:half], data[half:])], cfg)
    st = manifest.Store.from_bytes(manifest.merge_manifests([manifest.build_manifest(r, i, 2) for i, r in enumerate(rs)]).to_bytes())
    assert any((s.chunk_map["shard"] != i).any() for i, s in enumerate(st.shards))   # a chunk of one shard stored on the other
    fd2, fd1 = find.StoreFinder(st, dev), out["plain"][1]
    pats = _store_patterns(data, fd1.cuts.tolist()) + [data[half - 6: half + 6].tobytes()]
    for ic in (False, True):
        a, b = fd1.find(pats, ignore_case=ic), fd2.find(pats, ignore_case=ic)
        assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("ptr", "offsets", "counts"))
    assert fd2.find(pats[-1:]).offsets.tolist() == ref.occurrences(data.tobytes(), pats[-1])
    with pytest.raises(read.ReadError, match="merge_manifests"):
        find.StoreFinder(manifest.build_manifest(rs[1], 1, 2), dev)


# ---- 5. the densest chunking -------------------------------------------------------------------------------------------------------------
def test_smallest_chunk_sizes(dev):
    import torch
    from hmse_amd import IngestConfig, corpus, find, ingest, manifest
    cfg = IngestConfig(min_size=64, avg_size=256, max_size=1024, seg_size=1 << 16)
    w = corpus.wiki_synth(192 << 10, seed=7)
    data = np.concatenate([w, w[10_000: 10_000 + (64 << 10)]])
    assert data.size == 256 << 10
    res = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    fd = find.StoreFinder(manifest.Manifest.from_bytes(manifest.build_manifest(res).to_bytes()), dev)
    cuts = fd.cuts.tolist()
    assert len(cuts) > 600
    b = data.tobytes()
    rng = np.random.default_rng(13)
    pats = [b[c - 3: c + 5] for c in cuts[5:-1:60]] + [b[o: o + m] for m in LENGTHS for o in (int(rng.integers(0, len(b) - 256)),)] + [b"e", b" "]
    for ic in (False, True):
        want = ref.find(b, pats, ic)
        got = fd.find(pats, ignore_case=ic)
        assert got.counts.tolist() == want[0] and got.ptr.tolist() == want[1] and got.offsets.tolist() == want[2]
        assert fd.count(pats, ignore_case=ic).tolist() == want[0]
