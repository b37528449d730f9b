"""GPU: dictionary search (hmse_amd.find.PatternSet, StoreFinder.count_set / find_set; hmse_findset_scan / _seams / _place) against the
plain-Python reference of tests/find_ref.py — per kernel on synthetic tables, set shapes that stress the directory, hit lists that run
out, inconsistent tables and damaged sets, poisoned / misaligned / guarded memory (tests/arena.py), and stores: POINTER and DELTA
records, tiny chunks of ragged segments, a two-shard merged store, the densest chunking.  All results are compared bit for bit; a set
of at most 32 patterns is also compared with the grouped kernels (ops.find_scan / find_seams / find_place) on the same tables."""
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
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc", "findset.hip")).read()
S = int(re.search(r"constexpr int FSET_STRIP = (\d+);", _SRC).group(1))                  # the scan's strip: bytes per lane
T = S * int(re.search(r"constexpr int FSET_NT = (\d+);", _SRC).group(1))                # its tile: bytes per workgroup and trip
B = 24                                                                                   # a hit: position << 24 | id
HASH = 0x9E3779B1
LENGTHS = (4, 5, 16, 17, 255, 256)


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


def _pairs(hits, bits=B):
    return sorted((int(h) >> bits, int(h) & ((1 << bits) - 1)) for h in hits.tolist())


def _long(ps):
    """The unique patterns the set's kernels answer (4 bytes or more): [(unique id, bytes)]."""
    return [(u, p) for u, p in enumerate(ps.unique) if len(p) >= 4]


def _want_scan(ps, raw, raw_off, mult=None):
    lg = _long(ps)
    hits, counts = ref.scan_hits(raw, raw_off, [p for _, p in lg], ps.ignore_case, mult)
    full = [0] * ps.n_unique
    for (u, _), c in zip(lg, counts):
        full[u] = c
    return sorted((o, lg[j][0]) for o, j in hits), full


def check_scan(dev, raw, raw_off, pats, ic=False, mult=None):
    """ops.findset_scan on host inputs against the reference (and, up to 32 patterns, against ops.find_scan) -> sorted (position, id)."""
    import torch
    from hmse_amd import find, ops
    ps = find.PatternSet(pats, ic, dev)
    raw_d, ro = _t(raw, dev), _t(np.asarray(raw_off, np.int64), dev)
    mu = None if mult is None else _t(np.asarray(mult, np.int32), dev)
    want, want_counts = _want_scan(ps, raw, raw_off, mult)
    h, n, c = ops.findset_scan(raw_d, ro, mu, ps.set)
    assert h.dtype == torch.int64 and c.dtype == torch.int64 and c.numel() == ps.n_unique
    got = _pairs(h)
    assert got == want and n == len(want) and c.tolist() == want_counts
    h0, n0, c0 = ops.findset_scan(raw_d, ro, mu, ps.set, hits_cap=0)                       # count-only: the same counts, no list
    assert h0.numel() == 0 and n0 == n and c0.tolist() == want_counts
    lg = _long(ps)
    if 0 < len(lg) <= 32:
        flat, off = find.pack_patterns([p for _, p in lg])
        oh, on, oc = ops.find_scan(raw_d, ro, mu, _t(flat, dev), off, ic)
        assert sorted((o, lg[j][0]) for o, j in _pairs(oh, 8)) == got and on == n and oc.tolist() == [want_counts[u] for u, _ in lg]
    return got


def tables(corpus, cuts):
    """A chunk map over `corpus`: exact dedupe of the chunks in order of first appearance -> (raw, raw_off, slot)."""
    seen, recs, slot = {}, [], []
    for k in range(len(cuts) - 1):
        c = bytes(corpus[cuts[k]: cuts[k + 1]])
        if c not in seen:
            seen[c] = len(recs)
            recs.append(c)
        slot.append(seen[c])
    return b"".join(recs), [0] + [int(v) for v in np.cumsum([len(r) for r in recs])], slot


def finder(dev, corpus, cuts):
    """A StoreFinder over a synthetic chunk map (no store behind it): the attributes StoreFinder.__init__ leaves."""
    import torch
    from hmse_amd import find
    raw, raw_off, slot = tables(corpus, cuts)
    fd = object.__new__(find.StoreFinder)
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    fd.dev, fd.n_bytes, fd.n_records = dev, len(corpus), len(raw_off) - 1
    fd.raw, fd.raw_off, fd.slot, fd.cuts = _t(raw if raw else np.zeros(0, np.uint8), dev), d(raw_off), d(slot), d(cuts)
    fd.mult = torch.bincount(fd.slot, minlength=fd.n_records).to(torch.int32)
    return fd


def check_find_set(dev, fd, corpus, pats, ic=False, want=None):
    """find_set and count_set against ref.find on the corpus bytes (and against StoreFinder.find up to 32 patterns)."""
    import torch
    from hmse_amd import find
    want = ref.find(corpus, pats, ic) if want is None else want
    ps = find.PatternSet(pats, ic, dev)
    got = fd.find_set(ps)
    assert got.counts.tolist() == want[0] and got.ptr.tolist() == want[1]
    assert got.offsets.tolist() == want[2]
    assert got.offsets.dtype == torch.int64 and got.ptr.dtype == torch.int64 and got.counts.dtype == torch.int64
    assert fd.count_set(ps).tolist() == want[0]
    if len(pats) <= 32:
        old = fd.find(pats, ignore_case=ic)
        assert all(torch.equal(getattr(old, f), getattr(got, f)) for f in ("ptr", "offsets", "counts"))
    return got


def pipeline(dev, corpus, cuts, pats, ic=False):
    """scan -> sort -> place and the seams over a synthetic chunk map, each against the partition rule of the reference."""
    import torch
    from hmse_amd import find, ops
    ps = find.PatternSet(pats, ic, dev)
    lg = _long(ps)
    raw, raw_off, slot = tables(corpus, cuts)
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    raw_d, ro, cu, sl = _t(raw if raw else np.zeros(0, np.uint8), dev), d(raw_off), d(cuts), d(slot)
    win, wseam = ref.split(corpus, [p for _, p in lg], cuts, ic)
    want_in, want_seam = [(o, lg[j][0]) for o, j in win], sorted((o, lg[j][0]) for o, j in wseam)
    mult = torch.bincount(sl, minlength=len(raw_off) - 1).to(torch.int32)
    hits, n, counts = ops.findset_scan(raw_d, ro, mult, ps.set)
    hits = torch.sort(hits)[0]
    lo = torch.searchsorted(hits, ro << B)
    chunk_out = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((lo[1:] - lo[:-1])[sl], 0)])
    placed = ops.findset_place(hits, ro, cu, sl, chunk_out, int(chunk_out[-1]))
    got_in = [(int(h) >> B, int(h) & 0xFFFFFF) for h in placed.tolist()]
    assert got_in == sorted(want_in)                                                   # as laid out: ascending by (offset, id)
    assert counts.tolist() == [sum(1 for _, u in want_in if u == q) for q in range(ps.n_unique)]
    sh, sn, sc = ops.findset_seams(raw_d, ro, cu, sl, ps.set)
    assert _pairs(sh) == want_seam and sn == len(want_seam)
    assert sc.tolist() == [sum(1 for _, u in want_seam if u == q) for q in range(ps.n_unique)]
    assert ops.findset_seams(raw_d, ro, cu, sl, ps.set, hits_cap=0)[1] == sn
    if 0 < len(lg) <= 32:                                                              # the grouped kernels on the same tables
        flat, off = find.pack_patterns([p for _, p in lg])
        oh = ops.find_seams(raw_d, ro, cu, sl, _t(flat, dev), off, ic)[0]
        assert sorted((o, lg[j][0]) for o, j in _pairs(oh, 8)) == want_seam
    return sorted(want_in), want_seam


# ---- 1. the scan on synthetic tables -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", LENGTHS)
def test_scan_around_tile_and_strip_boundaries(dev, m):
    """One record of 3T bytes with matches starting at EVERY offset of [T - m, T + 1] and [S - m, S + 1] (a run of one byte), then a
    pattern of distinct bytes planted at each of those distances from a tile's and a strip's first byte."""
    rec = np.full(3 * T, ord("."), np.uint8)
    rec[T - m: T + 1 + m] = ord("q")
    rec[S - m if S >= m else 0: S + 1 + m] = ord("q")
    got = check_scan(dev, rec.tobytes(), [0, 3 * T], [b"q" * m])
    starts = {p for p, _ in got}
    assert set(range(T - m, T + 2)) <= starts and set(range(max(S - m, 0), S + 2)) <= starts
    rng = np.random.default_rng(m)
    pat = bytes(rng.permutation(np.arange(65, 91, dtype=np.uint8))[:min(m, 26)]) * (m // 26 + 1)
    pat = pat[:m - 1] + b"!"                                                           # (ends differently: no self-overlap to lean on)
    rels = list(range(-m, 2)) if m <= 17 else [-m, -m + 1, -S - 1, -S, -S + 1, -3, -2, -1, 0, 1]
    rec = np.full(3 * T, ord("."), np.uint8)
    want, o0 = [], 2 * S
    for i, r in enumerate(rels):                                                       # around a strip's first byte, 3 strips apart each
        o = o0 + 3 * S * (i + 1) + r
        rec[o: o + m] = np.frombuffer(pat, np.uint8)
        want.append(o)
    for r in (rels[0], -3, -2, -1, 0, 1):                                               # around the tiles' first bytes
        for base in (T, 2 * T):
            o = base + r
            if not any(abs(o - w) < m for w in want):
                rec[o: o + m] = np.frombuffer(pat, np.uint8)
                want.append(o)
    got = check_scan(dev, rec.tobytes(), [0, rec.size], [pat, pat[:4]])
    assert sorted(p for p, j in got if j == 0) == sorted(want) and len(want) >= len(rels) + 2


def test_window_reaching_over_the_record_s_end_and_over_raw_bytes(dev):
    """Records that end 1, 2 and 3 bytes behind a candidate's start (its four-byte window reaches into the next record, or over
    raw_bytes in the last one), junk in front of, between (a record no pattern may match across) and behind the records."""
    pats = [b"abcd", b"abcdef", b"bcda", b"dabc", b"cdab"]
    recs = [b"xxabcdef", b"a", b"bcd", b"ab", b"cd", b"abc", b"dabcd", b"", b"abcdabc"]
    lead, tail = b"abcdefabcd", b"defabcdef"
    raw = lead + b"".join(recs) + tail
    raw_off = [len(lead)] + [len(lead) + int(v) for v in np.cumsum([len(r) for r in recs])]
    got = check_scan(dev, raw, raw_off, pats)
    assert got == sorted([(12, 0), (12, 1), (raw_off[6], 3), (raw_off[6] + 1, 0), (raw_off[8], 0), (raw_off[8] + 1, 2), (raw_off[8] + 2, 4), (raw_off[8] + 3, 3)])
    for cut in (1, 2, 3):                                                              # the last record ends at raw_bytes, `cut` bytes into "abcd"
        body = b"." * (T - 2) + b"abcdabcd"[: 4 + cut]
        check_scan(dev, body, [0, len(body)], pats)
        check_scan(dev, body, [0, 5, len(body)], pats, ic=True)
    # raw_bytes inside the buffer: "cd" lies right behind it
    import torch
    from hmse_amd import find, ops
    ps = find.PatternSet(pats, False, dev)
    for n in (T + 2, 3 * S + 2, 2, 13):
        buf = _t(b"." * (n - 2) + b"abcdcdab", dev)
        h, nh, c = ops.findset_scan(buf, _t(np.array([0, n], np.int64), dev), None, ps.set, raw_bytes=n)
        assert nh == 0 and h.numel() == 0 and int(c.sum()) == 0


def test_scan_counts_runs_multiplicities_and_a_lane_with_more_than_256_hits(dev):
    """A run of one byte against the chain of nested prefixes of lengths 4..256: every position of the run holds up to 253 hits, a
    lane's strip of 128 positions tens of thousands — counted first, stored at the reserved place."""
    import torch
    from hmse_amd import find, ops
    run = 3 * S + 57
    raw = b"." * 100 + b"a" * run + b"." * 100
    pats = [b"a" * m for m in range(4, 257)]
    ps = find.PatternSet(pats, False, dev)
    raw_d, ro = _t(raw, dev), _t(np.array([0, len(raw)], np.int64), dev)
    h, n, c = ops.findset_scan(raw_d, ro, None, ps.set)
    want = [run - m + 1 for m in range(4, 257)]
    assert c.tolist() == want and n == sum(want) and n > 256 * 128
    got = torch.sort(h)[0]
    exp = torch.tensor(sorted(((100 + o) << B) | (m - 4) for m in range(4, 257) for o in range(run - m + 1)), dtype=torch.int64, device=dev)
    assert torch.equal(got, exp)
    raw_off, mult = [0, 50, 50, 100 + run // 2, len(raw)], [3, 7, 2, 1000]
    want_hits, want_counts = _want_scan(ps, raw, raw_off, mult)
    h, n, c = ops.findset_scan(raw_d, _t(np.array(raw_off, np.int64), dev), _t(np.array(mult, np.int32), dev), ps.set)
    assert c.tolist() == want_counts and n == len(want_hits) and _pairs(h) == want_hits


# ---- 2. set shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def words(dev):
    """A 256 KiB corpus of random lower-case words (some capitalised), a chunk map with tiny chunks, its finder."""
    rng = np.random.default_rng(77)
    vocab = [bytes(rng.integers(97, 123, int(rng.integers(2, 10)), dtype=np.uint8)) for _ in range(3000)]
    text = b" ".join(vocab[i] if rng.random() < 0.9 else vocab[i].capitalize() for i in rng.integers(0, 3000, 60000))[: 256 << 10]
    assert len(text) == 256 << 10
    cuts = [0]
    while cuts[-1] < len(text):
        cuts.append(min(len(text), cuts[-1] + int(rng.choice([0, 1, 2, 3, 700, 2500, 5000, 9000]))))
    return text, cuts, finder(dev, text, cuts), rng


def _drawn(text, rng, n):
    """n patterns: two in three cut out of the text (8..40 bytes, word n-grams and their pieces), the rest absent."""
    out = []
    for i in range(n):
        m = int(rng.integers(4, 41))
        o = int(rng.integers(0, len(text) - m))
        out.append(text[o: o + m] if i % 3 else bytes(rng.integers(97, 123, m, dtype=np.uint8)) + b"#")
    return out


@pytest.mark.parametrize("n_pat", [0, 1, 33, 4096])
def test_set_sizes_against_the_reference(dev, words, n_pat):
    text, cuts, fd, rng = words
    pats = _drawn(text, np.random.default_rng(n_pat), n_pat)
    for ic in (False, True):
        got = check_find_set(dev, fd, text, [p.swapcase() for p in pats] if ic else pats, ic)
        assert int(got.counts.sum()) >= (2 * n_pat) // 3
        if n_pat == 0:
            assert got.ptr.tolist() == [0] and got.offsets.numel() == 0 and got.counts.numel() == 0 and got.offsets.device.type == dev.type


def test_lengths_1_2_3_go_through_the_same_api(dev, words):
    text, cuts, fd, rng = words
    pats = [b"e", b"th", b"the", b" a ", b"q", b"zz", text[100:104], text[5000:5017], b"E", b"Th"] + [bytes([97 + i, 97 + (7 * i) % 26]) for i in range(40)]
    for ic in (False, True):
        check_find_set(dev, fd, text, pats, ic)
        check_find_set(dev, fd, text, pats[:10], ic)                                   # at most 32: also StoreFinder.find's answer
        check_find_set(dev, fd, text, [b"e", b"th"], ic)                               # no pattern of 4 bytes or more at all


def test_a_thousand_patterns_sharing_their_first_eight_bytes(dev, words):
    text, cuts, fd, rng = words
    head = b"prefix__"
    pats = [head + b"%03d" % i + bytes([97 + i % 26]) * (i % 7) for i in range(1000)]
    body = bytearray(text[: 96 << 10])
    want_at = {}
    for i in range(0, 1000, 3):
        o = 200 + 90 * i
        body[o: o + len(pats[i])] = pats[i]
        want_at[i] = o
    body = bytes(body)
    c = [x for x in cuts if x < len(body)] + [len(body)]
    got = check_find_set(dev, finder(dev, body, c), body, pats)
    assert all(want_at[i] in got.offsets[got.ptr[i]: got.ptr[i + 1]].tolist() for i in want_at)


def test_many_patterns_in_one_directory_cell(dev, words):
    """200 four-letter keys whose hash has the same top dir_bits bits: one cell holds them all, the walk tells them apart."""
    from hmse_amd import find
    text, cuts, fd, rng = words
    n, bits = 200, 9                                                                   # 2^9 >= 2 * 200
    keys = {}
    for a in range(26 ** 4):
        k = bytes([97 + a % 26, 97 + a // 26 % 26, 97 + a // 676 % 26, 97 + a // 17576])
        cell = ((int.from_bytes(k, "little") * HASH) & 0xFFFFFFFF) >> (32 - bits)
        keys.setdefault(cell, []).append(k)
        if len(keys[cell]) == n:
            break
    pats = [k + b"-tail%d" % i for i, k in enumerate(keys[cell])]
    ps = find.PatternSet(pats, False, dev)
    assert ps.dir_bits == bits and int(ps.dir[cell + 1]) - int(ps.dir[cell]) == n
    body = bytearray(text[: 64 << 10])
    for i in range(0, n, 2):
        body[300 * i + 50: 300 * i + 50 + len(pats[i])] = pats[i]
    body = bytes(body)
    c = [x for x in cuts if x < len(body)] + [len(body)]
    got = check_find_set(dev, finder(dev, body, c), body, pats)
    assert got.counts.tolist() == [1 - i % 2 for i in range(n)]


def test_nested_prefixes_repeats_and_case(dev, words):
    text, cuts, fd, rng = words
    o = 12_345
    chain = [text[o: o + m] for m in range(4, 257)]                                   # all present at one offset
    got = check_find_set(dev, fd, text, chain)
    assert all(o in got.offsets[got.ptr[j]: got.ptr[j + 1]].tolist() for j in range(len(chain)))
    check_find_set(dev, fd, text, [c.upper() for c in chain[::5]], ic=True)
    same = [text[700:712]] * 50                                                        # the same pattern 50 times: each answered on its own
    got = check_find_set(dev, fd, text, same)
    assert len(set(got.counts.tolist())) == 1 and got.counts[0] >= 1 and got.offsets.numel() == 50 * int(got.counts[0])
    w = text[2000:2009]
    folded = [w, w.upper(), w.capitalize(), w.swapcase(), w[:4], w[:4].upper()]        # equal only after folding: distinct entries of the answer
    a = check_find_set(dev, fd, text, folded)
    b = check_find_set(dev, fd, text, folded, ic=True)
    assert b.counts.tolist()[:4] == [int(b.counts[0])] * 4 and int(b.counts[0]) >= int(a.counts[0]) >= 1 and a.counts.tolist()[1] == 0


def test_bytes_from_0x80_up_and_the_neighbours_of_the_letters(dev):
    odd = bytes([0xC1, 0xE1, 0x41, 0x61, 0x40, 0x60, 0x5B, 0x7B, 0x5A, 0x7A]) * 600
    cuts = [0, 7, 8, 8, 1000, 1003, 3000, len(odd)]
    fd = finder(dev, odd, cuts)
    groups = ([b"\xc1\xe1Aa", b"\xe1\xc1aA", b"\xc1\xe1aa@", b"a@`[{", b"A@`[{", b"a`@[{", b"@`[{Zz", b"`@{[zz", b"[{Zz\xc1", b"{[zz\xe1", b"Zz\xc1\xe1Aa@`"],
              [odd[i: i + 10] for i in range(10)] + [odd[i: i + 10].swapcase() for i in range(10)])
    for pats in groups:
        for ic in (False, True):
            check_find_set(dev, fd, odd, pats, ic)
            check_scan(dev, odd, [0, 1000, len(odd)], pats, ic)
    from hmse_amd import find
    c = fd.count_set(find.PatternSet([b"\xc1\xe1Aa", b"\xc1\xe1aa", b"\xe1\xe1aa"], True, dev)).tolist()
    assert c == [600, 600, 0]


# ---- 3. hit lists ------------------------------------------------------------------------------------------------------------------------
def _raw_scan(dev, raw, raw_off, fs, cap, sentinel=-7):
    """hmse_findset_scan called directly: -> (rc, hits tensor of cap + 64 entries prefilled with the sentinel, n_hits, counts, status)."""
    import torch
    from hmse_amd import _lib
    raw_d, ro = _t(raw, dev), _t(np.asarray(raw_off, np.int64), dev)
    hits = torch.full((cap + 64,), sentinel, dtype=torch.int64, device=dev)
    nh = torch.full((1,), sentinel, dtype=torch.int64, device=dev)
    counts = torch.full((fs.n_ids,), sentinel, dtype=torch.int64, device=dev)
    status = torch.full((1,), sentinel, dtype=torch.int32, device=dev)
    hdr = fs.header()
    rc = _lib.hip_lib().hmse_findset_scan(raw_d.data_ptr(), raw_d.numel(), ro.data_ptr(), len(raw_off) - 1, None, C.byref(hdr), hdr.flags,
                                          hits.data_ptr(), cap, nh.data_ptr(), counts.data_ptr(), status.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, hits, int(nh.item()), counts.tolist(), int(status.item())


def test_scan_hit_list_that_runs_out(dev):
    from hmse_amd import find, ops
    rng = np.random.default_rng(3)
    raw = bytes(rng.integers(97, 100, 2 * T + 77, dtype=np.uint8))
    raw_off, pats = [0, T + 5, 2 * T + 77], [b"abca", b"ccab", b"abcabc"]
    ps = find.PatternSet(pats, False, dev)
    want, want_counts = _want_scan(ps, raw, raw_off)
    assert len(want) > 2000
    rc, hits, n, counts, status = _raw_scan(dev, raw, raw_off, ps.set, len(want) - 1)  # one short of n_hits
    assert rc == 0 and status == 1 and n == len(want) and counts == want_counts       # bit 0; n_hits and counts exact all the same
    assert (hits[len(want) - 1:] == -7).all()                                         # nothing behind the list
    first = _pairs(hits[: len(want) - 1])
    assert len(set(first)) == len(want) - 1 and set(first) <= set(want)
    rc, hits, n, counts, status = _raw_scan(dev, raw, raw_off, ps.set, 16)
    assert status == 1 and n == len(want) and counts == want_counts and (hits[16:] == -7).all() and set(_pairs(hits[:16])) <= set(want)
    raw_d, ro = _t(raw, dev), _t(np.asarray(raw_off, np.int64), dev)
    h, n2, c2 = ops.findset_scan(raw_d, ro, None, ps.set, hits_cap=len(want) - 1)      # the wrapper's second call, with hits_cap = n_hits
    assert _pairs(h) == want and n2 == n and c2.tolist() == want_counts
    rc, hits, n, counts, status = _raw_scan(dev, raw, raw_off, ps.set, len(want))     # an exact list does not run out
    assert status == 0 and _pairs(hits[:n]) == want and (hits[n:] == -7).all()
    rc, hits, n, counts, status = _raw_scan(dev, raw, raw_off, ps.set, 0)             # count-only
    assert rc == 0 and status == 0 and n == len(want) and counts == want_counts and (hits == -7).all()


# ---- 4. inconsistent input ---------------------------------------------------------------------------------------------------------------
def test_inconsistent_tables_and_damaged_sets_set_bit_1_and_leave_the_outputs_alone(dev):
    import dataclasses
    import torch
    from hmse_amd import _lib, find, ops
    lib = _lib.hip_lib()
    raw = b"abcdabcdabcdabcd"
    pats = [b"abcd", b"cdab", b"bcdabc", b"dabcdab", b"abcdabcd", b"zzzz", b"zzzy"]
    ps = find.PatternSet(pats, False, dev)
    rc, hits, n, counts, status = _raw_scan(dev, raw, [0, 8, 16], ps.set, 32)
    want, want_counts = _want_scan(ps, raw, [0, 8, 16])
    assert rc == 0 and status == 0 and n == len(want) > 5 and counts == want_counts and _pairs(hits[:n]) == want   # the good call, for contrast
    for raw_off in ([0, 8, 4, 16], [0, 8, 17], [9, 8, 16]):                            # descending; records beyond raw_bytes
        rc, hits, n, counts, status = _raw_scan(dev, raw, raw_off, ps.set, 32)
        assert rc == 0 and status == 2 and n == 0 and counts == [0] * 7 and (hits == -7).all()
        with pytest.raises(ops.HmseError, match="inconsistent"):
            ops.findset_scan(_t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), None, ps.set)

    def damaged(**kw):
        new = {}
        for f, (i, v) in kw.items():
            t = getattr(ps.set, f).clone()
            t[i] = v
            new[f] = t
        return dataclasses.replace(ps.set, **new)
    top = int(ps.set.dir[-1])
    first_key = int(ps.set.ukey[0])
    sets = {"a descending directory": damaged(dir=(1, top + 3)), "a directory that ends early": damaged(dir=(-1, top - 1)),
            "an id out of range": damaged(uid=(2, ps.n_unique)), "a negative id": damaged(uid=(0, -1)),
            "a key that is not its pattern's first bytes": damaged(ukey=(0, first_key ^ 0x100)),
            "a length of 3": damaged(uoff=(1, int(ps.set.uoff[0]) + 3)), "bytes outside upat": damaged(uoff=(-1, ps.set.upat.numel() + 9)),
            "a descending byte range": damaged(uoff=(3, 0)), "a length above max_len": dataclasses.replace(ps.set, max_len=7),
            "a key without its bit": dataclasses.replace(ps.set, bitmap=torch.zeros_like(ps.set.bitmap))}
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    stream = torch.cuda.current_stream().cuda_stream
    raw_d, good_ro, good_cu, good_sl = _t(raw, dev), [0, 8, 16], [0, 8, 16, 24], [0, 1, 0]
    for name, fs in sets.items():
        rc, hits, n, counts, status = _raw_scan(dev, raw, [0, 8, 16], fs, 32)
        assert rc == 0 and status == 2 and n == 0 and counts == [0] * 7 and (hits == -7).all(), name
        with pytest.raises(ops.HmseError, match="inconsistent"):
            ops.findset_seams(raw_d, d(good_ro), d(good_cu), d(good_sl), fs)
    hdr = ps.set.header()
    for ro, cu, sl in (([0, 8, 16], [0, 8, 16, 24], [0, 2, 0]), (good_ro, [0, 8, 7, 15], good_sl), ([0, 9, 16], good_cu, good_sl),
                       (good_ro, [0, 8, 16, 25], good_sl), ([0, 8, 16], good_cu, [0, 1, -1]), (good_ro, [0, 8, 16, (1 << 40) + 8], good_sl)):
        hits = torch.full((64,), -7, dtype=torch.int64, device=dev)
        nh, counts, status = torch.full((1,), -7, dtype=torch.int64, device=dev), torch.full((7,), -7, dtype=torch.int64, device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev)
        ro_d, cu_d, sl_d = d(ro), d(cu), d(sl)
        rc = lib.hmse_findset_seams(raw_d.data_ptr(), 16, ro_d.data_ptr(), 2, cu_d.data_ptr(), sl_d.data_ptr(), 3, C.byref(hdr), 0,
                                    hits.data_ptr(), 64, nh.data_ptr(), counts.data_ptr(), status.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0 and int(status.item()) == 2 and int(nh.item()) == 0 and counts.tolist() == [0] * 7 and (hits == -7).all(), (ro, cu, sl)
        out = torch.full((64,), -7, dtype=torch.int64, device=dev)
        sorted_hits, chunk_out = d([0 << B, 4 << B, 8 << B]), d([0, 2, 3, 5])
        rc = lib.hmse_findset_place(sorted_hits.data_ptr(), 3, ro_d.data_ptr(), 2, cu_d.data_ptr(), sl_d.data_ptr(), 3, chunk_out.data_ptr(),
                                    out.data_ptr(), 64, status.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0 and int(status.item()) == 2 and (out == -7).all(), (ro, cu, sl)
    # the same calls with consistent tables go through; a chunk_out that is not the records' hit counts is bit 1, a short output bit 0
    ro_d, cu_d, sl_d = d(good_ro), d(good_cu), d(good_sl)
    sh, sn, sc = ops.findset_seams(raw_d, ro_d, cu_d, sl_d, ps.set)
    assert sn == len(ref.split(b"abcdabcd" * 3, pats, good_cu)[1]) and sn > 0
    sorted_hits = d([0 << B, 4 << B, 8 << B, 12 << B])
    assert [int(h) >> B for h in ops.findset_place(sorted_hits, ro_d, cu_d, sl_d, d([0, 2, 4, 6]), 6).tolist()] == [0, 4, 8, 12, 16, 20]
    with pytest.raises(ops.HmseError, match="inconsistent"):
        ops.findset_place(sorted_hits, ro_d, cu_d, sl_d, d([0, 2, 5, 7]), 7)
    with pytest.raises(ops.HmseError, match="inconsistent"):
        ops.findset_place(sorted_hits, ro_d, cu_d, sl_d, d([0, 2, 1, 3]), 3)
    with pytest.raises(ops.HmseError, match="exceeds"):
        ops.findset_place(sorted_hits, ro_d, cu_d, sl_d, d([0, 2, 4, 6]), 4)


# ---- 5. seams and place ------------------------------------------------------------------------------------------------------------------
SEAM_CASES = {
    "tiny chunks between normal ones": (b"abcdefghijklmnopqrstuvwxyz" * 40, [0, 300, 301, 303, 306, 306, 700, 701, 701, 701, 702, 1040]),
    "one chunk": (b"abcdabcdabcd", [0, 12]),
    "empty chunks only around one": (b"abcdabcdabcd", [0, 0, 12, 12]),
    "every byte its own chunk": (b"abcdabcdabcdabcd", list(range(17))),
    "chunks of two bytes": (b"abcdefabcdefabcdef", list(range(0, 19, 2))),
}


@pytest.mark.parametrize("name", sorted(SEAM_CASES))
def test_seams_and_place_on_synthetic_chunk_maps(dev, name):
    corpus, cuts = SEAM_CASES[name]
    pats = [corpus[o: o + m] for o, m in ((0, 4), (1, 5), (2, 6), (5, 4), (3, 9))] + [b"zabc", corpus[-4:], corpus[-3:] + b"\x00", corpus[-5:-1] + b"!"]
    pats += [corpus[c - 3: c + 5] for c in cuts if 3 <= c <= len(corpus) - 5][:8]
    for ic in (False, True):
        want_in, want_seam = pipeline(dev, corpus, cuts, [p.upper() if ic else p for p in pats], ic)
        got = check_find_set(dev, finder(dev, corpus, cuts), corpus, [p.upper() if ic else p for p in pats], ic)
    if name.startswith(("tiny", "every", "chunks")):
        assert want_seam
    # a match ending exactly at N is found, one that would need a byte past N is not (pattern 6 / patterns 7 and 8)
    assert len(corpus) - 4 in got.offsets[got.ptr[6]: got.ptr[7]].tolist() and got.counts[7:9].tolist() == [0, 0]


def test_seams_long_patterns_and_duplicate_chunks(dev):
    rng = np.random.default_rng(11)
    block = bytes(rng.integers(97, 123, 300, dtype=np.uint8))
    corpus = block + b"X" * 5 + block + block + b"YZ" + block[:100]
    # a 256-byte pattern running over five chunks (100 | 60 | 0 | 1 | 80 | ...), duplicate chunks (one record, three places), the last chunk
    cuts = [0, 100, 160, 160, 161, 241, 300, 305, 405, 465, 465, 466, 546, 605, 705, 765, 766, 846, 905, 907, 1007]
    assert cuts[-1] == len(corpus)
    pats = [corpus[50: 306], corpus[40: 295], block[90:110], block[:100], b"X" * 5, block[297:] + b"X", corpus[-100:], corpus[-101:], b"YZ" + block[:3]]
    assert len(pats[0]) == 256 and len(pats[1]) == 255
    want_in, want_seam = pipeline(dev, corpus, cuts, pats)                            # (ids of the UNIQUE patterns: 3 and 6 are equal)
    assert (50, 0) in want_seam and (0, 3) in want_in and (305, 3) in want_in and (605, 3) in want_in and (907, 3) in want_in and (906, 6) in want_seam
    pipeline(dev, corpus, cuts, [p.swapcase() for p in pats], ic=True)
    got = check_find_set(dev, finder(dev, corpus, cuts), corpus, pats)
    of = lambda j: got.offsets[got.ptr[j]: got.ptr[j + 1]].tolist()
    assert of(0) == [50] and of(3) == [0, 305, 605, 907] and of(6) == of(3) and of(7) == [906]


def test_empty_tables_and_empty_sets(dev):
    import torch
    from hmse_amd import find, ops
    z = lambda n, dt=torch.int64: torch.zeros(n, dtype=dt, device=dev)
    ps = find.PatternSet([b"abcd", b"ab"], False, dev)
    h, n, c = ops.findset_seams(z(0, torch.uint8), z(1), z(1), z(0), ps.set)
    assert h.numel() == 0 and n == 0 and c.tolist() == [0, 0]
    assert ops.findset_place(z(0), z(1), z(1), z(0), z(1), 0).numel() == 0
    h, n, c = ops.findset_scan(z(0, torch.uint8), z(1), None, ps.set)
    assert h.numel() == 0 and n == 0 and c.tolist() == [0, 0]
    for empty in (find.PatternSet([], False, dev), find.PatternSet([b"ab", b"c"], True, dev)):   # no entry of 4 bytes or more
        assert empty.n_entries == 0
        raw = _t(b"abcdabcd", dev)
        h, n, c = ops.findset_scan(raw, _t(np.array([0, 8], np.int64), dev), None, empty.set)
        assert h.numel() == 0 and n == 0 and c.tolist() == [0] * empty.n_unique
        h, n, c = ops.findset_seams(raw, _t(np.array([0, 8], np.int64), dev), _t(np.array([0, 8], np.int64), dev), z(1), empty.set)
        assert n == 0 and c.tolist() == [0] * empty.n_unique
    fd = finder(dev, b"", [0])
    f = fd.find_set(ps)
    assert f.counts.tolist() == [0, 0] and f.ptr.tolist() == [0, 0, 0] and f.offsets.numel() == 0 and fd.count_set(ps).tolist() == [0, 0]
    with pytest.raises(ValueError, match="PatternSet"):
        fd.find_set([b"abcd"])
    with pytest.raises(ValueError, match="lives on"):
        fd.find_set(find.PatternSet([b"abcd"]))


# ---- 6. memory ---------------------------------------------------------------------------------------------------------------------------
def _memory_case():
    rng = np.random.default_rng(21)
    block = bytes(rng.integers(97, 101, 700, dtype=np.uint8))
    corpus = block + b"abcd" + block + bytes(rng.integers(97, 101, T + 300, dtype=np.uint8)) + block[:350]
    cuts = [0, 350, 700, 702, 704, 1054, 1404, 1404 + T, 1404 + T + 300, 1404 + T + 650]
    assert cuts[-1] == len(corpus)
    pats = [b"abcd", b"ABCDA", b"dcba", corpus[340:360], corpus[698:708], b"aaaa", b"aaaab", corpus[-9:], corpus[1400:1656]]
    return corpus, cuts, pats


MEMORY = [("zero", 0, False), ("ones", 0, False), ("random", 0, False), ("random", 1, False), ("random", 2, False), ("random", 3, False),
          ("random", 13, False), ("random", 0, True)]


@pytest.mark.parametrize("pattern,misalign,distrust", MEMORY)
def test_entry_points_depend_on_their_arguments_only(dev, monkeypatch, pattern, misalign, distrust):
    """Each of the three entry points on poisoned memory (outputs, status words and counts included: distrust = the wrapper's own fills
    are poisoned, too), with raw and upat off their alignment, the set's arrays between guard bands."""
    import torch
    from hmse_amd import find, ops
    corpus, cuts, pats = _memory_case()
    raw, raw_off, slot = tables(corpus, cuts)
    ar = A.Arena(dev, pattern, seed=17).install(monkeypatch, distrust_zeros=distrust, byte_misalign=misalign)
    i64 = lambda a: ar.place(np.asarray(a, np.int64))
    i32 = lambda a: ar.place(a.view(np.int32).copy())
    raw_d = ar.place(np.frombuffer(raw, np.uint8).copy(), misalign=misalign)
    ro, cu, sl = i64(raw_off), i64(cuts), i64(slot)
    mult_h = np.bincount(slot, minlength=len(raw_off) - 1).astype(np.int32)
    mult = ar.place(mult_h)
    for ic in (False, True):
        ps = find.PatternSet(pats, ic)
        fs = ops.FindSet(ar.place(ps.upat.copy(), misalign=misalign), i32(ps.uoff), i32(ps.ukey), i32(ps.uid), i32(ps.dir), i32(ps.bitmap),
                         ps.n_unique, ps.dir_bits, ps.max_len, ic)
        lg = _long(ps)
        win, wseam = ref.split(corpus, [p for _, p in lg], cuts, ic)
        want_in, want_seam = sorted((o, lg[j][0]) for o, j in win), sorted((o, lg[j][0]) for o, j in wseam)
        want_scan, want_counts = _want_scan(ps, raw, raw_off, mult_h.tolist())
        hits, n, counts = ops.findset_scan(raw_d, ro, mult, fs)
        assert _pairs(hits) == want_scan and n == len(want_scan) and counts.tolist() == want_counts
        assert ops.findset_scan(raw_d, ro, mult, fs, hits_cap=0)[2].tolist() == want_counts
        assert _pairs(ops.findset_scan(raw_d, ro, None, fs, hits_cap=5)[0]) == want_scan
        sh, sn, sc = ops.findset_seams(raw_d, ro, cu, sl, fs)
        assert _pairs(sh) == want_seam and sn == len(want_seam) and int(sc.sum()) == sn and sn > 0
        hs = ar.place(torch.sort(hits)[0])
        lo = torch.searchsorted(hs, ro << B)
        chunk_out = ar.place(torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((lo[1:] - lo[:-1])[sl], 0)]))
        placed = ops.findset_place(hs, ro, cu, sl, chunk_out, len(want_in))
        assert _pairs(placed) == want_in and [int(h) >> B for h in placed.tolist()] == [o for o, _ in want_in]
    ar.check()


@pytest.mark.parametrize("misalign", [0, 3])
def test_nothing_behind_raw_bytes_is_a_match(dev, monkeypatch, misalign):
    """raw_bytes ends inside the buffer after "...ab", with "cd" lying right behind it: no hit, and no guard band changes."""
    from hmse_amd import find, ops
    ar = A.Arena(dev, "random", seed=23).install(monkeypatch)
    ps = find.PatternSet([b"abcd", b"bcdc", b"..ab", b".abc"], False, dev)
    for n in (T + 2, 3 * S + 2, 4, 13):
        body = np.full(n, ord("."), np.uint8)
        body[-2:] = np.frombuffer(b"ab", np.uint8)
        raw, both = ar.place_with_tail(body, np.frombuffer(b"cd" * 40, np.uint8).copy(), misalign=misalign)
        assert both[n - 2: n + 2].cpu().numpy().tobytes() == b"abcd"
        ro = ar.place(np.array([0, n], np.int64))
        hits, nh, counts = ops.findset_scan(raw, ro, None, ps.set)
        assert _pairs(hits) == [(n - 4, 2)] and nh == 1 and counts.tolist() == [0, 0, 1, 0]
    # the seams read raw through the chunk map only: a last chunk that ends at raw_bytes, "cd" behind it
    body = np.frombuffer(b"....ab", np.uint8).copy()
    raw, both = ar.place_with_tail(body, np.frombuffer(b"cd" * 40, np.uint8), misalign=misalign)
    ro, cu, sl = ar.place(np.array([0, 5, 6], np.int64)), ar.place(np.array([0, 5, 6], np.int64)), ar.place(np.array([0, 1], np.int64))
    sh, sn, sc = ops.findset_seams(raw, ro, cu, sl, ps.set)
    assert _pairs(sh) == [(2, 2)] and sc.tolist() == [0, 0, 1, 0]
    ar.check()


# ---- 7. store level ----------------------------------------------------------------------------------------------------------------------
def _store_input():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import variants_dataset
    from hmse_amd import corpus
    w = corpus.wiki_synth(MIB, seed=42)
    return np.concatenate([w[: 600_000], w[100_000: 400_000],                         # a repeated 300 000-byte stretch: POINTER chunks
                           variants_dataset(w)[:300_000],                            # a near-duplicate family: DELTA records
                           np.full(100_000, ord("e"), np.uint8)])                    # many POINTERs to one record, every boundary a seam


def _ragged_seg_off(n, dev):
    import torch
    sizes = [MIB // 2, 1, 2, 3, 70, MIB // 2, 1, 70, 3, 2]
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
    half = 600_000 + 150_000                                                           # inside the repeated stretch: POINTERs across shards
    rs = ingest.ingest_shards_local([torch.from_numpy(p).to(dev) for p in (data[:half], data[half:])], cfg)
    st = manifest.Store.from_bytes(manifest.merge_manifests([manifest.build_manifest(r, i, 2) for i, r in enumerate(rs)]).to_bytes())
    out["two shards"] = (st, find.StoreFinder(st, dev))
    return cfg, data, out


@pytest.fixture(scope="module")
def store_patterns(stores):
    """2000 patterns over the store's input and their reference answers in both case modes, computed once."""
    cfg, data, out = stores
    rng = np.random.default_rng(9)
    b = data.tobytes()
    cuts = out["plain"][1].cuts.tolist()
    pats = [b[o: o + m] for m in (1, 2, 3) + LENGTHS for o in (int(rng.integers(0, len(b) - 256)),)]      # 9: every boundary length
    pats += [b[c - 3: c + 5] for c in cuts[1:-1: max(1, (len(cuts) - 2) // 12)][:12]]                 # 12: straddling a cut
    pats += [b"e" * 4, b"eeeee", b"e" * 256, b"e" * 255 + b"x", b" the ", b"The ", b"of", b"\n", b"e", b"ee", b"and "]   # frequent ones; the run
    pats = pats[:32]
    assert len(pats) == 32
    while len(pats) < 2000:
        m = int(rng.integers(6, 49))
        o = int(rng.integers(0, len(b) - m))
        pats.append(b[o: o + m] if len(pats) % 2 else bytes(rng.integers(97, 123, m, dtype=np.uint8)))    # half from the corpus, half absent
    want = {ic: ref.find(b, [p.swapcase() for p in pats] if ic else pats, ic) for ic in (False, True)}
    return pats, want


@pytest.mark.parametrize("ic", [False, True])
@pytest.mark.parametrize("name", ["plain", "ragged", "two shards"])
def test_store_finder_set_equals_the_reference(stores, store_patterns, dev, name, ic):
    import torch
    from hmse_amd import KIND_DELTA, KIND_POINTER, find
    cfg, data, out = stores
    m, fd = out[name]
    if name != "two shards":
        kinds, lens = m.chunk_map["kind"], m.chunk_map["raw_length"]
        assert (kinds == KIND_POINTER).sum() > 20 and (kinds == KIND_DELTA).sum() > 2
        if name == "ragged":
            assert (lens < cfg.min_size).sum() >= 8 and {1, 2, 3, 70} <= set(lens.tolist())
    else:
        assert any((s.chunk_map["shard"] != i).any() for i, s in enumerate(m.shards))   # a chunk of one shard stored on the other
    assert fd.n_bytes == data.size and int(fd.raw.numel()) < data.size - 300_000      # the scan reads unique bytes only
    pats, want = store_patterns
    q = [p.swapcase() for p in pats] if ic else pats
    ps = find.PatternSet(q, ic, dev)
    assert ps.n_patterns == 2000 and ps.resident_bytes > 64 << 10
    got = fd.find_set(ps)
    assert got.counts.tolist() == want[ic][0] and got.ptr.tolist() == want[ic][1]
    assert got.offsets.tolist() == want[ic][2]
    assert fd.count_set(ps).tolist() == want[ic][0]
    sub = fd.find_set(find.PatternSet(q[:32], ic, dev))                                # a 32-pattern subset: StoreFinder.find's answer, too
    old = fd.find(q[:32], ignore_case=ic)
    assert all(torch.equal(getattr(old, f), getattr(sub, f)) for f in ("ptr", "offsets", "counts"))
    assert sub.counts.tolist() == want[ic][0][:32]


def test_store_finder_set_limits_and_the_one_off_form(stores, dev, monkeypatch):
    from hmse_amd import find, manifest, ops
    cfg, data, out = stores
    m, fd = out["plain"]
    pats = [b"eeee", b" the ", b"e"] + [b"absent-%d" % i for i in range(20)]
    ps = find.PatternSet(pats, False, dev)
    monkeypatch.setattr(ops, "findset_place", lambda *a, **k: pytest.fail("materialised before max_hits was checked"))
    with pytest.raises(ValueError, match=r"^find: (\d+) occurrences exceed max_hits = 10; the largest counts: pattern \d+: \d+(, pattern \d+: \d+){9}$"):
        fd.find_set(ps, max_hits=10)
    monkeypatch.undo()
    c = fd.count_set(ps).tolist()
    assert fd.find_set(ps, max_hits=sum(c)).offsets.numel() == sum(c)
    with pytest.raises(ValueError, match="exceed max_hits"):
        fd.find_set(ps, max_hits=sum(c) - 1)
    empty = find.StoreFinder(manifest.Store([]), dev)
    f = empty.find_set(ps)
    assert f.counts.tolist() == [0] * 23 and f.ptr.tolist() == [0] * 24 and f.offsets.numel() == 0 and empty.count_set(ps).tolist() == [0] * 23
    got = find.find_set(m, [b" the ", b" THE "], dev, ignore_case=True)                # the one-off form
    n = len(ref.occurrences(data.tobytes(), b" the ", True))
    assert got.counts.tolist() == [n, n] and got.offsets[:n].tolist() == got.offsets[n:].tolist()


# ---- 8. the densest chunking -------------------------------------------------------------------------------------------------------------
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
    pats = [b[c - 3: c + 5] for c in cuts[5:-1:6]] + [b[o: o + m] for m in (1, 2, 3) + LENGTHS for o in (int(rng.integers(0, len(b) - 256)),)] + [b"e", b" "]
    pats += [b[o: o + 300][:int(m)] for o, m in zip(rng.integers(0, len(b) - 300, 400), rng.integers(4, 257, 400))]
    for ic in (False, True):
        check_find_set(dev, fd, b, pats, ic)
