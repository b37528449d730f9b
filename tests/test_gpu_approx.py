"""GPU: approximate search (hmse_amd.find find_approx; hmse_approx_scan / hmse_approx_seams / hmse_approx_spans, hits laid out by
hmse_find_place) against Sellers' dynamic programme of tests/approx_ref.py — per kernel on synthetic tables, on poisoned / misaligned /
guarded memory (tests/arena.py), and on stores built the way tests/test_gpu_find.py builds its own: POINTER and DELTA records, tiny
chunks of ragged segments, a two-shard merged store, the densest chunking.  All results are compared bit for bit."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import arena as A
import approx_ref as ref
import lines_ref

pytestmark = pytest.mark.gpu

KIB = 1 << 10
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc", "approx.hip")).read()
S = int(re.search(r"constexpr int AX_STRIP = (\d+);", _SRC).group(1))                    # the scan's strip: bytes per lane and tile
T = S * int(re.search(r"constexpr int AX_NT = (\d+);", _SRC).group(1))                   # its tile: bytes per workgroup and trip
GRID = int(re.search(r"constexpr uint32_t AX_MAX_BLOCKS = (\d+);", _SRC).group(1))      # the scan's largest grid
ALPHA = b"abcdAB\n"


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


def _pats(dev, pats):
    off = [0]
    for p in pats:
        off.append(off[-1] + len(p))
    return _t(b"".join(pats), dev), off


def word(o, d, j):
    return (o << 8) | (d << 3) | j


def scan(dev, raw, raw_off, pats, ks, mult=None, ic=False, hits_cap=None):
    import torch
    from hmse_amd import ops
    pat, off = _pats(dev, pats)
    h, n, c = ops.approx_scan(_t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), None if mult is None else _t(np.asarray(mult, np.int32), dev),
                              pat, off, ks, ic, hits_cap)
    assert h.dtype == torch.int64 and c.dtype == torch.int64 and c.numel() == len(pats)
    return sorted(h.tolist()), n, c.tolist()


def check_scan(dev, raw, raw_off, pats, ks, mult=None, ic=False):
    """-> the sorted hit words, after comparing list, n_hits, counts and the count-only mode with the oracle."""
    want, want_counts = ref.scan_hits(raw, raw_off, pats, ks, mult, ic)
    got, n, counts = scan(dev, raw, raw_off, pats, ks, mult, ic)
    assert got == want and n == len(want) and counts == want_counts
    _, n0, counts0 = scan(dev, raw, raw_off, pats, ks, mult, ic, hits_cap=0)
    assert n0 == n and counts0 == counts
    return got


def tables(corpus, cuts):
    """A chunk map over `corpus`: exact dedupe of the chunks in order of first appearance -> (raw, raw_off, slot)."""
    recs, slot = [], []
    for k in range(len(cuts) - 1):
        c = bytes(corpus[cuts[k]: cuts[k + 1]])
        if c not in recs:
            recs.append(c)
        slot.append(recs.index(c))
    return b"".join(recs), [0] + [int(v) for v in np.cumsum([len(r) for r in recs])], slot


def occurrences(corpus, pats, ks, ic=False):
    return [ref.find_np(corpus, p, k, ic) for p, k in zip(pats, ks)]


def pipeline(dev, corpus, cuts, pats, ks, ic=False):
    """scan -> sort -> hmse_find_place, the seams and the spans of every hit over a synthetic chunk map, each against the oracle and its
    partition rule.  -> (scan ends, seam ends) as lists of (offset, errors, pattern)."""
    import torch
    from hmse_amd import ops
    raw, raw_off, slot = tables(corpus, cuts)
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    raw_d, ro, cu, sl = _t(raw if raw else np.zeros(0, np.uint8), dev), d(raw_off), d(cuts), d(slot)
    pat, off = _pats(dev, pats)
    occ = occurrences(corpus, pats, ks, ic)
    want_scan, want_seam = [], []
    for j, (p, k) in enumerate(zip(pats, ks)):
        a, b = ref.split(occ[j], len(p) + k, cuts)
        want_scan += [(o, e, j) for o, e in a]
        want_seam += [(o, e, j) for o, e in b]
    words = lambda trip: sorted(word(*x) for x in trip)
    mult = torch.bincount(sl, minlength=len(raw_off) - 1).to(torch.int32)
    hits, n, counts = ops.approx_scan(raw_d, ro, mult, pat, off, ks, ic)
    hits = torch.sort(hits)[0]
    lo = torch.searchsorted(hits, ro << 8)
    chunk_out = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((lo[1:] - lo[:-1])[sl], 0)])
    placed = ops.find_place(hits, ro, cu, sl, chunk_out, int(chunk_out[-1]))
    assert placed.tolist() == words(want_scan)                                         # as laid out: ascending by corpus offset
    assert counts.tolist() == [sum(1 for x in want_scan if x[2] == j) for j in range(len(pats))]
    sh, sn, sc = ops.approx_seams(raw_d, ro, cu, sl, pat, off, ks, ic)
    assert sorted(sh.tolist()) == words(want_seam) and sn == len(want_seam)
    assert sc.tolist() == [sum(1 for x in want_seam if x[2] == j) for j in range(len(pats))]
    n0, c0 = ops.approx_seams(raw_d, ro, cu, sl, pat, off, ks, ic, hits_cap=0)[1:]
    assert n0 == sn and c0.tolist() == sc.tolist()
    # the spans of every hit, scan and seam ends alike, in one call
    every = want_scan + want_seam
    if every:
        start, st = ops.approx_spans(raw_d, ro, cu, sl, pat, off, ic, d([word(*x) for x in every]))
        want_start = {}
        for j, p in enumerate(pats):
            mine = [(o, e) for o, e, jj in every if jj == j]
            want_start.update({(o, e, j): s for (o, e), s in zip(mine, ref.spans_np(corpus, p, mine, ic))})
        assert st == 0 and start.tolist() == [want_start[x] for x in every]
        assert all(len(pats[j]) - e <= o + 1 - want_start[(o, e, j)] <= len(pats[j]) + e for o, e, j in every)
    return want_scan, want_seam


# ---- 1. per kernel, synthetic tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 63, 64])
def test_scan_around_tile_and_strip_boundaries(dev, m):
    """One record of 3T bytes with matches of q{m} ending at EVERY offset of [T - W, T + W] and [S - W, S + W] (runs of one byte), for
    k = 0, 1 and min(m - 1, 16)."""
    for k in sorted({0, min(1, m - 1), min(m - 1, 16)}):
        W = m + k
        rec = np.full(3 * T, ord("."), np.uint8)
        rec[T - W - m: T + W + 1] = ord("q")
        rec[max(S - W - m, 0): S + W + 1] = ord("q")
        got = check_scan(dev, rec.tobytes(), [0, 3 * T], [b"q" * m], [k])
        ends = {h >> 8 for h in got}
        assert set(range(T - W, T + W + 1)) <= ends and set(range(max(S - W, W - 1), S + W + 1)) <= ends
        assert {(h >> 3) & 31 for h in got} == set(range(k + 1)) and {h & 7 for h in got} == {0}


def test_scan_64_equal_bytes_against_a_run_over_a_tile_edge(dev):
    """m = 64: the mask is all ones, the top bit is bit 63, the add's carry runs through the whole column and out of it."""
    rec = np.full(3 * T, ord("."), np.uint8)
    rec[T - 300: T + 300] = ord("a")                                                   # a run of 600 bytes straddling the tile edge
    rec[T + 10] = ord("b")
    rec[2 * T - 40: 2 * T - 8] = ord("a")
    rec[2 * T - 8: 2 * T + 24] = ord("b")
    pats, ks = [b"a" * 64, b"a" * 64, b"a" * 32 + b"b" * 32, b"a" * 63], [0, 3, 2, 0]
    got = check_scan(dev, rec.tobytes(), [0, 3 * T], pats, ks)
    assert sum(1 for h in got if h & 7 == 0) == (310 - 63) + (289 - 63) and word(2 * T + 23, 0, 2) in got   # the run, split by the b at T + 10
    assert {(h >> 3) & 31 for h in got if h & 7 == 1} == {0, 1, 2, 3}


def test_scan_ends_obey_the_rule_and_nothing_crosses_a_record(dev):
    for pats, ks in (([b"abbbc"], [1]), ([b"abbbcabb", b"bc"], [3, 0]), ([b"b"], [0]), ([b"abbbcabbbcabbbcabbbcabbbcabbbcab", b"cab"], [16, 2])):
        W = max(len(p) + k for p, k in zip(pats, ks))
        body = b"abbbc" * 120
        recs = [b"", body[:1], body[:max(W - 1, 0)], body[:W], body[:W + 1], b"", body[:2 * W + 3], body[:600]]
        # junk in front of raw_off[0] (the head of a match) and behind raw_off[n_rec]: a few bytes, then more than two tiles of it on either
        # side with three EMPTY records first — whole tiles in front of the records and behind them
        for front, n_empty, back in ((b"abbb", 0, b"cabbbcabbbc" * 8), (b"cabbb" * (2 * T // 5 + 40) + b"abbb", 3, b"cabbbcabbbc" * (2 * T // 11 + 8))):
            raw, raw_off = front, [len(front)] * (n_empty + 1)
            for rec in recs:                                                           # junk between the records, as records with mult 0
                raw += rec
                raw_off.append(len(raw))
                raw += b"abbbcabbb"
                raw_off.append(len(raw))
            mult = [5] * n_empty + [3, 0] * len(recs)
            raw += back
            assert len(front) > 2 * T or not n_empty
            got = check_scan(dev, raw, raw_off, pats, ks, mult)
            for h in got:
                p, j = h >> 8, h & 7
                r = max(i for i in range(len(raw_off) - 1) if raw_off[i] <= p)
                assert raw_off[r] <= p < raw_off[r + 1] and p + 1 - raw_off[r] >= len(pats[j]) + ks[j]
            assert len(got) > 0


def test_mult_count_only_and_a_list_that_runs_out(dev):
    import torch
    from hmse_amd import _lib
    pats, ks = [b"abcd", b"cdab"], [1, 0]
    raw = b"abcdabxd" * 25 + b"abcd" * 5 + b"zz" * 10
    raw_off, mult = [0, 200, 220, 240], [3, 0, 1000000]
    want, want_counts = ref.scan_hits(raw, raw_off, pats, ks, mult)
    unweighted = ref.scan_hits(raw, raw_off, pats, ks)[1]
    assert len(want) > 100 and want_counts[0] % 3 == 0 and unweighted != want_counts
    assert scan(dev, raw, raw_off, pats, ks, mult) == (want, len(want), want_counts)
    assert scan(dev, raw, raw_off, pats, ks, None) == (want, len(want), unweighted)
    assert scan(dev, raw, raw_off, pats, ks, mult, hits_cap=0) == ([], len(want), want_counts)
    assert scan(dev, raw, raw_off, pats, ks, mult, hits_cap=7) == (want, len(want), want_counts)   # ran out: ops repeats once with the exact capacity
    # the raw call: bit 0, exact counts, nothing written behind the capacity
    raw_d, ro, mu = _t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), _t(np.asarray(mult, np.int32), dev)
    pat, off = _pats(dev, pats)
    hits = torch.full((64,), -7, dtype=torch.int64, device=dev)
    nh, st = (torch.full((1,), -7, dtype=dt, device=dev) for dt in (torch.int64, torch.int32))
    cnt = torch.full((3,), -7, dtype=torch.int64, device=dev)
    rc = _lib.hip_lib().hmse_approx_scan(raw_d.data_ptr(), len(raw), ro.data_ptr(), 3, mu.data_ptr(), pat.data_ptr(), (C.c_uint32 * 3)(*off),
                                         (C.c_uint8 * 2)(*ks), 2, 0, hits.data_ptr(), 7, nh.data_ptr(), cnt.data_ptr(), st.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and int(st) == 1 and int(nh) == len(want) and cnt.tolist() == want_counts + [-7]
    assert (hits[7:] == -7).all() and set(hits[:7].tolist()) <= set(want)


def test_more_tiles_than_the_grid(dev):
    """(GRID + 3) tiles: the grid stride is taken.  The filler holds no byte of the pattern, so an end with only filler in its window is
    no occurrence (every alignment costs m > k) and the oracle looks at the planted places alone, each with W bytes of filler in front."""
    n = (GRID + 3) * T + 123
    rng = np.random.default_rng(4)
    raw = np.full(n, ord("."), np.uint8)
    at = np.sort(rng.choice(n // 64 - 2, 3000, replace=False) + 1) * 64
    variants = [b"Qz7xW", b"Qz7yW", b"Qz7W", b"Qy7yW", b"Qz7xxW"]
    pat, k = b"Qz7xW", 1
    want = []
    for i, o in enumerate(at.tolist()):
        v = variants[i % len(variants)]
        raw[o: o + len(v)] = np.frombuffer(v, np.uint8)
    raw[n - 5:] = np.frombuffer(pat, np.uint8)                                         # the last byte of raw ends a match
    blob = raw.tobytes()
    for o in at.tolist() + [n - 5]:
        want += [word(o - 16 + e, d, 0) for e, d in ref.find(blob[o - 16: o + 16], pat, k) if e >= len(pat) + k]
    got, nh, counts = scan(dev, blob, [0, n], [pat], [k])
    assert got == sorted(want) and nh == len(want) and counts == [len(want)] and len(want) > 3000
    assert len({o // T for o in at.tolist()}) > GRID and word(n - 1, 0, 0) in got


def test_eight_patterns_in_one_launch_and_equal_patterns(dev):
    rng = np.random.default_rng(8)
    pats = [b"a", b"ab", b"abcabcab", b"dcbadcbadcbadcba", b"abcd" * 8, bytes(rng.integers(97, 101, 63, dtype=np.uint8)),
            bytes(rng.integers(97, 101, 64, dtype=np.uint8)), b"abcabcab"]
    ks = [0, 1, 2, 5, 16, 9, 16, 2]
    corpus = bytearray(rng.integers(97, 101, 6000, dtype=np.uint8).tobytes())
    corpus = bytes(ref.plant(rng, corpus, pats, ks, b"abcd"))
    cuts = [0, 700, 1400, 1400 + 64, 3000, 3000, 4500, 6000]
    want_scan, want_seam = pipeline(dev, corpus, cuts, pats, ks)
    per = lambda j: sorted((o, e) for o, e, jj in want_scan + want_seam if jj == j)
    assert all(per(j) for j in range(8)) and per(2) == per(7)                          # equal patterns are answered each on its own
    for n_pat in (1, 2, 3, 5):                                                        # every instantiation of the scan kernel
        check_scan(dev, corpus, [0, len(corpus)], pats[2: 2 + n_pat], ks[2: 2 + n_pat])


def test_seams_over_tiny_and_empty_chunks_chains_and_both_ends_of_the_corpus(dev):
    rng = np.random.default_rng(6)
    pats, ks = [b"abcdabcdab", b"dcba", b"bd"], [2, 1, 0]
    W = 12
    corpus = bytearray(rng.integers(97, 101, 1500, dtype=np.uint8).tobytes())
    corpus = ref.plant(rng, corpus, pats, ks, b"abcd")
    corpus[:10] = pats[0]                                                              # chunk 0: the start clamps at the corpus's first byte
    corpus[-10:] = pats[0]                                                             # the last chunk ends at N
    corpus[400:410] = pats[0]                                                          # a match lying across three chunks: 400..402, 403..406, 407..
    corpus = bytes(corpus)
    lens = [0, 1, 2, W - 1] + [1] * (2 * W + 5) + [0, 2, 0, 0, 1, W, W + 1]            # a chain of tiny chunks longer than 2 W
    cuts = [0] + [int(v) for v in np.cumsum(lens)]
    assert cuts[-1] < 400
    cuts += [403, 407, 700, 700, 701, 1100, 1100 + W - 1, 1490, 1499, 1500, 1500, 1500]
    want_scan, want_seam = pipeline(dev, corpus, cuts, pats, ks)
    assert (9, 0, 0) in want_seam and (409, 0, 0) in want_seam and (1499, 0, 0) in want_seam and want_scan
    assert {0, 1} <= {j for _, _, j in want_seam}
    pipeline(dev, corpus, [0] + list(range(1, 1501)), pats, ks)                        # the densest map: every end is a seam end
    pipeline(dev, corpus, [0, 1500], [b"b"], [0])                                      # W = 1: no seam work at all


def test_ignore_case_folds_a_to_z_and_nothing_else(dev):
    pats, ks = [b"a@[`{\xc1Z", b"Q\xe1q"], [1, 0]
    corpus = (b"..A@[`{\xc1z..a`{@[\xe1z..a@[`{\xe1Z..A@{`[\xc1z..q\xe1Q..q\xc1Q..a@[`\xc1z..") * 6
    cuts = [0, 7, 20, 33, 34, 60, 61, len(corpus)]
    for ic in (True, False):
        want_scan, want_seam = pipeline(dev, corpus, cuts, pats, ks, ic)
        ends = {(o, e, j) for o, e, j in want_scan + want_seam if o < 70}
        if ic:
            assert {(8, 0, 0), (26, 1, 0), (64, 0, 0), (40, 0, 1)} <= ends and (18, 1, 0) not in ends and (45, 0, 1) not in ends   # \xe1 is not \xc1, ` is not @
        else:
            assert ends == {(26, 1, 0)}


def test_spans_flag_hits_that_cannot_be(dev):
    from hmse_amd import ops
    corpus = b"..abcd..abxd..a"
    raw, raw_off, slot = tables(corpus, [0, 5, 9, len(corpus)])
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    pat, off = _pats(dev, [b"abcd", b"xd"])
    args = (_t(raw, dev), d(raw_off), d([0, 5, 9, len(corpus)]), d(slot), pat, off, False)
    good = [word(5, 0, 0), word(11, 1, 0), word(11, 0, 1), word(4, 1, 0), word(14, 3, 0)]
    start, st = ops.approx_spans(*args, d(good))
    assert st == 0 and start.tolist() == [2, 8, 10, 2, 14] == [ref.span(corpus, p, o, e) for o, e, p in ((5, 0, b"abcd"), (11, 1, b"abcd"), (11, 0, b"xd"), (4, 1, b"abcd"), (14, 3, b"abcd"))]
    N = len(corpus)
    for bad in (word(N, 0, 0), word(N + 12345, 1, 1), word(5, 0, 2), word(11, 0, 0), word(3, 0, 1), word(0, 0, 0), word(0, 3, 0)):
        start, st = ops.approx_spans(*args, d(good[:2] + [bad] + good[2:]))
        assert st == 1 and start.tolist() == [2, 8, (bad >> 8) + 1, 10, 2, 14]
    z = ops.approx_spans(*args, d([]))
    assert z[0].numel() == 0 and z[1] == 0


def test_empty_tables(dev):
    import torch
    from hmse_amd import ops
    z = lambda n, dt=torch.int64: torch.zeros(n, dtype=dt, device=dev)
    pat, off = _pats(dev, [b"ab", b"abc"])
    h, n, c = ops.approx_seams(z(0, torch.uint8), z(1), z(1), z(0), pat, off, [1, 1])
    assert h.numel() == 0 and n == 0 and c.tolist() == [0, 0]
    h, n, c = ops.approx_scan(z(0, torch.uint8), z(1), None, pat, off, [1, 1])
    assert h.numel() == 0 and n == 0 and c.tolist() == [0, 0]
    start, st = ops.approx_spans(z(0, torch.uint8), z(1), z(1), z(0), pat, off, False, torch.tensor([5 << 8], device=dev))
    assert start.tolist() == [6] and st == 1                                           # an empty corpus: every offset lies outside it


def _raw_calls(dev, raw, raw_off, cuts, slot, pats, ks):
    """The three entry points on outputs poisoned with -7 -> [(rc, status, n_hits, counts, outputs untouched)]."""
    import torch
    from hmse_amd import _lib
    lib, stream = _lib.hip_lib(), torch.cuda.current_stream().cuda_stream
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    raw_d, ro, cu, sl = _t(raw, dev), d(raw_off), d(cuts), d(slot)
    pat, off = _pats(dev, pats)
    po, kk, P = (C.c_uint32 * len(off))(*off), (C.c_uint8 * len(ks))(*ks), len(pats)
    out = []
    for which in ("scan", "seams", "spans"):
        hits = torch.full((64,), -7, dtype=torch.int64, device=dev)
        nh, st = (torch.full((1,), -7, dtype=dt, device=dev) for dt in (torch.int64, torch.int32))
        cnt = torch.full((P,), -7, dtype=torch.int64, device=dev)
        if which == "scan":
            rc = lib.hmse_approx_scan(raw_d.data_ptr(), len(raw), ro.data_ptr(), len(raw_off) - 1, None, pat.data_ptr(), po, kk, P, 0, hits.data_ptr(), 64,
                                      nh.data_ptr(), cnt.data_ptr(), st.data_ptr(), stream)
        elif which == "seams":
            rc = lib.hmse_approx_seams(raw_d.data_ptr(), len(raw), ro.data_ptr(), len(raw_off) - 1, cu.data_ptr(), sl.data_ptr(), len(slot),
                                       pat.data_ptr(), po, kk, P, 0, hits.data_ptr(), 64, nh.data_ptr(), cnt.data_ptr(), st.data_ptr(), stream)
        else:
            words = d([word(3, 0, 0), word(11, 0, 0)])
            rc = lib.hmse_approx_spans(raw_d.data_ptr(), len(raw), ro.data_ptr(), len(raw_off) - 1, cu.data_ptr(), sl.data_ptr(), len(slot),
                                       pat.data_ptr(), po, P, 0, words.data_ptr(), 2, hits.data_ptr(), st.data_ptr(), stream)
            nh[0], cnt[:] = 0, 0
        torch.cuda.synchronize()
        out.append((rc, int(st), int(nh), cnt.tolist(), bool((hits == -7).all())))
    return out


def test_inconsistent_tables_set_bit_1_and_nothing_is_written(dev):
    from hmse_amd import ops
    raw, raw_off, cuts, slot = b"abcdabcdabcdabcd", [0, 8, 16], [0, 8, 16, 24], [0, 1, 0]
    pats, ks = [b"abcd", b"cdab"], [1, 0]
    good = _raw_calls(dev, raw, raw_off, cuts, slot, pats, ks)
    assert [c[:2] for c in good] == [(0, 0)] * 3 and good[0][2] > 0 and good[1][2] > 0 and not good[2][4]
    for ro, cu, sl in (([0, 8, 4], cuts, slot), ([0, 8, 17], cuts, slot), (raw_off, [0, 8, 7, 15], slot), (raw_off, cuts, [0, 2, 0]),
                       (raw_off, [0, 8, 16, 25], slot)):
        res = _raw_calls(dev, raw, ro, cu, sl, pats, ks)
        assert res[1] == (0, 2, 0, [0, 0], True) and res[2] == (0, 2, 0, [0, 0], True), (ro, cu, sl)
        if ro != raw_off:
            assert res[0] == (0, 2, 0, [0, 0], True)
    bad = [_t(np.asarray(a, np.int64), dev) for a in (raw_off, cuts, [0, 2, 0])]
    pat, off = _pats(dev, pats)
    with pytest.raises(ops.HmseError, match="inconsistent"):
        ops.approx_seams(_t(raw, dev), bad[0], bad[1], bad[2], pat, off, ks)
    with pytest.raises(ops.HmseError, match="inconsistent"):
        ops.approx_spans(_t(raw, dev), bad[0], bad[1], bad[2], pat, off, False, bad[0])
    with pytest.raises(ops.HmseError, match="inconsistent"):
        ops.approx_scan(_t(raw, dev), _t(np.asarray([0, 8, 17], np.int64), dev), None, pat, off, ks)


# ---- 2. memory ---------------------------------------------------------------------------------------------------------------------------
MEMORY = [("zero", 0, False), ("ones", 0, False), ("random", 0, False), ("random", 1, False), ("random", 3, False), ("random", 13, False),
          ("random", 0, True)]


@pytest.mark.parametrize("pattern,misalign,distrust", MEMORY)
def test_entry_points_depend_on_their_arguments_only(dev, monkeypatch, pattern, misalign, distrust):
    """The three entry points (and hmse_find_place behind the scan) on poisoned memory — outputs, status words and counts included —
    with raw and the patterns off their alignment, between guard bands."""
    import torch
    from hmse_amd import ops
    rng = np.random.default_rng(21)
    block = bytes(rng.integers(97, 101, 700, dtype=np.uint8))
    corpus = block + b"abcd" + block + bytes(rng.integers(97, 101, T + 300, dtype=np.uint8)) + block[:350]
    cuts = [0, 350, 700, 702, 704, 1054, 1404, 1404 + T, 1404 + T + 300, 1404 + T + 650]
    raw, raw_off, slot = tables(corpus, cuts)
    ar = A.Arena(dev, pattern, seed=17).install(monkeypatch, distrust_zeros=distrust, byte_misalign=misalign)
    i64 = lambda a: ar.place(np.asarray(a, np.int64))
    raw_d = ar.place(np.frombuffer(raw, np.uint8).copy(), misalign=misalign)
    ro, cu, sl = i64(raw_off), i64(cuts), i64(slot)
    mult = ar.place(np.bincount(slot, minlength=len(raw_off) - 1).astype(np.int32))
    for pats, ks in (([block[100:108], b"abcd"], [1, 0]), ([block[640:700] + b"abcd", block[40:104]], [8, 8])):
        off = [0]
        for p in pats:
            off.append(off[-1] + len(p))
        pat = ar.place(np.frombuffer(b"".join(pats), np.uint8).copy(), misalign=misalign)
        occ = occurrences(corpus, pats, ks)
        parts = [ref.split(occ[j], len(p) + ks[j], cuts) for j, p in enumerate(pats)]
        want_scan = sorted(word(o, e, j) for j, (a, _) in enumerate(parts) for o, e in a)
        want_seam = sorted(word(o, e, j) for j, (_, b) in enumerate(parts) for o, e in b)
        want_raw, want_counts = ref.scan_hits(raw, raw_off, pats, ks, mult.tolist())
        hits, n, counts = ops.approx_scan(raw_d, ro, mult, pat, off, ks)
        assert sorted(hits.tolist()) == want_raw and n == len(want_raw) and counts.tolist() == want_counts and sum(want_counts) == len(want_scan)
        assert ops.approx_scan(raw_d, ro, mult, pat, off, ks, hits_cap=0)[2].tolist() == want_counts
        assert sorted(ops.approx_scan(raw_d, ro, None, pat, off, ks, hits_cap=5)[0].tolist()) == want_raw
        sh, sn, sc = ops.approx_seams(raw_d, ro, cu, sl, pat, off, ks)
        assert sorted(sh.tolist()) == want_seam and sn == len(want_seam) == int(sc.sum()) and want_seam and want_raw
        hs = ar.place(torch.sort(hits)[0])
        lo = torch.searchsorted(hs, ro << 8)
        chunk_out = ar.place(torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((lo[1:] - lo[:-1])[sl], 0)]))
        placed = ops.find_place(hs, ro, cu, sl, chunk_out, len(want_scan))
        assert placed.tolist() == want_scan
        every = ar.place(torch.cat([placed, sh]))
        start, st = ops.approx_spans(raw_d, ro, cu, sl, pat, off, False, every)
        want_start = []
        for h in every.tolist():
            want_start.append(ref.spans_np(corpus, pats[h & 7], [(h >> 8, (h >> 3) & 31)])[0])
        assert st == 0 and start.tolist() == want_start
    ar.check()


@pytest.mark.parametrize("misalign", [0, 3])
def test_nothing_behind_raw_bytes_is_read_as_data(dev, monkeypatch, misalign):
    """raw_bytes ends inside the buffer after "...abc", with "d" and more lying right behind it: the column stops at raw_bytes."""
    from hmse_amd import ops
    ar = A.Arena(dev, "random", seed=23).install(monkeypatch)
    pat = ar.place(np.frombuffer(b"abcd", np.uint8).copy())
    for n in (T + 2, 3 * S + 2, 7, 13):
        body = np.full(n, ord("."), np.uint8)
        body[-3:] = np.frombuffer(b"abc", np.uint8)
        body[:4] = np.frombuffer(b"abcd", np.uint8)
        raw, both = ar.place_with_tail(body, np.frombuffer(b"dabcd" * 20, np.uint8).copy(), misalign=misalign)
        ro, cu, sl = (ar.place(np.array(v, np.int64)) for v in ([0, n], [0, n], [0]))
        hits, nh, _ = ops.approx_scan(raw, ro, None, pat, [0, 4], [0])
        assert sorted(hits.tolist()) == [word(3, 0, 0)] and nh == 1
        hits, nh, _ = ops.approx_scan(raw, ro, None, pat, [0, 4], [1])
        assert sorted(hits.tolist()) == [word(4, 1, 0), word(n - 1, 1, 0)] and nh == 2   # "abc" with one deletion, not "abcd"
        sh, sn, _ = ops.approx_seams(raw, ro, cu, sl, pat, [0, 4], [1])
        assert sorted(sh.tolist()) == [word(2, 1, 0), word(3, 0, 0)] and sn == 2
    ar.check()


# ---- 3. store level ----------------------------------------------------------------------------------------------------------------------
MARK = b"zq-marker-XY"
STORE_PATTERNS = [(MARK, 2), (b"2024-01-31", 1), (b"ERROR code id=7", 3), (b"ringing", 1), (b"192.168.0.1", 0)]
STORE_IC = True


def _planted(w):
    """The synthetic text with noisy copies of the store patterns written over it at seeded places."""
    w = w.copy()
    rng = np.random.default_rng(77)
    alphabet = b"abcXY019-. =:"
    for o in np.sort(rng.choice(w.size // 64 - 1, 800, replace=False)) * 64:
        p, k = STORE_PATTERNS[int(rng.integers(0, len(STORE_PATTERNS)))]
        s = ref.noisy(rng, p.swapcase() if rng.integers(0, 2) else p, int(rng.integers(0, k + 2)), alphabet)
        w[o: o + len(s)] = np.frombuffer(s, np.uint8)
    return w


SEG = 256 * KIB


def _store_input():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import variants_dataset
    from hmse_amd import corpus
    w = _planted(corpus.wiki_synth(1 << 20, seed=42))
    return np.concatenate([w[: 640 * KIB], w[100_000: 450_000],                       # a repeated 350 000-byte stretch: POINTER chunks
                           variants_dataset(w)[:300_000],                            # a near-duplicate family: DELTA records
                           np.full(100_000, ord("e"), np.uint8)])                    # many POINTERs to one record, every boundary a seam


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
    from hmse_amd import IngestConfig, find, ingest, manifest
    cfg = IngestConfig(seg_size=SEG)
    data = _store_input()
    d = torch.from_numpy(data).to(dev)
    out = {}
    for name, seg_off in (("plain", None), ("ragged", _ragged_seg_off(data.size, dev))):
        res = ingest.ingest_shard(d, cfg, seg_off)
        m = manifest.Manifest.from_bytes(manifest.build_manifest(res).to_bytes())
        out[name] = (m, find.StoreFinder(m, dev))
    return cfg, data, out


@pytest.fixture(scope="module")
def oracle(stores):
    """Per store pattern the oracle's [(last byte, errors)] over the stores' bytes — computed once."""
    b = stores[1].tobytes()
    return [ref.find_np(b, p, k, STORE_IC) for p, k in STORE_PATTERNS]


def _equals(found, want):
    counts = [len(w) for w in want]
    assert found.counts.tolist() == counts and found.ptr.tolist() == [0] + [int(v) for v in np.cumsum(counts)]
    assert found.offsets.tolist() == [o for w in want for o, _ in w] and found.errors.tolist() == [e for w in want for _, e in w]


@pytest.mark.parametrize("name", ["plain", "ragged"])
def test_find_approx_equals_the_oracle(stores, oracle, dev, name):
    import torch
    from hmse_amd import KIND_DELTA, KIND_POINTER, find
    cfg, data, out = stores
    m, fd = out[name]
    kinds, lens = m.chunk_map["kind"], m.chunk_map["raw_length"]
    assert (kinds == KIND_POINTER).sum() > 0 and (kinds == KIND_DELTA).sum() > 0
    if name == "ragged":
        assert {1, 2, 3, 70} <= set(lens.tolist())
    pats, ks = [p for p, _ in STORE_PATTERNS], [k for _, k in STORE_PATTERNS]
    assert all(len(w) > 20 for w in oracle) and any(e for w in oracle for _, e in w)
    got = fd.find_approx(pats, ks, STORE_IC)
    assert isinstance(got, find.ApproxFound) and isinstance(got, find.Found) and got.errors.dtype == torch.int64
    _equals(got, oracle)
    assert fd.count_approx(pats, ks, STORE_IC).tolist() == [len(w) for w in oracle]
    assert fd.count_approx(pats[1:2], ks[1], STORE_IC).tolist() == [len(oracle[1])]
    # k = 0 is the exact search, shifted to the last byte
    exact = fd.find(pats, STORE_IC)
    zero = fd.find_approx(pats, 0, STORE_IC)
    shift = torch.repeat_interleave(torch.tensor([len(p) - 1 for p in pats], device=dev), exact.counts)
    assert zero.offsets.tolist() == (exact.offsets + shift).tolist() and zero.counts.tolist() == exact.counts.tolist() and not zero.errors.any()
    assert exact.offsets.numel() > 50
    # the spans and their text
    b = data.tobytes()
    start, end = fd.spans(got)
    want_start = [s for (p, _), w in zip(STORE_PATTERNS, oracle) for s in ref.spans_np(b, p, w, STORE_IC)]
    assert start.tolist() == want_start and end.tolist() == [o + 1 for w in oracle for o, _ in w]
    text, off = fd.text((start, end))
    assert text.cpu().numpy().tobytes() == b"".join(b[s: e] for s, e in zip(want_start, end.tolist()))
    # from a best end to its line
    best = find.best_ends(got)
    want_best = [ref.best_ends(w) for w in oracle]
    _equals(best, want_best)
    lines = fd.grep_approx(pats[:3], ks[:3], STORE_IC, before=1)
    sub = want_best[:3]
    ptr = [0] + [int(v) for v in np.cumsum([len(w) for w in sub])]
    want_lines = lines_ref.lines(b, ([len(w) for w in sub], ptr, [o for w in sub for o, _ in w]), 0x0A, 1, 0)
    for f in ("ptr", "start", "end", "hits", "counts"):
        assert getattr(lines, f).tolist() == want_lines[f], f
    assert lines.flags.tolist() == want_lines["flags"]


def test_find_approx_groups_limits_and_edges(stores, oracle, dev):
    import torch
    from hmse_amd import find, manifest
    cfg, data, out = stores
    m, fd = out["plain"]
    pats, ks = [p for p, _ in STORE_PATTERNS], [k for _, k in STORE_PATTERNS]
    order = [0, 1, 2, 3, 4, 1, 0, 3, 2, 4, 1]                                          # eleven patterns: two groups, equal ones among them
    many = fd.find_approx([pats[i] for i in order], [ks[i] for i in order], STORE_IC)
    _equals(many, [oracle[i] for i in order])
    assert fd.count_approx([pats[i] for i in order], [ks[i] for i in order], STORE_IC).tolist() == [len(oracle[i]) for i in order]
    start, end = fd.spans(many)
    b = data.tobytes()
    assert start.tolist() == [s for i in order for s in ref.spans_np(b, pats[i], oracle[i], STORE_IC)]
    with pytest.raises(ValueError, match=r"counts per pattern: \[\d+, \d+\]"):
        fd.find_approx(pats[:2], ks[:2], STORE_IC, max_hits=10)
    n1 = len(oracle[1])
    assert fd.find_approx(pats[1:2], ks[1:2], STORE_IC, max_hits=n1).offsets.numel() == n1
    z = fd.find_approx([], 1)
    assert z.ptr.tolist() == [0] and z.offsets.numel() == 0 and z.errors.numel() == 0 and fd.count_approx([], 1).numel() == 0
    assert z.offsets.dtype == torch.int64 and z.offsets.device.type == "cuda"
    empty = find.StoreFinder(manifest.Store([]), dev)
    f = empty.find_approx(pats[:2], 1)
    assert f.counts.tolist() == [0, 0] and f.ptr.tolist() == [0, 0, 0] and f.offsets.numel() == 0 and empty.count_approx(pats[:1], 1).tolist() == [0]
    got = find.find_approx(m, pats[3:4], ks[3], dev, STORE_IC)                          # the one-off forms
    assert got.offsets.tolist() == [o for o, _ in oracle[3]]
    assert find.grep_approx(m, pats[3:4], ks[3], dev, STORE_IC).counts.tolist() == fd.lines(find.best_ends(got)).counts.tolist()


def test_two_shard_store_gives_the_one_shard_results(stores, oracle, dev):
    import torch
    from hmse_amd import find, ingest, manifest
    cfg, data, out = stores
    half = 640 * KIB + 175_000                                                       # inside the repeated stretch: POINTERs across shards
    rs = ingest.ingest_shards_local([torch.from_numpy(p).to(dev) for p in (data[:half], data[half:])], cfg)
    st = manifest.Store.from_bytes(manifest.merge_manifests([manifest.build_manifest(r, i, 2) for i, r in enumerate(rs)]).to_bytes())
    pats, ks = [p for p, _ in STORE_PATTERNS], [k for _, k in STORE_PATTERNS]
    _equals(find.StoreFinder(st, dev).find_approx(pats, ks, STORE_IC), oracle)


def test_smallest_chunk_sizes(dev):
    import torch
    from hmse_amd import IngestConfig, corpus, find, ingest, manifest
    cfg = IngestConfig(min_size=64, avg_size=256, max_size=1024, seg_size=1 << 16)
    w = _planted(corpus.wiki_synth(192 << 10, seed=7))
    data = np.concatenate([w, w[10_000: 10_000 + (64 << 10)]])
    res = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    fd = find.StoreFinder(manifest.Manifest.from_bytes(manifest.build_manifest(res).to_bytes()), dev)
    assert fd.cuts.numel() > 600
    b = data.tobytes()
    pats, ks = [p for p, _ in STORE_PATTERNS] + [b[5000:5064]], [k for _, k in STORE_PATTERNS] + [16]   # W = 80: most chunks are all seam ends
    want = [ref.find_np(b, p, k, STORE_IC) for p, k in zip(pats, ks)]
    assert all(want)
    got = fd.find_approx(pats, ks, STORE_IC)
    _equals(got, want)
    assert fd.count_approx(pats, ks, STORE_IC).tolist() == [len(w) for w in want]
    assert fd.spans(got)[0].tolist() == [s for p, w in zip(pats, want) for s in ref.spans_np(b, p, w, STORE_IC)]
