"""GPU: regular-expression search (hmse_amd.regex / hmse_amd.find; hmse_regex_scan / hmse_regex_seams, hits laid out by hmse_find_place)
against the `re` oracle of tests/regex_ref.py — per kernel on synthetic tables, on poisoned / misaligned / guarded memory
(tests/arena.py), and on stores built the way tests/test_gpu_find.py builds its own: POINTER and DELTA records, tiny chunks of ragged
segments, a two-shard merged store, the densest chunking.  All results are compared bit for bit."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import arena as A
import lines_ref
import regex_ref as ref

pytestmark = pytest.mark.gpu

MIB = 1 << 20
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc", "regex.hip")).read()
S = int(re.search(r"constexpr int RX_STRIP = (\d+);", _SRC).group(1))                    # the scan's strip: bytes per lane and tile
T = S * int(re.search(r"constexpr int RX_NT = (\d+);", _SRC).group(1))                   # its tile: bytes per workgroup and trip
GRID = int(re.search(r"constexpr uint32_t RX_MAX_BLOCKS = (\d+);", _SRC).group(1))      # the scan's largest grid


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


def _rx(dev, pattern, ic=False, dotall=False):
    from hmse_amd.regex import Regex
    return Regex(pattern, ic, dotall, device=dev)


def scan(dev, raw, raw_off, r, mult=None, hits_cap=None):
    import torch
    from hmse_amd import ops
    h, n, c = ops.regex_scan(_t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), None if mult is None else _t(np.asarray(mult, np.int32), dev),
                             r.rx, hits_cap)
    assert h.dtype == torch.int64 and c.dtype == torch.int64 and c.numel() == 1
    return sorted(h.tolist()), n, int(c[0])


def check_scan(dev, raw, raw_off, r, mult=None):
    """-> the hits as sorted (position, length) pairs, after comparing list, n_hits, count and the count-only mode with the oracle."""
    want, want_count = ref.scan_hits(raw, raw_off, r.pattern, r.reach, mult, r.ignore_case, r.dotall)
    got, n, count = scan(dev, raw, raw_off, r, mult)
    assert got == want and n == len(want) and count == want_count
    _, n0, count0 = scan(dev, raw, raw_off, r, mult, hits_cap=0)
    assert n0 == n and count0 == count
    return [(h >> 8, (h & 255) + 1) for h in got]


def tables(corpus, cuts):
    """A chunk map over `corpus`: exact dedupe of the chunks in order of first appearance -> (raw, raw_off, slot)."""
    chunks = [bytes(corpus[cuts[k]: cuts[k + 1]]) for k in range(len(cuts) - 1)]
    recs, slot = [], []
    for c in chunks:
        if c not in recs:
            recs.append(c)
        slot.append(recs.index(c))
    return b"".join(recs), [0] + [int(v) for v in np.cumsum([len(r) for r in recs])], slot


def pipeline(dev, corpus, cuts, r):
    """scan -> sort -> hmse_find_place and the seams over a synthetic chunk map, each against the partition rule of the oracle."""
    import torch
    from hmse_amd import ops
    raw, raw_off, slot = tables(corpus, cuts)
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    raw_d, ro, cu, sl = _t(raw if raw else np.zeros(0, np.uint8), dev), d(raw_off), d(cuts), d(slot)
    want_scan, want_seam = ref.split(corpus, ref.find(corpus, r.pattern, r.reach, r.ignore_case, r.dotall), r.reach, cuts)
    word = lambda pairs: [(o << 8) | (l - 1) for o, l in pairs]
    mult = torch.bincount(sl, minlength=len(raw_off) - 1).to(torch.int32)
    hits, n, count = ops.regex_scan(raw_d, ro, mult, r.rx)
    hits = torch.sort(hits)[0]
    lo = torch.searchsorted(hits, ro << 8)
    chunk_out = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((lo[1:] - lo[:-1])[sl], 0)])
    placed = ops.find_place(hits, ro, cu, sl, chunk_out, int(chunk_out[-1]))
    assert placed.tolist() == word(want_scan) and int(count[0]) == len(want_scan)      # as laid out: ascending by corpus offset
    sh, sn, sc = ops.regex_seams(raw_d, ro, cu, sl, r.rx)
    assert sorted(sh.tolist()) == word(want_seam) and sn == len(want_seam) and int(sc[0]) == sn
    assert ops.regex_seams(raw_d, ro, cu, sl, r.rx, hits_cap=0)[1] == sn
    return want_scan, want_seam


# ---- 1. per kernel, synthetic tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 255, 256])
def test_scan_around_tile_and_strip_boundaries(dev, m):
    """One record of 3T bytes with matches of q{m} starting at EVERY offset of [T - m, T + 1] and [S - m, S + 1] (runs of one byte)."""
    rec = np.full(3 * T, ord("."), np.uint8)
    rec[T - m: T + 1 + m] = ord("q")
    rec[max(S - m, 0): S + 1 + m] = ord("q")
    r = _rx(dev, b"q{%d}" % m)
    assert r.reach == m
    got = check_scan(dev, rec.tobytes(), [0, 3 * T], r)
    starts = {p for p, _ in got}
    assert set(range(T - m, T + 2)) <= starts and set(range(max(S - m, 0), S + 2)) <= starts and {l for _, l in got} == {m}


def test_scan_run_over_a_tile_edge_caps_every_length_at_256(dev):
    rec = np.full(3 * T, ord("."), np.uint8)
    rec[T - 300: T + 300] = ord("q")                                                   # a run of 600 bytes straddling the tile edge
    got = dict(check_scan(dev, rec.tobytes(), [0, 3 * T], _rx(dev, b"q+")))
    assert len(got) == 600 and all(got[T - 300 + i] == min(256, 600 - i) for i in range(600))   # capped, then shrinking to the run's end


def test_walks_that_end_at_the_overhang_s_last_byte_and_at_raw_bytes(dev):
    r = _rx(dev, b"a{256}")
    raw = np.full(T + 255, ord("."), np.uint8)
    raw[T - 1:] = ord("a")                                                             # the tile's last start, the overhang's last byte = raw_bytes
    assert check_scan(dev, raw.tobytes(), [0, T + 255], r) == [(T - 1, 256)]
    assert check_scan(dev, raw.tobytes() + b"a", [0, T + 256], r) == [(T - 1, 256), (T, 256)]
    assert check_scan(dev, raw.tobytes()[:-1], [0, T + 254], r) == []
    plus = _rx(dev, b"a+b")                                                            # reach 256: the record's last 255 starts are no scan starts
    raw = b"." * 100 + b"a" * 255 + b"b" + b"aab" + b"." * 253
    assert check_scan(dev, raw, [0, len(raw)], plus) == [(100 + i, 256 - i) for i in range(255)] + [(356, 3)]


def test_scan_starts_obey_the_rule_and_nothing_crosses_a_record(dev):
    for pat in (b"ab{3}c?", b"[ab]{4}", b"ab", b"b+", b"b"):
        r = _rx(dev, pat)
        R = r.reach
        body = (b"abbbc" * 120)
        recs = [b"", body[:1], body[:max(R - 1, 0)], body[:R], body[:R + 1], b"", body[:2 * R + 3], body[:600]]
        raw, raw_off = b"bbbb", [4]
        for rec in recs:                                                               # junk between the records, as records with mult 0
            raw += rec
            raw_off.append(len(raw))
            raw += b"abbbcabbb"
            raw_off.append(len(raw))
        mult = [1, 0] * len(recs)
        got = check_scan(dev, raw, raw_off, r, mult)
        ends = raw_off[1:]
        for p, l in got:
            e = min(x for x in ends if x > p)
            assert e - p >= R and p + l <= e
        assert len(got) > 0


def test_mult_count_only_and_a_list_that_runs_out(dev):
    import torch
    from hmse_amd import _lib, ops
    r = _rx(dev, b"[ab]c")
    raw = b"acbc" * 50 + b"ac" * 10 + b"zz" * 10
    raw_off, mult = [0, 200, 220, 240], [3, 0, 1000000]
    want, want_count = ref.scan_hits(raw, raw_off, r.pattern, r.reach, mult)
    assert len(want) == 110 and want_count == 300
    assert scan(dev, raw, raw_off, r, mult) == (want, 110, 300)
    assert scan(dev, raw, raw_off, r, None) == (want, 110, 110)
    assert scan(dev, raw, raw_off, r, mult, hits_cap=0) == ([], 110, 300)
    assert scan(dev, raw, raw_off, r, mult, hits_cap=7) == (want, 110, 300)            # ran out: ops repeats once with the exact capacity
    # the raw call: bit 0, exact counts, nothing written behind the capacity
    raw_d, ro, mu = _t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), _t(np.asarray(mult, np.int32), dev)
    hits = torch.full((64,), -7, dtype=torch.int64, device=dev)
    nh, cnt, st = (torch.full((1,), -7, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.int32))
    hdr = r.rx.header()
    rc = _lib.hip_lib().hmse_regex_scan(raw_d.data_ptr(), len(raw), ro.data_ptr(), 3, mu.data_ptr(), C.byref(hdr), hits.data_ptr(), 7,
                                        nh.data_ptr(), cnt.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and int(st) == 1 and int(nh) == 110 and int(cnt) == 300 and (hits[7:] == -7).all() and set(hits[:7].tolist()) <= set(want)


def test_every_position_of_a_tile_survives_the_first_step(dev):
    """[^\\n]*x over tiles without a newline: more survivors than one round of the hand-out (one per lane) holds — T of them."""
    raw = np.full(2 * T + 500, ord("a"), np.uint8)
    raw[::100] = ord("x")
    raw[T + 77] = ord("\n")
    got = check_scan(dev, raw.tobytes(), [0, raw.size], _rx(dev, rb"[^\n]*x"))
    assert len(got) > T


def test_more_tiles_than_the_grid(dev):
    n = (GRID + 3) * T + 123
    rng = np.random.default_rng(4)
    raw = np.full(n, ord("."), np.uint8)
    at = np.sort(rng.choice(n // 8 - 1, 3000, replace=False)) * 8                      # apart: no two overlap
    for i, ch in enumerate(b"Qz7"):
        raw[at + i] = ch
    raw[at[::2] + 3] = ord("9")
    r = _rx(dev, rb"Qz\d+")
    got, nh, count = scan(dev, raw.tobytes(), [0, n], r)
    want = [(int(o) << 8) | ((4 if i % 2 == 0 else 3) - 1) for i, o in enumerate(at) if n - int(o) >= r.reach]
    assert got == want and nh == len(want) and count == len(want) and len({o // T for o in at.tolist()}) > GRID


SEAM_CASES = [(b"ab+c", False), (b"[ab]{2,5}", False), (b"(ab|b)c?", True), (rb"a[^\n]*c", False), (b"c", False)]


@pytest.mark.parametrize("pat,ic", SEAM_CASES)
def test_seams_over_tiny_and_empty_chunks(dev, pat, ic):
    rng = np.random.default_rng(len(pat))
    corpus = bytes(np.frombuffer(b"abcAB\n", np.uint8)[rng.integers(0, 6, 900)]) + b"abbbbc" * 20 + b"ab"
    lens = []
    while sum(lens) < len(corpus):
        lens.append(int(rng.choice([0, 1, 2, 1, 2, 3, 7, 40, 300])))
    lens[-1] -= sum(lens) - len(corpus)
    cuts = [0] + [int(v) for v in np.cumsum(lens)] + [len(corpus)] * 2                # the last chunks are empty: N clips the walk
    r = _rx(dev, pat, ic)
    want_scan, want_seam = pipeline(dev, corpus, cuts, r)
    if r.reach > 1:
        assert want_seam and (want_scan or r.reach == 256)                             # (reach 256: nearly every chunk is all seam starts)
    else:
        assert not want_seam                                                           # reach = 1: no seam work


def test_a_match_running_over_five_chunks_and_duplicate_chunks(dev):
    rng = np.random.default_rng(11)
    block = bytes(rng.integers(97, 123, 300, dtype=np.uint8)).replace(b"q", b"r")
    corpus = block + b"Q" * 5 + block + block + b"YZ" + block[:100]
    cuts = [0, 100, 160, 160, 161, 241, 300, 305, 405, 465, 465, 466, 546, 605, 705, 765, 766, 846, 905, 907, 1007]
    assert cuts[-1] == len(corpus)
    r = _rx(dev, b"[a-z]{200,256}")
    want_scan, want_seam = pipeline(dev, corpus, cuts, r)
    assert (50, 250) in want_seam and (0, 256) in want_seam and (1006, 1) not in want_seam
    pipeline(dev, corpus, cuts, _rx(dev, b"Q+[a-z]{1,3}"))
    pipeline(dev, corpus, cuts, _rx(dev, b"[a-z]+", True))


def test_empty_tables(dev):
    import torch
    from hmse_amd import ops
    z = lambda n, dt=torch.int64: torch.zeros(n, dtype=dt, device=dev)
    r = _rx(dev, b"ab")
    h, n, c = ops.regex_seams(z(0, torch.uint8), z(1), z(1), z(0), r.rx)
    assert h.numel() == 0 and n == 0 and c.tolist() == [0]
    h, n, c = ops.regex_scan(z(0, torch.uint8), z(1), None, r.rx)
    assert h.numel() == 0 and n == 0 and c.tolist() == [0]


def _raw_calls(dev, raw, raw_off, cuts, slot, hdr):
    """Both entry points on outputs poisoned with -7 -> [(rc, status, n_hits, count, hits untouched)]."""
    import torch
    from hmse_amd import _lib
    lib, stream = _lib.hip_lib(), torch.cuda.current_stream().cuda_stream
    d = lambda a: _t(np.asarray(a, np.int64), dev)
    raw_d, ro, cu, sl = _t(raw, dev), d(raw_off), d(cuts), d(slot)
    out = []
    for which in ("scan", "seams"):
        hits = torch.full((64,), -7, dtype=torch.int64, device=dev)
        nh, cnt, st = (torch.full((1,), -7, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.int32))
        if which == "scan":
            rc = lib.hmse_regex_scan(raw_d.data_ptr(), len(raw), ro.data_ptr(), len(raw_off) - 1, None, C.byref(hdr), hits.data_ptr(), 64,
                                     nh.data_ptr(), cnt.data_ptr(), st.data_ptr(), stream)
        else:
            rc = lib.hmse_regex_seams(raw_d.data_ptr(), len(raw), ro.data_ptr(), len(raw_off) - 1, cu.data_ptr(), sl.data_ptr(), len(slot),
                                      C.byref(hdr), hits.data_ptr(), 64, nh.data_ptr(), cnt.data_ptr(), st.data_ptr(), stream)
        torch.cuda.synchronize()
        out.append((rc, int(st), int(nh), int(cnt), bool((hits == -7).all())))
    return out


def test_a_damaged_automaton_sets_bit_2_and_inconsistent_tables_bit_1(dev):
    import torch
    from hmse_amd import ops
    from hmse_amd.regex import Regex
    raw, raw_off, cuts, slot = b"abcdabcdabcdabcd", [0, 8, 16], [0, 8, 16, 24], [0, 1, 0]
    host = Regex(b"ab+c?")
    good = _rx(dev, b"ab+c?")
    assert [c[:2] for c in _raw_calls(dev, raw, raw_off, cuts, slot, good.rx.header())] == [(0, 0), (0, 0)]
    damaged = []
    t = host.table.copy(); t[host.n_classes + 1] = host.n_states; damaged.append((t, host.classmap))          # an entry >= n_states
    t = host.table.copy(); t[-1] = 0x8000 | (host.n_states + 5); damaged.append((t, host.classmap))
    t = host.table.copy(); t[0] = 1; damaged.append((t, host.classmap))                                        # a non-zero dead row
    t = host.table.copy(); t[host.n_classes - 1] = 0x8000; damaged.append((t, host.classmap))
    m = host.classmap.copy(); m[200] = host.n_classes; damaged.append((host.table, m))                         # a class out of range
    for t, m in damaged:
        bad = ops.Regex(_t(t.view(np.int16), dev), _t(m, dev), host.n_states, host.n_classes, host.reach)
        assert _raw_calls(dev, raw, raw_off, cuts, slot, bad.header()) == [(0, 4, 0, 0, True)] * 2
        with pytest.raises(ops.HmseError, match="bad automaton"):
            ops.regex_scan(_t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), None, bad)
    for ro, cu, sl in (([0, 8, 4], cuts, slot), ([0, 8, 17], cuts, slot), (raw_off, [0, 8, 7, 15], slot), (raw_off, cuts, [0, 2, 0]),
                       (raw_off, [0, 8, 16, 25], slot)):
        res = _raw_calls(dev, raw, ro, cu, sl, good.rx.header())
        assert res[1] == (0, 2, 0, 0, True), (ro, cu, sl)
        if ro != raw_off:
            assert res[0] == (0, 2, 0, 0, True)
    with pytest.raises(ops.HmseError, match="inconsistent"):
        ops.regex_seams(_t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), _t(np.asarray(cuts, np.int64), dev), _t(np.asarray([0, 2, 0], np.int64), dev), good.rx)


# ---- 2. memory ---------------------------------------------------------------------------------------------------------------------------
MEMORY = [("zero", 0, False), ("ones", 0, False), ("random", 0, False), ("random", 1, False), ("random", 3, False), ("random", 13, False),
          ("random", 0, True)]


@pytest.mark.parametrize("pattern,misalign,distrust", MEMORY)
def test_entry_points_depend_on_their_arguments_only(dev, monkeypatch, pattern, misalign, distrust):
    """Both entry points (and hmse_find_place behind the scan) on poisoned memory — outputs, status words and counts included — with raw
    off its alignment, between guard bands."""
    import torch
    from hmse_amd import ops
    from hmse_amd.regex import Regex
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
    for pat in (b"ab+c", b"[ab]{3}d?", b"d[a-c]*d"):
        h = Regex(pat)
        rx = ops.Regex(ar.place(h.table.view(np.int16).copy()), ar.place(h.classmap.copy(), misalign=misalign), h.n_states, h.n_classes, h.reach)
        want_scan, want_seam = ref.split(corpus, ref.find(corpus, pat, h.reach), h.reach, cuts)
        want_raw, want_count = ref.scan_hits(raw, raw_off, pat, h.reach, mult.tolist())
        hits, n, count = ops.regex_scan(raw_d, ro, mult, rx)
        assert sorted(hits.tolist()) == want_raw and n == len(want_raw) and int(count[0]) == want_count == len(want_scan)
        assert int(ops.regex_scan(raw_d, ro, mult, rx, hits_cap=0)[2][0]) == want_count
        assert sorted(ops.regex_scan(raw_d, ro, None, rx, hits_cap=5)[0].tolist()) == want_raw
        sh, sn, sc = ops.regex_seams(raw_d, ro, cu, sl, rx)
        assert sorted(sh.tolist()) == [(o << 8) | (l - 1) for o, l in want_seam] and sn == len(want_seam) == int(sc[0])
        hs = ar.place(torch.sort(hits)[0])
        lo = torch.searchsorted(hs, ro << 8)
        chunk_out = ar.place(torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((lo[1:] - lo[:-1])[sl], 0)]))
        assert ops.find_place(hs, ro, cu, sl, chunk_out, len(want_scan)).tolist() == [(o << 8) | (l - 1) for o, l in want_scan]
    ar.check()


@pytest.mark.parametrize("misalign", [0, 3])
def test_nothing_behind_raw_bytes_is_read_as_data(dev, monkeypatch, misalign):
    """raw_bytes ends inside the buffer after "...ab", with "bbc" lying right behind it: the walk stops at raw_bytes."""
    from hmse_amd import ops
    from hmse_amd.regex import Regex
    ar = A.Arena(dev, "random", seed=23).install(monkeypatch)
    h = Regex(b"ab{1,3}c?")
    rx = ops.Regex(ar.place(h.table.view(np.int16).copy()), ar.place(h.classmap.copy()), h.n_states, h.n_classes, h.reach)
    for n in (T + 2, 3 * S + 2, 7, 13):
        body = np.full(n, ord("."), np.uint8)
        body[-2:] = np.frombuffer(b"ab", np.uint8)
        body[:5] = np.frombuffer(b"abbc.", np.uint8)
        raw, both = ar.place_with_tail(body, np.frombuffer(b"bbc" * 30, np.uint8).copy(), misalign=misalign)
        ro, cu, sl = (ar.place(np.array(v, np.int64)) for v in ([0, n], [0, n], [0]))
        hits, nh, _ = ops.regex_scan(raw, ro, None, rx)
        assert sorted(hits.tolist()) == [(0 << 8) | 3] and nh == 1                     # (n - 2 is no scan start: 2 < reach = 5)
        sh, sn, _ = ops.regex_seams(raw, ro, cu, sl, rx)
        assert sorted(sh.tolist()) == [((n - 2) << 8) | 1] and sn == 1                 # "ab", not "abbbc"
    ar.check()


# ---- 3. store level ----------------------------------------------------------------------------------------------------------------------
MARK = b"zq-marker"
STORE_PATTERNS = [(rb"hzms", False), (rb"\d{4}-\d\d-\d\d", False), (rb"\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}", False), (rb"[A-Za-z]+ing", False),
                  (rb"(error|warn|etr)[a-z ]*id=", True), (rb"[^\n]*" + MARK, False)]


def _planted(w):
    """The synthetic text with dates, addresses, log words and a marker written over it at seeded places."""
    w = w.copy()
    rng = np.random.default_rng(77)
    words = [b"2024-01-31", b"1999-12-3", b"192.168.0.1", b"10.0.0.256.7", b"ERROR code id=7", b"Warn  id=", b"warning", MARK, b"1.2.3", b"ringing"]
    for o in np.sort(rng.choice(w.size // 64 - 1, 1500, replace=False)) * 64:
        s = words[int(rng.integers(0, len(words)))]
        w[o: o + len(s)] = np.frombuffer(s, np.uint8)
    return w


def _store_input():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import variants_dataset
    from hmse_amd import corpus
    w = _planted(corpus.wiki_synth(2 * MIB, seed=42))
    return np.concatenate([w[: MIB + 300_000], w[200_000: 900_000],                   # a repeated 700 000-byte stretch: POINTER chunks
                           variants_dataset(w)[:600_000],                            # a near-duplicate family: DELTA records
                           np.full(200_000, ord("e"), np.uint8)])                    # many POINTERs to one record, every boundary a seam


def _ragged_seg_off(n, dev):
    import torch
    off = [0]
    for s in [MIB, 1, 2, 3, 70, MIB, 1, 70, 3, 2]:
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


@pytest.fixture(scope="module")
def oracle(stores, dev):
    """Per store pattern: the compiled Regex and the oracle's [(offset, length)] over the stores' bytes — computed once."""
    b = stores[1].tobytes()
    rxs = [_rx(dev, p, ic) for p, ic in STORE_PATTERNS]
    return rxs, [ref.find(b, r.pattern, r.reach, r.ignore_case) for r in rxs]


def _equals(found, want):
    counts = [len(w) for w in want]
    assert found.counts.tolist() == counts and found.ptr.tolist() == [0] + [int(v) for v in np.cumsum(counts)]
    assert found.offsets.tolist() == [o for w in want for o, _ in w] and found.lengths.tolist() == [l for w in want for _, l in w]


@pytest.mark.parametrize("name", ["plain", "ragged"])
def test_find_regex_equals_the_oracle(stores, oracle, dev, name):
    import torch
    from hmse_amd import KIND_DELTA, KIND_POINTER, find
    cfg, data, out = stores
    m, fd = out[name]
    kinds, lens = m.chunk_map["kind"], m.chunk_map["raw_length"]
    assert (kinds == KIND_POINTER).sum() > 50 and (kinds == KIND_DELTA).sum() > 5
    if name == "ragged":
        assert (lens < cfg.min_size).sum() >= 8 and {1, 2, 3, 70} <= set(lens.tolist())
    rxs, want = oracle
    assert all(len(w) > 20 for w in want)
    got = fd.find_regex(rxs)
    assert isinstance(got, find.RegexFound) and isinstance(got, find.Found) and got.lengths.dtype == torch.int64
    _equals(got, want)
    assert fd.count_regex(rxs).tolist() == [len(w) for w in want] and fd.count_regex(rxs[1]).tolist() == [len(want[1])]
    assert fd.find_regex(rxs[0]).offsets.tolist() == fd.find([STORE_PATTERNS[0][0]]).offsets.tolist()      # a pure literal: find's offsets
    # from a hit to its line, and grep -o's choice
    b = data.tobytes()
    lines = fd.grep_regex(rxs[1:3], before=1)
    sub = want[1:3]
    ptr = [0, len(sub[0]), len(sub[0]) + len(sub[1])]
    want_lines = lines_ref.lines(b, ([len(w) for w in sub], ptr, [o for w in sub for o, _ in w]), 0x0A, 1, 0)
    for f in ("ptr", "start", "end", "hits", "counts"):
        assert getattr(lines, f).tolist() == want_lines[f], f
    assert lines.flags.tolist() == want_lines["flags"]
    keep = find.nonoverlapping(got)
    k_off, k_len = keep.offsets.tolist(), keep.lengths.tolist()
    for j, w in enumerate(want):
        idx = ref.nonoverlapping([o for o, _ in w], [l for _, l in w])
        a, e = int(keep.ptr[j]), int(keep.ptr[j + 1])
        assert k_off[a:e] == [w[i][0] for i in idx] and k_len[a:e] == [w[i][1] for i in idx]


def test_find_regex_limits_and_edges(stores, oracle, dev):
    import torch
    from hmse_amd import find, manifest
    from hmse_amd.regex import Regex
    cfg, data, out = stores
    m, fd = out["plain"]
    rxs, want = oracle
    with pytest.raises(ValueError, match=r"counts per pattern: \[\d+, \d+\]"):
        fd.find_regex(rxs[:2], max_hits=10)
    n1 = len(want[1])
    assert fd.find_regex(rxs[1], max_hits=n1).offsets.numel() == n1
    z = fd.find_regex([])
    assert z.ptr.tolist() == [0] and z.offsets.numel() == 0 and z.lengths.numel() == 0 and fd.count_regex([]).numel() == 0
    assert z.offsets.dtype == torch.int64 and z.offsets.device.type == "cuda"
    with pytest.raises(ValueError):
        fd.find_regex(Regex(b"ab"))                                                    # compiled without a device
    with pytest.raises(ValueError):
        fd.find_regex([b"ab"])
    empty = find.StoreFinder(manifest.Store([]), dev)
    f = empty.find_regex(rxs[:2])
    assert f.counts.tolist() == [0, 0] and f.ptr.tolist() == [0, 0, 0] and f.offsets.numel() == 0 and empty.count_regex(rxs[0]).tolist() == [0]
    got = find.find_regex(m, rxs[2], dev)                                              # the one-off forms
    assert got.offsets.tolist() == [o for o, _ in want[2]]
    assert find.grep_regex(m, rxs[2], dev).counts.tolist() == fd.lines(got).counts.tolist()


def test_two_shard_store_gives_the_one_shard_results(stores, oracle, dev):
    import torch
    from hmse_amd import find, ingest, manifest
    cfg, data, out = stores
    half = MIB + 300_000 + 350_000                                                   # inside the repeated stretch: POINTERs across shards
    rs = ingest.ingest_shards_local([torch.from_numpy(p).to(dev) for p in (data[:half], data[half:])], cfg)
    st = manifest.Store.from_bytes(manifest.merge_manifests([manifest.build_manifest(r, i, 2) for i, r in enumerate(rs)]).to_bytes())
    _equals(find.StoreFinder(st, dev).find_regex(oracle[0]), oracle[1])


def test_smallest_chunk_sizes(dev):
    import torch
    from hmse_amd import IngestConfig, corpus, find, ingest, manifest
    cfg = IngestConfig(min_size=64, avg_size=256, max_size=1024, seg_size=1 << 16)
    w = _planted(corpus.wiki_synth(192 << 10, seed=7))
    data = np.concatenate([w, w[10_000: 10_000 + (64 << 10)]])
    res = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    fd = find.StoreFinder(manifest.Manifest.from_bytes(manifest.build_manifest(res).to_bytes()), dev)
    assert fd.cuts.numel() > 600
    word = re.search(rb"[a-z]{4}", data.tobytes()[5000:]).group()                      # a literal of this corpus
    rxs = [_rx(dev, p, ic) for p, ic in [(word, False)] + STORE_PATTERNS[1:]]
    want = [ref.find(data.tobytes(), r.pattern, r.reach, r.ignore_case) for r in rxs]
    assert all(want)
    _equals(fd.find_regex(rxs), want)
    assert fd.count_regex(rxs).tolist() == [len(w) for w in want]
