"""GPU: regular-expression search with assertions (hmse_amd.regex.Regex(assertions=True) / hmse_amd.find; hmse_regexa_scan /
hmse_regexa_seams of include/hmse_regexa.h, hits laid out by hmse_find_place) against the `re` oracle of tests/regexa_ref.py — per kernel on
synthetic tables, on poisoned / misaligned / guarded memory (tests/arena.py), and on stores built the way tests/test_gpu_regex.py builds
its own, only smaller: the oracle asks `re` about the WHOLE buffer for every length, so large buffers carry their interesting bytes in
filler the pattern cannot touch and the oracle is asked inside windows around them.  All results are compared bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import arena as A
import lines_ref
import regexa_ref as ref

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc", "regexa.hip")).read()
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
    return Regex(pattern, ic, dotall, device=dev, assertions=True)


def scan(dev, raw, raw_off, r, mult=None, hits_cap=None):
    import torch
    from hmse_amd import ops
    h, n, c = ops.regexa_scan(_t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), None if mult is None else _t(np.asarray(mult, np.int32), dev),
                              r.rx, hits_cap)
    assert h.dtype == torch.int64 and c.dtype == torch.int64 and c.numel() == 1
    return sorted(h.tolist()), n, int(c[0])


def check_scan(dev, raw, raw_off, r, mult=None, windows=None, elsewhere=False):
    """-> the hits as sorted (position, length) pairs, after comparing list, n_hits, count and the count-only mode with the oracle (asked
    inside `windows` of raw positions only: a hit anywhere else is a difference, unless `elsewhere` says that the caller holds the
    whole list against its construction)."""
    want, want_count = ref.scan_hits(raw, raw_off, r.pattern, r.reach, mult, r.ignore_case, r.dotall, windows)
    got, n, count = scan(dev, raw, raw_off, r, mult)
    if elsewhere:
        assert [h for h in got if any(lo <= h >> 8 < hi for lo, hi in windows)] == want and n == len(got) == count
    else:
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
    want_scan, want_seam = ref.split(ref.find(corpus, r.pattern, r.reach, r.ignore_case, r.dotall), r.reach, cuts)
    word = lambda pairs: [(o << 8) | (l - 1) for o, l in pairs]
    mult = torch.bincount(sl, minlength=len(raw_off) - 1).to(torch.int32)
    hits, n, count = ops.regexa_scan(raw_d, ro, mult, r.rx)
    hits = torch.sort(hits)[0]
    lo = torch.searchsorted(hits, ro << 8)
    chunk_out = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((lo[1:] - lo[:-1])[sl], 0)])
    placed = ops.find_place(hits, ro, cu, sl, chunk_out, int(chunk_out[-1]))
    assert placed.tolist() == word(want_scan) and int(count[0]) == len(want_scan)      # as laid out: ascending by corpus offset
    sh, sn, sc = ops.regexa_seams(raw_d, ro, cu, sl, r.rx)
    assert sorted(sh.tolist()) == word(want_seam) and sn == len(want_seam) and int(sc[0]) == sn
    assert ops.regexa_seams(raw_d, ro, cu, sl, r.rx, hits_cap=0)[1] == sn
    return want_scan, want_seam


# ---- 1. the scan, one record of 3T bytes ---------------------------------------------------------------------------------------------------
FLIP_AT = ([T, 2 * T, S, 16], [17, T + 17])                                            # (16 stands in front of 17: two passes)


@pytest.mark.parametrize("pat,yes,no", [(rb"^a", b"\n", b"."), (rb"\ba", b".", b"x"), (rb"\Ba", b"x", b".")])
def test_the_byte_in_front_decides_at_tile_strip_and_piece_boundaries(dev, pat, yes, no):
    """'a' at the first byte of a tile, a strip and a piece (and one behind): a hit iff the byte in front — the last byte of the tile,
    strip or piece before — has the right kind."""
    r = _rx(dev, pat)
    for places in FLIP_AT:
        windows = [(p - 3, p + 3) for p in places]
        for front, hit in ((yes, True), (no, False)):
            rec = np.full(3 * T, ord("-"), np.uint8)
            for p in places:
                rec[p], rec[p - 1] = ord("a"), front[0]
            got = check_scan(dev, rec.tobytes(), [0, 3 * T], r, windows=windows)
            assert got == ([(p, 1) for p in sorted(places)] if hit else []), (front, got)
    places = FLIP_AT[0][:3]
    rec = np.full(3 * T, ord("-"), np.uint8)                                           # both at once: each place on its own
    for i, p in enumerate(places):
        rec[p], rec[p - 1] = ord("a"), (yes if i % 2 == 0 else no)[0]
    got = check_scan(dev, rec.tobytes(), [0, 3 * T], r, windows=[(p - 3, p + 3) for p in places])
    assert got == sorted((p, 1) for i, p in enumerate(places) if i % 2 == 0)


@pytest.mark.parametrize("start", [T - 1, T - 256, T])
@pytest.mark.parametrize("pat,m,yes,no", [(rb"a{256}$", 256, b"\n", b"-"), (rb"a{256}\b", 256, b"-", b"x"), (rb"a{255}\B", 255, b"x", b"\n")])
def test_the_look_ahead_byte_of_a_longest_match_at_the_tile_edge(dev, start, pat, m, yes, no):
    """m bytes of 'a' behind '.' from `start`: the byte at start + m decides — for start = T - 1 and m = 256 the last staged byte."""
    r = _rx(dev, pat)
    assert r.reach == m
    for behind, hit in ((yes, True), (no, False)):
        rec = np.full(3 * T, ord("."), np.uint8)
        rec[start: start + m] = ord("a")
        rec[start + m] = behind[0]
        got = check_scan(dev, rec.tobytes(), [0, 3 * T], r, windows=[(start - 2, start + m + 2)])
        assert got == ([(start, m)] if hit else []), (behind, got)


def test_a_run_over_a_tile_edge_ends_at_a_word_boundary_or_nowhere(dev):
    """600 'q' over the tile edge, q+\\b: a start with 256 or fewer bytes of run left matches to the run's end; one with more sees 'q' behind
    every length it can reach and is no occurrence.  The oracle is asked at both ends of the run and around the change."""
    rec = np.full(3 * T, ord("."), np.uint8)
    a, e = T - 300, T + 300
    rec[a:e] = ord("q")
    got = check_scan(dev, rec.tobytes(), [0, 3 * T], _rx(dev, rb"q+\b"), windows=[(a - 2, a + 3), (e - 258, e - 253), (e - 3, e + 2)], elsewhere=True)
    assert got == [(o, e - o) for o in range(e - 256, e)]
    assert [g for g in got if g[0] in (e - 256, e - 1)] == [(e - 256, 256), (e - 1, 1)]


def test_every_position_of_a_tile_survives_and_a_tile_where_only_the_kind_filter_rejects(dev):
    n = 2 * T + 500
    raw = np.full(n, ord("a"), np.uint8)
    raw[::100] = ord("x")
    r = _rx(dev, rb"[^\n]*x\B")                                                         # every start survives its first byte, whatever stands in front
    xs = np.arange(0, n, 100)
    want = []                                                                          # by construction: the last x within 256 bytes (an 'a' follows it)
    for o in range(1, n - r.reach):
        x = xs[np.searchsorted(xs, o + 255, "right") - 1]
        want.append((o, int(x) - o + 1))
    got = check_scan(dev, raw.tobytes(), [0, n], r, windows=[(T - 4, T + 4), (1, 4), (2 * T - 2, 2 * T + 2)], elsewhere=True)
    assert got == want and len(got) > T
    raw[:] = ord("a")                                                                  # 'a' survives the first step of three start states, but a word byte stands in front
    for p in (S - 1, T - 1, T + 15, 2 * T - 1):
        raw[p] = ord(".")
    got = check_scan(dev, raw.tobytes(), [0, n], _rx(dev, rb"\ba"), windows=[(p - 2, p + 4) for p in (S - 1, T - 1, T + 15, 2 * T - 1)])
    assert got == [(S, 1), (T, 1), (T + 16, 1), (2 * T, 1)]


def test_more_tiles_than_the_grid(dev):
    n = (GRID + 3) * T + 123
    rng = np.random.default_rng(4)
    raw = np.full(n, ord("."), np.uint8)
    at = np.sort(rng.choice(n // 8 - 2, 3000, replace=False) + 1) * 8                  # apart: no two overlap
    for i, ch in enumerate(b"Qz7"):
        raw[at + i] = ch
    raw[at[::2] - 1] = 0x0A                                                            # every second one stands at a line start
    raw[at[::4] + 3] = ord("_")                                                        # and every second of those runs into a word byte
    r = _rx(dev, rb"^Qz\d\b")
    got, nh, count = scan(dev, raw.tobytes(), [0, n], r)
    want = [(int(o) << 8) | 2 for i, o in enumerate(at) if i % 4 == 2 and n - int(o) > r.reach]
    assert got == want and nh == len(want) and count == len(want) and len({o // T for o in at.tolist()}) > GRID
    buf, orc = raw.tobytes(), ref.Oracle(r.pattern)
    for i in (0, 1, 2, 3, 2998, 2999):                                                 # the construction itself, asked of `re`
        assert orc.length_at(buf, int(at[i]), r.reach) == (3 if i % 4 == 2 else 0)


def test_mult_count_only_and_a_list_that_runs_out(dev):
    import torch
    from hmse_amd import _lib
    r = _rx(dev, rb"\b[ab]c\b")
    raw = b" ac bc" * 50 + b" ac" * 10 + b"zz" * 10
    raw_off, mult = [0, 300, 330, 350], [3, 0, 1000000]
    want, want_count = ref.scan_hits(raw, raw_off, r.pattern, r.reach, mult)
    assert len(want) == 108 and want_count == 297                                      # (the records' last match has no look-ahead byte inside)
    assert scan(dev, raw, raw_off, r, mult) == (want, 108, 297)
    assert scan(dev, raw, raw_off, r, None) == (want, 108, 108)
    assert scan(dev, raw, raw_off, r, mult, hits_cap=0) == ([], 108, 297)
    assert scan(dev, raw, raw_off, r, mult, hits_cap=7) == (want, 108, 297)            # ran out: ops repeats once with the exact capacity
    raw_d, ro, mu = _t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), _t(np.asarray(mult, np.int32), dev)
    hits = torch.full((64,), -7, dtype=torch.int64, device=dev)
    nh, cnt, st = (torch.full((1,), -7, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.int32))
    hdr = r.rx.header()
    rc = _lib.hip_lib().hmse_regexa_scan(raw_d.data_ptr(), len(raw), ro.data_ptr(), 3, mu.data_ptr(), C.byref(hdr), hits.data_ptr(), 7,
                                         nh.data_ptr(), cnt.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and int(st) == 1 and int(nh) == 108 and int(cnt) == 297 and (hits[7:] == -7).all() and set(hits[:7].tolist()) <= set(want)


# ---- 2. the scan rule ------------------------------------------------------------------------------------------------------------------------
def test_scan_starts_obey_the_rule_and_nothing_depends_on_a_neighbouring_record(dev):
    for pat in (rb"^ab", rb"b\b", rb"\bab{1,3}\b", rb"[ab]{4}$", rb"\Bb+"):
        r = _rx(dev, pat)
        R = r.reach
        body = b"ab abbb\nab ab" * 60
        recs = [body[:1], body[:R], body[:R + 1], body[:R + 2], body[:2 * R + 3], body[:600], b"ab", b"\nab\n"]
        relative = []
        for junk in (b"\n", b"ab", b" "):                                              # the same records between different neighbours
            raw, raw_off = junk * 2, [len(junk) * 2]
            for rec in recs:
                raw += rec
                raw_off.append(len(raw))
                raw += junk * 3
                raw_off.append(len(raw))
            mult = [1, 0] * len(recs)
            got = check_scan(dev, raw, raw_off, r, mult)
            rel = []
            for p, l in got:
                k = max(i for i, x in enumerate(raw_off) if x <= p)
                assert p > raw_off[k] and raw_off[k + 1] - p > R and p + l < raw_off[k + 1]
                if k % 2 == 0:
                    rel.append((k, p - raw_off[k], l))
            relative.append(rel)
        assert relative[0] == relative[1] == relative[2] and (len(relative[0]) > 0 or R == 256)


# ---- 3. the seams ----------------------------------------------------------------------------------------------------------------------------
SEAM_CASES = [rb"^ab", rb"b$", rb"\Aab", rb"b\Z", rb"\bab\b", rb"^[ab]{2,5}$", rb"\Bb+c?", rb"(^|c)a\b", rb"^[^\n]*c$"]


@pytest.mark.parametrize("pat", SEAM_CASES)
def test_seams_over_tiny_and_empty_chunks(dev, pat):
    r = _rx(dev, pat)
    R = r.reach
    rng = np.random.default_rng(len(pat))
    corpus = b"ab " + bytes(np.frombuffer(b"abc \n\nab", np.uint8)[rng.integers(0, 8, 700)]) + b"\nab cab\nabbbc" * 12 + b"\nab"
    lens = [0, 1, 0, 2, 1, 1, 0, 0]                                                    # "ab" + ... : ^ and \b at 0 through an empty first chunk
    for _ in range(3):
        lens += [min(R, 60), 0, 1, min(R + 1, 61), 2, 0, 0, min(R + 2, 62)]
    while sum(lens) < len(corpus):
        lens.append(int(rng.choice([0, 1, 2, 1, 2, 3, 7, 40, 300])))
    lens[-1] -= sum(lens) - len(corpus)
    cuts = [0] + [int(v) for v in np.cumsum(lens)] + [len(corpus)] * 2                # the last chunks are empty: N is the edge
    q = corpus.index(b"\nab", 300) + 1                                                # empty chunks between a newline and the chunk in front of which ^ is asked
    cuts = sorted(cuts + [q] * 4)
    want_scan, want_seam = pipeline(dev, corpus, cuts, r)
    assert want_seam
    found = dict(want_scan + want_seam)
    if pat in (rb"^ab", rb"\Aab", rb"\bab\b"):
        assert found.get(0) == 2                                                       # the edge in front of the corpus
    if pat in (rb"b$", rb"b\Z", rb"\bab\b"):
        assert (len(corpus) - 1 in found) or (len(corpus) - 2 in found)               # the edge behind it
    if pat == rb"\Aab":
        assert list(found) == [0]
    if pat == rb"b\Z":
        assert list(found) == [len(corpus) - 1]


def test_a_match_running_over_five_chunks_whose_look_ahead_lies_in_a_sixth(dev):
    rng = np.random.default_rng(11)
    block = bytes(rng.integers(97, 123, 230, dtype=np.uint8))
    corpus = b"- " + block + b" " + block + b"_" + block[:100] + b"\n" + block[:40]
    cuts = [0, 1, 2, 50, 51, 51, 120, 200, 232, 233, 300, 463, 464, 500, 564, 565, 605]
    assert cuts[-1] == len(corpus) and cuts[8] == 2 + 230 and corpus[232:233] == b" "
    r = _rx(dev, rb"\b[a-z]{200,256}\b")
    want_scan, want_seam = pipeline(dev, corpus, cuts, r)
    assert (2, 230) in want_seam and not [w for w in want_scan + want_seam if w[0] in range(233, 464)]      # the second block runs into '_'
    pipeline(dev, corpus, cuts, _rx(dev, rb"[a-z]+$"))
    pipeline(dev, corpus, cuts, _rx(dev, rb"^[a-z]{1,40}\Z|\A- "))


PIPE_PATTERNS = [rb"^a", rb"a$", rb"\ba+\b", rb"\Ba", rb"(^|b)a", rb"a($|b)", rb"^.*$", rb"(a|^)(b|$)", rb"\w+$", rb"^\W", rb".\b.", rb"ab"]


@pytest.mark.parametrize("pat", PIPE_PATTERNS)
def test_scan_place_and_seams_over_random_chunk_maps_with_duplicates(dev, pat):
    r = _rx(dev, pat)
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        blocks = [bytes(np.frombuffer(b"aab- \n_", np.uint8)[rng.integers(0, 7, int(n))]) for n in (1, 2, 3, 9, 30, 70)]
        order = rng.integers(0, len(blocks), 40)
        corpus, cuts = b"", [0]
        for i in order:
            corpus += blocks[i]
            cuts.append(len(corpus))
            if rng.integers(0, 5) == 0:
                cuts.append(len(corpus))                                               # an empty chunk
        _, _, slot = tables(corpus, cuts)
        assert len(set(slot)) < len(slot) - 10                                         # duplicates
        pipeline(dev, corpus, cuts, r)


def test_one_record_in_four_contexts(dev):
    """The record `cat` after a newline, after `con`, in front of `s` and in front of a newline: the answer differs from place to place."""
    corpus = b"x\ncat concat cats\ncat\n cat"
    cuts = [0, 2, 5, 9, 12, 13, 16, 18, 21, 23, 26]
    assert [corpus[a:b] for a, b in zip(cuts, cuts[1:])].count(b"cat") == 5
    raw, raw_off, slot = tables(corpus, cuts)
    assert raw.count(b"cat") == 1
    for pat in (rb"^cat", rb"\bcat\b", rb"cat$", rb"\Bcat", rb"cat\Z"):
        r = _rx(dev, pat)
        want_scan, want_seam = pipeline(dev, corpus, cuts, r)
        assert not want_scan and [o for o, _ in want_seam] == [m.start() for m in re.finditer(pat, corpus, re.M)]
    assert [m.start() for m in re.finditer(rb"^cat", corpus, re.M)] == [2, 18] and [m.start() for m in re.finditer(rb"cat$", corpus, re.M)] == [18, 23]


# ---- 4. memory -------------------------------------------------------------------------------------------------------------------------------
def test_empty_tables(dev):
    import torch
    from hmse_amd import ops
    z = lambda n, dt=torch.int64: torch.zeros(n, dtype=dt, device=dev)
    r = _rx(dev, rb"^ab")
    h, n, c = ops.regexa_seams(z(0, torch.uint8), z(1), z(1), z(0), r.rx)
    assert h.numel() == 0 and n == 0 and c.tolist() == [0]
    h, n, c = ops.regexa_scan(z(0, torch.uint8), z(1), None, r.rx)
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
            rc = lib.hmse_regexa_scan(raw_d.data_ptr(), len(raw), ro.data_ptr(), len(raw_off) - 1, None, C.byref(hdr), hits.data_ptr(), 64,
                                      nh.data_ptr(), cnt.data_ptr(), st.data_ptr(), stream)
        else:
            rc = lib.hmse_regexa_seams(raw_d.data_ptr(), len(raw), ro.data_ptr(), len(raw_off) - 1, cu.data_ptr(), sl.data_ptr(), len(slot),
                                       C.byref(hdr), hits.data_ptr(), 64, nh.data_ptr(), cnt.data_ptr(), st.data_ptr(), stream)
        torch.cuda.synchronize()
        out.append((rc, int(st), int(nh), int(cnt), bool((hits == -7).all())))
    return out


def test_a_damaged_automaton_sets_bit_2_and_inconsistent_tables_bit_1(dev):
    from hmse_amd import ops
    from hmse_amd.regex import Regex
    raw, raw_off, cuts, slot = b"ab cdab\nab cdab\n", [0, 8, 16], [0, 8, 16, 24], [0, 1, 0]
    host = Regex(rb"\bab+c?$|^ab", assertions=True)
    good = _rx(dev, host.pattern)
    nc, ns = host.n_classes, host.n_states
    assert [c[:2] for c in _raw_calls(dev, raw, raw_off, cuts, slot, good.rx.header())] == [(0, 0), (0, 0)]
    damaged = []
    t = host.table.copy(); t[nc + 1] = ns; damaged.append((t, host.classmap))                                   # an entry >= n_states
    t = host.table.copy(); t[-2] = 0x8000 | (ns + 5); damaged.append((t, host.classmap))
    t = host.table.copy(); t[0] = 1; damaged.append((t, host.classmap))                                         # a non-zero dead row
    t = host.table.copy(); t[nc - 1] = 0x8000; damaged.append((t, host.classmap))
    m = host.classmap.copy(); m[200] = nc - 1; damaged.append((host.table, m))                                  # a byte in the EDGE class
    m = host.classmap.copy(); m[200] = nc; damaged.append((host.table, m))                                      # and beyond
    m = host.classmap.copy(); m[ord("a")] = m[0x0A]; damaged.append((host.table, m))                            # a class that mixes kinds
    m = host.classmap.copy(); m[ord("-")] = m[ord("z")]; damaged.append((host.table, m))
    t = host.table.copy(); t[2 * nc + nc - 1] |= 1; damaged.append((t, host.classmap))                          # the EDGE column leads somewhere
    for t, m in damaged:
        bad = ops.RegexA(_t(t.view(np.int16), dev), _t(m, dev), ns, nc, host.reach, host.start)
        assert _raw_calls(dev, raw, raw_off, cuts, slot, bad.header()) == [(0, 4, 0, 0, True)] * 2
        with pytest.raises(ops.HmseError, match="bad automaton"):
            ops.regexa_scan(_t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), None, bad)
    for ro, cu, sl in (([0, 8, 4], cuts, slot), ([0, 8, 17], cuts, slot), (raw_off, [0, 8, 7, 15], slot), (raw_off, cuts, [0, 2, 0]),
                       (raw_off, [0, 8, 16, 25], slot)):
        res = _raw_calls(dev, raw, ro, cu, sl, good.rx.header())
        assert res[1] == (0, 2, 0, 0, True), (ro, cu, sl)
        if ro != raw_off:
            assert res[0] == (0, 2, 0, 0, True)
    with pytest.raises(ops.HmseError, match="inconsistent"):
        ops.regexa_seams(_t(raw, dev), _t(np.asarray(raw_off, np.int64), dev), _t(np.asarray(cuts, np.int64), dev), _t(np.asarray([0, 2, 0], np.int64), dev), good.rx)


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
    letters = np.frombuffer(b"ab \n", np.uint8)
    block = bytes(letters[rng.integers(0, 4, 300)])
    corpus = block + b"ab\n" + block + bytes(letters[rng.integers(0, 4, 400)]) + block[:150]
    cuts = [0, 150, 300, 301, 303, 453, 603, 1003, 1153]
    assert cuts[-1] == len(corpus)
    raw, raw_off, slot = tables(corpus, cuts)
    ar = A.Arena(dev, pattern, seed=17).install(monkeypatch, distrust_zeros=distrust, byte_misalign=misalign)
    i64 = lambda a: ar.place(np.asarray(a, np.int64))
    raw_d = ar.place(np.frombuffer(raw, np.uint8).copy(), misalign=misalign)
    ro, cu, sl = i64(raw_off), i64(cuts), i64(slot)
    mult = ar.place(np.bincount(slot, minlength=len(raw_off) - 1).astype(np.int32))
    for pat in (rb"^ab", rb"\b[ab]{3}\b", rb"b[ab ]*$"):
        h = Regex(pat, assertions=True)
        rx = ops.RegexA(ar.place(h.table.view(np.int16).copy()), ar.place(h.classmap.copy(), misalign=misalign), h.n_states, h.n_classes, h.reach, h.start)
        want_scan, want_seam = ref.split(ref.find(corpus, pat, h.reach), h.reach, cuts)
        want_raw, want_count = ref.scan_hits(raw, raw_off, pat, h.reach, mult.tolist())
        hits, n, count = ops.regexa_scan(raw_d, ro, mult, rx)
        assert sorted(hits.tolist()) == want_raw and n == len(want_raw) and int(count[0]) == want_count == len(want_scan)
        assert int(ops.regexa_scan(raw_d, ro, mult, rx, hits_cap=0)[2][0]) == want_count
        assert sorted(ops.regexa_scan(raw_d, ro, None, rx, hits_cap=5)[0].tolist()) == want_raw
        sh, sn, sc = ops.regexa_seams(raw_d, ro, cu, sl, rx)
        assert sorted(sh.tolist()) == [(o << 8) | (l - 1) for o, l in want_seam] and sn == len(want_seam) == int(sc[0])
        hs = ar.place(torch.sort(hits)[0])
        lo = torch.searchsorted(hs, ro << 8)
        chunk_out = ar.place(torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((lo[1:] - lo[:-1])[sl], 0)]))
        assert ops.find_place(hs, ro, cu, sl, chunk_out, len(want_scan)).tolist() == [(o << 8) | (l - 1) for o, l in want_scan]
    ar.check()


@pytest.mark.parametrize("misalign", [0, 3])
def test_nothing_behind_raw_bytes_is_read_as_data(dev, monkeypatch, misalign):
    """raw_bytes ends inside the buffer after "... ab", with "bbc" lying right behind it: the seam walk takes the EDGE at N, so `ab\\b` and
    `ab$` hold there; a kernel that read on would see "abbbc"."""
    from hmse_amd import ops
    from hmse_amd.regex import Regex
    ar = A.Arena(dev, "random", seed=23).install(monkeypatch)
    h = Regex(rb"ab{1,3}c?\b", assertions=True)
    e = Regex(rb"ab$", assertions=True)
    mk = lambda x: ops.RegexA(ar.place(x.table.view(np.int16).copy()), ar.place(x.classmap.copy()), x.n_states, x.n_classes, x.reach, x.start)
    rx, ex = mk(h), mk(e)
    for n in (T + 2, 3 * S + 2, 9, 13):
        body = np.full(n, ord("."), np.uint8)
        body[-2:] = np.frombuffer(b"ab", np.uint8)
        body[1:6] = np.frombuffer(b"abbc.", np.uint8)
        raw, both = ar.place_with_tail(body, np.frombuffer(b"bbc" * 30, np.uint8).copy(), misalign=misalign)
        ro, cu, sl = (ar.place(np.array(v, np.int64)) for v in ([0, n], [0, n], [0]))
        hits, nh, _ = ops.regexa_scan(raw, ro, None, rx)
        want_scan = [(1 << 8) | 3] if n - 1 > h.reach else []                          # (n - 2 is no scan start)
        assert sorted(hits.tolist()) == want_scan and nh == len(want_scan)
        sh, sn, _ = ops.regexa_seams(raw, ro, cu, sl, rx)
        assert sorted(sh.tolist()) == sorted(([] if want_scan else [(1 << 8) | 3]) + [((n - 2) << 8) | 1]) and sn == len(sh)      # "ab", not "abbbc"
        sh, sn, _ = ops.regexa_seams(raw, ro, cu, sl, ex)
        assert sh.tolist() == [((n - 2) << 8) | 1]
    ar.check()


# ---- 5. store level ----------------------------------------------------------------------------------------------------------------------
STORE_PATTERNS = [(rb"^ERROR", False), (rb"\b\d{4}-\d\d-\d\d\b", False), (rb"\bwarn(ing)?\b", True), (rb"id=\d$", False), (rb"\Bing\b", False)]
PLAIN_PATTERNS = [(rb"\d{4}-\d\d-\d\d", False), (rb"(error|warn)[a-z ]{0,6}id=", True), (rb"[A-Za-z]{2,9}ing", False)]


def _planted(w):
    """The synthetic text with log lines, dates and words written over it at seeded places, some at line starts and ends."""
    w = w.copy()
    rng = np.random.default_rng(77)
    words = [b"\nERROR code id=7\n", b" ERROR id=12 ", b"\nWarn  id=3 x", b" warning ", b"xwarningx", b" 2024-01-31 ", b"12024-01-312", b" 1999-12-31\n", b" ringing ", b" ing ",
             b"ERROR\n", b" warn\n"]
    for o in np.sort(rng.choice(w.size // 48 - 1, 900, replace=False)) * 48:
        s = words[int(rng.integers(0, len(words)))]
        w[o: o + len(s)] = np.frombuffer(s, np.uint8)
    return w


def _store_input():
    from hmse_amd import corpus
    w = _planted(corpus.wiki_synth(64 << 10, seed=42))
    near = w[8_000: 24_000].copy()                                                     # a near-duplicate stretch: DELTA records
    rng = np.random.default_rng(5)
    idx = rng.integers(0, near.size, near.size // 300)
    near[idx] = rng.integers(97, 123, idx.size, dtype=np.uint8)
    return np.concatenate([w, w[20_000: 36_000], near, np.full(4_000, ord("e"), np.uint8), np.frombuffer(b"\nERROR", np.uint8)])


@pytest.fixture(scope="module")
def stores(dev):
    import torch
    from hmse_amd import IngestConfig, find, ingest, manifest
    cfg = IngestConfig(min_size=64, avg_size=256, max_size=1024, seg_size=1 << 16)
    data = _store_input()
    d = torch.from_numpy(data).to(dev)
    off = [0]
    for s in [1 << 16, 1, 2, 3, 70, 1 << 15, 1, 70, 3, 2]:                              # ragged segments: tiny chunks
        off.append(off[-1] + s)
    while off[-1] < data.size:
        off.append(min(off[-1] + (1 << 16), data.size))
    out = {}
    for name, seg_off in (("plain", None), ("ragged", torch.tensor(off, dtype=torch.int64, device=dev))):
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
    from hmse_amd.regex import Regex
    cfg, data, out = stores
    m, fd = out[name]
    kinds, lens = m.chunk_map["kind"], m.chunk_map["raw_length"]
    assert (kinds == KIND_POINTER).sum() > 20 and (kinds == KIND_DELTA).sum() > 0
    if name == "ragged":
        assert {1, 2, 3, 70} <= set(lens.tolist())
    rxs, want = oracle
    assert all(len(w) > 20 for w in want)
    got = fd.find_regex(rxs)
    assert isinstance(got, find.RegexFound) and got.lengths.dtype == torch.int64
    _equals(got, want)
    assert fd.count_regex(rxs).tolist() == [len(w) for w in want] and fd.count_regex(rxs[1]).tolist() == [len(want[1])]
    assert want[0][-1] == (data.size - 5, 5) and want[0][0][0] > 0                     # ^ERROR at the corpus's very end: $ and the edge
    # grep: the lines `re` finds
    b = data.tobytes()
    lines = fd.grep_regex(rxs[0])
    at = [mm.start() for mm in re.finditer(rb"^ERROR", b, re.M)]
    want_lines = lines_ref.lines(b, ([len(at)], [0, len(at)], at), 0x0A, 0, 0)
    for f in ("ptr", "start", "end", "hits", "counts"):
        assert getattr(lines, f).tolist() == want_lines[f], f
    assert lines.start.tolist() == at and len(at) > 20                                 # every such line starts with its match
    keep = find.nonoverlapping(got)
    assert keep.counts.tolist() == got.counts.tolist()                                 # (none of these patterns overlaps itself)
    # assertion-free patterns: the asserting path returns exactly what the plain path returns
    for p, ic in PLAIN_PATTERNS:
        plain, asserting = fd.find_regex(Regex(p, ic, device=dev)), fd.find_regex(_rx(dev, p, ic))
        assert plain.offsets.numel() > 20
        assert asserting.offsets.tolist() == plain.offsets.tolist() and asserting.lengths.tolist() == plain.lengths.tolist()
        assert fd.count_regex(_rx(dev, p, ic)).tolist() == plain.counts.tolist()


def test_two_shard_store_and_the_one_off_forms(stores, oracle, dev):
    import torch
    from hmse_amd import find, ingest, manifest
    cfg, data, out = stores
    rxs, want = oracle
    half = (64 << 10) + 8_000                                                          # inside the repeated stretch: POINTERs across shards
    rs = ingest.ingest_shards_local([torch.from_numpy(p).to(dev) for p in (data[:half], data[half:])], cfg)
    st = manifest.Store.from_bytes(manifest.merge_manifests([manifest.build_manifest(r, i, 2) for i, r in enumerate(rs)]).to_bytes())
    _equals(find.StoreFinder(st, dev).find_regex(rxs), want)
    m, fd = out["plain"]
    assert find.find_regex(m, rxs[2], dev).offsets.tolist() == [o for o, _ in want[2]]
    assert find.grep_regex(m, rxs[0], dev).counts.tolist() == fd.grep_regex(rxs[0]).counts.tolist()
    empty = find.StoreFinder(manifest.Store([]), dev)
    f = empty.find_regex(rxs[:2])
    assert f.counts.tolist() == [0, 0] and f.offsets.numel() == 0 and empty.count_regex(rxs[0]).tolist() == [0]
    with pytest.raises(ValueError):
        from hmse_amd.regex import Regex
        fd.find_regex(Regex(rb"^ab", assertions=True))                                 # compiled without a device
