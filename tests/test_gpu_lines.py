"""GPU: lines of a hit (hmse_amd.find lines / text / grep; hmse_lines_extent / hmse_lines_gather) against the plain-Python reference of
tests/lines_ref.py — the two kernels on synthetic chunk maps (every offset of a small corpus under five chunkings, the edges of a trip
and of a lane, reach, deduplicated records, bad input), on poisoned / misaligned / guarded memory (tests/arena.py), and on stores with
POINTER and DELTA records.  All results are compared bit for bit.  The shapes are the smallest at which the kernels can go wrong."""
import os
import re

import numpy as np
import pytest

import arena as A_
import find_ref
import lines_ref as ref
from test_sync_host import SEG, corpora

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc", "lines.hip")).read()
T = int(re.search(r"constexpr uint32_t LINES_TRIP = (\d+);", _SRC).group(1))             # bytes one trip looks at
NL = 0x0A
BAD = ref.BAD


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    import torch
    a = np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)


def _tables(dev, corpus, cuts, place=None):
    place = place or (lambda x, **kw: _t(x, dev))
    raw, raw_off, slot = ref.tables(corpus, cuts)
    i64 = lambda v: np.asarray(v, np.int64).reshape(-1)
    return place(np.frombuffer(raw, np.uint8).copy(), side="raw"), place(i64(raw_off)), place(i64(cuts)), place(i64(slot))


def check_extent(dev, corpus, cuts, pos, d=NL, b=0, a=0, R=1 << 16, tabs=None, place=None):
    """ops.lines_extent on host inputs, asserted equal to the reference -> (list of (start, end, flags), status)."""
    import torch
    from hmse_amd import ops
    tabs = tabs or _tables(dev, corpus, cuts, place)
    p = (place or (lambda x, **kw: _t(x, dev)))(np.asarray(pos, np.int64).reshape(-1))
    start, end, flags, status = ops.lines_extent(*tabs, p, d, b, a, R)
    assert start.dtype == torch.int64 and end.dtype == torch.int64 and flags.dtype == torch.uint8
    assert start.numel() == end.numel() == flags.numel() == len(pos)
    got = list(zip(start.tolist(), end.tolist(), flags.tolist()))
    want = [ref.extent(corpus, int(o), d, b, a, R) for o in pos]
    assert got == want, next((o, g, w) for o, g, w in zip(pos, got, want) if g != w)
    assert status == (1 if any(w[2] == BAD for w in want) else 0)
    return got, status


def _text(n, seed, every=20, d=NL):
    rng = np.random.default_rng(seed)
    c = rng.integers(97, 123, n, dtype=np.uint8)
    c[rng.random(n) < 1.0 / every] = d
    return c.tobytes()


def _chunkings(corpus, d=NL):
    n = len(corpus)
    rng = np.random.default_rng(5)
    def walk(draw):
        cuts = [0]
        while cuts[-1] < n:
            cuts.append(min(cuts[-1] + int(draw()), n))
        return cuts
    at = [i for i in range(n) if corpus[i] == d]
    return {"one": [0, n], "tiny": walk(lambda: rng.integers(0, 3)) + [n, n], "ragged": walk(lambda: rng.integers(1, 301)),
            "at-delimiters": sorted({0, n, *at}), "behind-delimiters": sorted({0, n, *(i + 1 for i in at)})}


# ---- 1. every offset ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "tiny", "ragged", "at-delimiters", "behind-delimiters"])
def test_every_offset_of_a_small_corpus(dev, name):
    corpus = _text(3 * T + 37, seed=1)
    cuts = _chunkings(corpus)[name]
    assert cuts[0] == 0 and cuts[-1] == len(corpus) and (name != "tiny" or {0, 1, 2} >= set(np.diff(cuts).tolist()))
    tabs = _tables(dev, corpus, cuts)
    for b, a in ((0, 0), (1, 0), (0, 1), (3, 2)):
        got, status = check_extent(dev, corpus, cuts, list(range(len(corpus))), NL, b, a, tabs=tabs)
        assert status == 0 and not any(f for _, _, f in got)
        assert all((s, e) == ref.split_extent(corpus, o, NL, b, a) for o, (s, e, _) in enumerate(got))


# ---- 2. trip and lane edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", ["one", "ragged"])
def test_trip_and_lane_edges(dev, chunks):
    n, o = 12 * T, 6 * T
    cuts = [0, n] if chunks == "one" else sorted({0, n, o, o - 1, o + 1, o - T, o + T, *np.random.default_rng(3).integers(1, n, 30).tolist()})
    def corpus_with(at):
        c = bytearray(b"." * n)
        for p in at:
            c[p] = NL
        return bytes(c)
    # the closing and the opening delimiter at distance T - 1, T, T + 1; in lane 0 and lane 63 of the first trip on either side
    for dist in (0, 1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        corpus = corpus_with([o + dist] + ([o - dist] if dist else []))
        got, _ = check_extent(dev, corpus, cuts, [o, o + 1, o - 1])
        assert got[0] == ((o - dist + 1) if dist else 0, o + dist, 0)
    # b = a = 3 with exactly one delimiter per trip: the count carries across trips
    one_per_trip = [o + k * T + T // 2 for k in range(5)] + [o - 1 - k * T - T // 2 for k in range(5)]
    got, _ = check_extent(dev, corpus_with(one_per_trip), cuts, [o], NL, 3, 3)
    assert got == [(o - 1 - 3 * T - T // 2 + 1, o + 3 * T + T // 2, 0)]
    # b = a = 3 with all four delimiters in one trip: the rank select picks the fourth, not the first
    fwd, back = [o + 3, o + 10, o + 11, o + 40, o + 41, o + 63], [o - 2, o - 3, o - 30, o - 60, o - 61, o - 64]
    corpus = corpus_with(fwd + back)
    got, _ = check_extent(dev, corpus, cuts, [o], NL, 3, 3)
    assert got == [(o - 60 + 1, o + 40, 0)]
    for b, a in ((0, 0), (1, 1), (2, 2), (4, 4), (5, 5), (6, 6)):
        check_extent(dev, corpus, cuts, [o, o - 1, o + 1, o + 3, o - 2], NL, b, a)


# ---- 3. reach ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [0x00, 0x0A, 0xFF])
def test_reach_cuts_and_the_corpus_edges_do_not(dev, d):
    n, o = 8 * T, 4 * T
    cuts = sorted({0, n, o, *np.random.default_rng(d).integers(1, n, 20).tolist()})
    fill = 0x41 if d != 0x41 else 0x42
    for R in (1, 2, T, T + 1):
        for dist in (R - 1, R, R + 1):
            c = bytearray([fill]) * n
            c[o + dist] = d                                # the closing delimiter is the (dist + 1)-th byte looked at
            if dist:
                c[o - dist] = d
            got, _ = check_extent(dev, bytes(c), cuts, [o], d, 0, 0, R)
            s, e, f = got[0]
            assert bool(f & ref.END_CUT) == (dist >= R) and e == min(o + dist, o + R)
            assert bool(f & ref.START_CUT) == (dist > R or dist == 0) and s == (o - dist + 1 if 0 < dist <= R else o - R)
        plain = bytes([fill]) * n
        got, _ = check_extent(dev, plain, cuts, [0, 1, R - 1, R, R + 1, n - 1, n - 2, n - R, n - R - 1, n - R + 1 if R > 1 else n - 1], d, 2, 2, R)
        assert got[0] == (0, min(R, n), ref.END_CUT) and got[5] == (n - 1 - R, n, ref.START_CUT)       # the corpus's edge is no cut
    plain = bytes([fill]) * n
    got, _ = check_extent(dev, plain, cuts, [0, o, n - 1], d, 1, 1)                                 # no delimiter at all
    assert got == [(0, n, 0)] * 3
    only = bytes([d]) * (2 * T + 3)                                                                 # delimiters only
    for b, a in ((0, 0), (3, 2), (T, T + 1)):
        check_extent(dev, only, [0, 1, 3, T, 2 * T + 3], list(range(len(only))), d, b, a)
        check_extent(dev, only, [0, 1, 3, T, 2 * T + 3], list(range(len(only))), d, b, a, R=2)


# ---- 4. deduplicated records -------------------------------------------------------------------------------------------------------------
def test_one_record_at_three_places_gives_three_extents(dev):
    r = b"rrrr"
    chunks = [b"1\nAA", r, b"BB\n2\nC", r, b"DDD\n3\n", r, b"E"]
    corpus = b"".join(chunks)
    cuts = [0] + np.cumsum([len(c) for c in chunks]).tolist()
    raw, raw_off, slot = ref.tables(corpus, cuts)
    assert slot[1] == slot[3] == slot[5] and len(raw_off) - 1 == 5                          # one record, mapped by three chunks
    pos = [cuts[k] + 2 for k in (1, 3, 5)]                                                  # the same in-record position
    got, _ = check_extent(dev, corpus, cuts, pos)
    assert [corpus[s:e] for s, e, _ in got] == [b"AArrrrBB", b"CrrrrDDD", b"rrrrE"]
    got, _ = check_extent(dev, corpus, cuts, pos, NL, 1, 1)
    assert [corpus[s:e] for s, e, _ in got] == [b"1\nAArrrrBB\n2", b"2\nCrrrrDDD\n3", b"3\nrrrrE"]
    check_extent(dev, corpus, cuts, list(range(len(corpus))), NL, 1, 0, R=6)


# ---- 5. bad input ------------------------------------------------------------------------------------------------------------------------
def _raw_extent(dev, raw, raw_off, cuts, slot, pos, n=None, n_chunks=None, sentinel=0x5A):
    """hmse_lines_extent through ctypes on outputs and a status word that start as `sentinel` -> (start, end, flags, status) lists."""
    import torch
    from hmse_amd import _lib
    i64 = lambda v: _t(np.asarray(v, np.int64).reshape(-1), dev)
    raw_d, ro, cu, sl, p = _t(raw, dev), i64(raw_off), i64(cuts), i64(slot), i64(pos)
    n = len(pos) if n is None else n
    m = max(len(pos), 1)
    start, end = torch.full((m,), -7, dtype=torch.int64, device=dev), torch.full((m,), -7, dtype=torch.int64, device=dev)
    flags, status = torch.full((m,), sentinel, dtype=torch.uint8, device=dev), torch.full((1,), -1, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t.numel() else None
    rc = _lib.hip_lib().hmse_lines_extent(ptr(raw_d), raw_d.numel(), ro.data_ptr(), len(raw_off) - 1, cu.data_ptr(), ptr(sl),
                                          len(slot) if n_chunks is None else n_chunks, ptr(p), n, NL, 0, 0, 100, start.data_ptr(), end.data_ptr(),
                                          flags.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return start.tolist(), end.tolist(), flags.tolist(), int(status.item())


def test_bad_positions_and_inconsistent_tables(dev):
    from hmse_amd import ops
    corpus = _text(300, seed=2)
    cuts = [0, 100, 100, 250, 300]
    n = len(corpus)
    got, status = check_extent(dev, corpus, cuts, [5, n, 299, n + 1, 1 << 40, -1, 0, 2 ** 63 - 1], NL, 1, 1)
    assert status == 1 and [g[2] == BAD for g in got] == [False, True, False, True, True, True, False, True]
    raw, raw_off, slot = ref.tables(corpus, cuts)
    pos = [0, 5, 299, 300]
    good = _raw_extent(dev, raw, raw_off, cuts, slot, pos)
    assert good[3] == 1 and good[2] == [0, 0, 0, BAD] and good[0][1] == ref.extent(corpus, 5)[0]
    for bad_cuts, bad_slot, bad_off in (([0, 100, 90, 250, 300], slot, raw_off),            # cuts descend
                                        (cuts, [0, 1, len(raw_off) - 1, 3], raw_off),        # a slot outside the index
                                        ([0, 100, 100, 250, 301], slot, raw_off),            # a chunk longer than its record
                                        ([1, 100, 100, 250, 300], slot, raw_off),            # the corpus does not start at 0
                                        (cuts, slot, raw_off[:-1] + [raw_off[-1] + 50])):    # records beyond raw
        start, end, flags, status = _raw_extent(dev, raw, bad_off, bad_cuts, bad_slot, pos)
        assert status == 2 and start == [0] * 4 and end == [0] * 4 and flags == [BAD] * 4
        i64 = lambda v: _t(np.asarray(v, np.int64), dev)
        with pytest.raises(ops.HmseError, match="inconsistent tables"):
            ops.lines_extent(_t(raw, dev), i64(bad_off), i64(bad_cuts), i64(bad_slot), i64(pos), NL, 0, 0, 16)
    # n = 0: the status word is cleared, nothing else is written; through the wrapper: empty outputs
    start, end, flags, status = _raw_extent(dev, raw, raw_off, cuts, slot, [], n=0)
    assert status == 0 and start == [-7] and flags == [0x5A]
    got, status = check_extent(dev, corpus, cuts, [])
    assert got == [] and status == 0
    # n_chunks = 0: N = 0, every position is bad
    start, end, flags, status = _raw_extent(dev, b"", [0], [0], [], [0, 1, 7])
    assert status == 1 and start == [0] * 3 and end == [0] * 3 and flags == [BAD] * 3
    got, status = check_extent(dev, b"", [0, 0, 0], [0, 3])                                  # empty chunks only
    assert status == 1


# ---- 6. gather ---------------------------------------------------------------------------------------------------------------------------
def check_gather(dev, corpus, cuts, start, end, tabs=None, place=None):
    import torch
    from hmse_amd import ops
    tabs = tabs or _tables(dev, corpus, cuts, place)
    place = place or (lambda x, **kw: _t(x, dev))
    want, off = ref.text(corpus, start, end)
    i64 = lambda v: place(np.asarray(v, np.int64).reshape(-1))
    out = ops.lines_gather(*tabs, i64(start), i64(end), i64(off), off[-1])
    assert out.dtype == torch.uint8 and out.numel() == off[-1]
    got = out.cpu().numpy().tobytes()
    assert got == want, next(i for i in range(len(start)) if got[off[i]: off[i + 1]] != want[off[i]: off[i + 1]])
    return out


def test_gather_over_tiny_chunks_empty_ranges_and_every_misalignment(dev):
    corpus = _text(6000, seed=3)
    ch = _chunkings(corpus)
    rng = np.random.default_rng(6)
    for name in ("tiny", "ragged", "one", "behind-delimiters"):
        tabs = _tables(dev, corpus, ch[name])
        a = rng.integers(0, len(corpus) + 1, 120)
        b = rng.integers(0, len(corpus) + 1, 120)
        s, e = np.minimum(a, b), np.maximum(a, b)
        e[::7] = s[::7]                                                                     # empty ranges, some at N
        s[3], e[3], s[4], e[4] = 0, len(corpus), len(corpus), len(corpus)
        e[10:40] = np.minimum(s[10:40] + rng.integers(1, 40, 30), len(corpus))              # short ones
        check_gather(dev, corpus, ch[name], s.tolist(), e.tolist(), tabs=tabs)
        check_gather(dev, corpus, ch[name], [], [], tabs=tabs)
    # every pair (source misalignment i, destination misalignment j) in one launch: one record at an aligned address, range k = 16 i + j
    # starts at 1024 + i (mod 16) and every length is 1 (mod 16), so out_off[k] = j (mod 16)
    s = [1024 + 16 * (k % 5) + (k // 16) for k in range(256)]
    e = [p + (1, 17, 33, 49, 1041)[k % 5] for k, p in enumerate(s)]
    out = check_gather(dev, corpus, [0, len(corpus)], s, e)
    off = ref.text(corpus, s, e)[1]
    assert out.data_ptr() % 16 == 0 and {(p % 16, q % 16) for p, q in zip(s, off)} == {(i, j) for i in range(16) for j in range(16)}


def test_gather_pieces_of_0_1_15_16_17_bytes_at_odd_destinations(dev):
    """The head, body and tail of the per-piece copy: pieces of 0, 1, 15, 16 and 17 bytes that each start at an odd byte of `out` (one-byte
    fillers in front where needed) — once as ranges of their own inside one chunk, once as the chunks that one range crosses."""
    corpus = _text(400, seed=8)
    lens, odd = [3], []                                      # 3 bytes first: what follows starts at an odd offset
    for L in (0, 1, 15, 16, 17):
        if sum(lens) % 2 == 0:
            lens.append(1)
        odd.append(len(lens))
        lens.append(L)
    bounds = np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert all(bounds[k] % 2 == 1 for k in odd) and [lens[k] for k in odd] == [0, 1, 15, 16, 17]
    s = [100 + 7 * k for k in range(len(lens))]
    out = check_gather(dev, corpus, [0, len(corpus)], s, [p + L for p, L in zip(s, lens)])
    assert out.data_ptr() % 16 == 0 and ref.text(corpus, s, [p + L for p, L in zip(s, lens)])[1][:len(lens) + 1] == bounds
    check_gather(dev, corpus, bounds + [len(corpus)], [0, 0], [bounds[-1], len(corpus)])


def test_gather_one_range_is_the_whole_corpus(dev):
    corpus = _text(100_003, seed=4, every=40)
    cuts = _chunkings(corpus)["ragged"]
    check_gather(dev, corpus, cuts, [0, 0, 1], [len(corpus), 0, len(corpus)])


def _raw_gather(dev, corpus, cuts, start, end, off, out_cap):
    import torch
    from hmse_amd import _lib
    raw_d, ro, cu, sl = _tables(dev, corpus, cuts)
    i64 = lambda v: _t(np.asarray(v, np.int64).reshape(-1), dev)
    s, e, o = i64(start), i64(end), i64(off)
    out = torch.full((max(out_cap, 1) + 64,), 0x5A, dtype=torch.uint8, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    rc = _lib.hip_lib().hmse_lines_gather(raw_d.data_ptr(), raw_d.numel(), ro.data_ptr(), ro.numel() - 1, cu.data_ptr(), sl.data_ptr(), sl.numel(),
                                          s.data_ptr(), e.data_ptr(), o.data_ptr(), len(start), out.data_ptr(), out_cap, status.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(status.item())


def test_a_refused_gather_writes_nothing(dev):
    from hmse_amd import ops
    corpus = _text(2000, seed=5)
    cuts = _chunkings(corpus)["ragged"]
    n = len(corpus)
    s, e = [0, 100, 700, 1500], [50, 100, 1400, 2000]
    want, off = ref.text(corpus, s, e)
    out, status = _raw_gather(dev, corpus, cuts, s, e, off, off[-1])
    assert status == 0 and out[:off[-1]].tobytes() == want and (out[off[-1]:] == 0x5A).all()
    out, status = _raw_gather(dev, corpus, cuts, s, e, off, off[-1] - 1)                       # one byte short
    assert status == 1 and (out == 0x5A).all()
    for s2, e2, off2 in ((s, e, [0, 50, 51, 751, 1251]),                                       # out_off is not the prefix sum
                         (s, e[:3] + [n + 1], off[:4] + [off[4] + 1]),                         # end > N, out_off agreeing with it
                         (s, e[:3] + [n + 1], off),
                         ([0, 100, 1400, 1500], [50, 100, 700, 2000], off),                    # a range that descends
                         (s, e, [-10, 40, 40, 740, 1240])):                                    # out_off wraps: 2^64 - 10, then 40
        out, status = _raw_gather(dev, corpus, cuts, s2, e2, off2, off[-1] + 8)
        assert status == 2 and (out == 0x5A).all(), (s2, e2, off2)
    tabs = _tables(dev, corpus, cuts)
    i64 = lambda v: _t(np.asarray(v, np.int64), dev)
    with pytest.raises(ops.HmseError, match="prefix sum"):
        ops.lines_gather(*tabs, i64(s), i64(e), i64([0, 50, 51, 751, 1251]), off[-1])
    with pytest.raises(ops.HmseError, match="exceeds the output"):
        ops.lines_gather(*tabs, i64(s), i64(e), i64(off), off[-1] - 1)


# ---- 7. arguments only -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["random", "ones", "zero"])
def test_both_calls_on_poisoned_misaligned_guarded_memory(dev, monkeypatch, pattern):
    """Inputs off their alignment between guard bands (the last record ends at raw's guarded end), outputs and status words from poisoned
    memory: every output is fully determined — the bad positions included — and no guard band is touched."""
    ar = A_.Arena(dev, pattern, seed=11).install(monkeypatch, distrust_zeros=True, byte_misalign=3)
    place = lambda x, side=None: ar.place(x, misalign=5 if side == "raw" else 0)
    corpus = _text(5 * T + 9, seed=7)
    n = len(corpus)
    for cuts in (_chunkings(corpus)["tiny"], _chunkings(corpus)["ragged"]):
        tabs = _tables(dev, corpus, cuts, place)
        pos = list(range(0, n, 3)) + [n - 1, n, n + 5]
        for b, a, R in ((0, 0, 1 << 16), (2, 1, T + 1), (1, 3, 7)):
            got, status = check_extent(dev, corpus, cuts, pos, NL, b, a, R, tabs=tabs, place=place)
            assert status == 1 and got[-1] == (0, 0, BAD)
        s = [0, 3, 17, n, 40, 0]
        e = [n, 3, 2 * T + 30, n, 41, 16]
        check_gather(dev, corpus, cuts, s, e, tabs=tabs, place=place)
    ar.check()


# ---- 8. stores ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stores(dev):
    import torch
    from hmse_amd import IngestConfig, find, ingest, manifest, read
    cfg = IngestConfig(seg_size=SEG)
    out = {}
    for k, d in corpora().items():
        if k == "B2":
            continue
        m = manifest.Manifest.from_bytes(manifest.build_manifest(ingest.ingest_shard(torch.from_numpy(d).to(dev), cfg)).to_bytes())
        corpus = read.read_manifest(m, dev).cpu().numpy().tobytes()
        assert corpus == d.tobytes()
        out[k] = (m, find.StoreFinder(m, dev), corpus)
    return cfg, out


PATS = [b"\n== ", b"hzms", b"no such words here", b"the", b"the", b"qt"]


def _same_lines(got, want):
    import torch
    for f in ("ptr", "start", "end", "hits", "counts"):
        assert getattr(got, f).dtype == torch.int64 and getattr(got, f).tolist() == want[f], f
    assert got.flags.dtype == torch.uint8 and got.flags.tolist() == want["flags"]


def _invariants(ln, found):
    ptr = ln.ptr.tolist()
    assert ptr[0] == 0 and ptr[-1] == ln.start.numel() == ln.end.numel() == ln.flags.numel() == ln.hits.numel()
    for j in range(len(ptr) - 1):
        lo, hi = ptr[j], ptr[j + 1]
        assert int(ln.hits[lo:hi].sum()) == int(found.counts[j]) and int(ln.counts[j]) == hi - lo
        pairs = list(zip(ln.start[lo:hi].tolist(), ln.end[lo:hi].tolist()))
        assert pairs == sorted(set(pairs))


@pytest.mark.parametrize("name", ["A", "B"])
def test_grep_on_stores_equals_the_reference(dev, stores, name):
    from hmse_amd import KIND_DELTA, KIND_POINTER
    cfg, out = stores
    m, fd, corpus = out[name]
    assert (m.chunk_map["kind"] == KIND_DELTA).any() and (m.chunk_map["kind"] == KIND_POINTER).any()
    found = fd.find(PATS)
    ref_found = find_ref.find(corpus, PATS)
    assert found.counts.tolist() == ref_found[0] and ref_found[0][0] > 10 and ref_found[0][1] > 500 and ref_found[0][2] == 0
    for b, a, reach in ((0, 0, 1 << 16), (2, 1, 1 << 16), (0, 0, 40), (1, 1, 100)):
        ln = fd.grep(PATS, before=b, after=a, reach=reach)
        want = ref.lines(corpus, ref_found, NL, b, a, reach)
        _same_lines(ln, want)
        _invariants(ln, found)
        assert ln.counts.tolist()[3] == ln.counts.tolist()[4] and ln.counts.tolist()[2] == 0       # two equal patterns; an absent one
        assert bool(ln.flags.any()) == (reach < 1000)                                              # a small reach cuts
        data, off = fd.text(ln)
        want_text, want_off = ref.text(corpus, want["start"], want["end"])
        assert off.tolist() == want_off and data.cpu().numpy().tobytes() == want_text
    ln = fd.grep(PATS)
    assert ln.counts.tolist()[1] == sum(1 for s in corpus.split(b"\n") if b"hzms" in s)              # grep -c
    # ignore_case; another delimiter; a tensor of offsets (unsorted, one twice) taken as one pattern
    ic = fd.grep([b"ETR", b"hZmS"], ignore_case=True, before=1)
    _same_lines(ic, ref.lines(corpus, find_ref.find(corpus, [b"ETR", b"hZmS"], True), NL, 1, 0))
    sp = fd.grep([b"hzms"], delim=b" ", after=1)
    _same_lines(sp, ref.lines(corpus, find_ref.find(corpus, [b"hzms"]), 0x20, 0, 1))
    offs = found.offsets[found.ptr[0]: found.ptr[1]]
    one = fd.lines(offs.flip(0).repeat(2)[:-1], after=1)
    twice = offs.tolist() * 2
    _same_lines(one, ref.lines(corpus, ([len(twice) - 1], [0, len(twice) - 1], sorted(twice[1:])), NL, 0, 1))
    data, off = fd.text((one.start, one.start + 5))
    assert data.cpu().numpy().tobytes() == b"".join(corpus[s: s + 5] for s in one.start.tolist())


def test_lines_limits_and_edges(dev, stores):
    import torch
    from hmse_amd import find, manifest
    cfg, out = stores
    m, fd, corpus = out["A"]
    with pytest.raises(ValueError, match=f"offset {fd.n_bytes} is not below n_bytes = {fd.n_bytes}"):
        fd.lines(torch.tensor([5, fd.n_bytes, 7], dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="offset -1 "):
        fd.lines(torch.tensor([-1], dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="int64"):
        fd.lines(torch.tensor([1], dtype=torch.int32, device=dev))
    ln = fd.grep([b"hzms"], before=2, after=2)
    total = int((ln.end - ln.start).sum())
    with pytest.raises(ValueError, match=f"hold {total} bytes"):
        fd.text(ln, max_bytes=total - 1)
    assert fd.text(ln, max_bytes=total)[0].numel() == total
    for z in (fd.grep([]), fd.grep([b"no such words here"]), fd.lines(torch.zeros(0, dtype=torch.int64, device=dev))):
        P = z.counts.numel()
        assert z.ptr.tolist() == [0] * (P + 1) and z.counts.tolist() == [0] * P
        assert all(getattr(z, f).numel() == 0 and getattr(z, f).device.type == "cuda" for f in ("start", "end", "flags", "hits"))
        assert z.flags.dtype == torch.uint8 and z.hits.dtype == torch.int64
        data, off = fd.text(z)
        assert data.numel() == 0 and data.dtype == torch.uint8 and off.tolist() == [0]
    empty = find.StoreFinder(manifest.Store([]), dev)
    z = empty.grep([b"a", b"bc"], before=1)
    assert z.ptr.tolist() == [0, 0, 0] and z.counts.tolist() == [0, 0] and z.start.numel() == 0 and empty.text(z)[0].numel() == 0
    with pytest.raises(ValueError, match="n_bytes = 0"):
        empty.lines(torch.zeros(1, dtype=torch.int64, device=dev))
    got = find.grep(m, [b"\n== "], dev, after=1)                                                     # the one-off form
    _same_lines(got, ref.lines(corpus, find_ref.find(corpus, [b"\n== "]), NL, 0, 1))


def test_two_shard_merged_store_gives_the_one_shard_lines(dev, stores):
    import torch
    from hmse_amd import find, ingest, manifest
    cfg, out = stores
    m, fd1, corpus = out["A"]
    d = np.frombuffer(corpus, np.uint8)
    half = 3 * SEG
    rs = ingest.ingest_shards_local([torch.from_numpy(d[:half].copy()).to(dev), torch.from_numpy(d[half:].copy()).to(dev)], cfg)
    st = manifest.Store.from_bytes(manifest.merge_manifests([manifest.build_manifest(r, i, 2) for i, r in enumerate(rs)]).to_bytes())
    assert len(st.shards) == 2
    fd2 = find.StoreFinder(st, dev)
    for kw in (dict(), dict(before=2, after=1), dict(reach=33)):
        a, b = fd1.grep(PATS, **kw), fd2.grep(PATS, **kw)
        assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("ptr", "start", "end", "flags", "hits", "counts"))
        assert torch.equal(fd1.text(a)[0], fd2.text(b)[0])
    across = fd2.lines(torch.tensor([half - 1, half], dtype=torch.int64, device=dev), before=1, after=1)   # a line across the shards
    _same_lines(across, ref.lines(corpus, ([2], [0, 2], [half - 1, half]), NL, 1, 1))
