"""GPU: the order of search results (hmse_amd.find sort / sort_regex; hmse_order_keys / hmse_order_lcp) against the plain-Python reference
of tests/order_ref.py — the two kernels on synthetic chunk maps (every range of a small corpus under five chunkings at depth 0, at its
end and in between; pairs whose first difference lies at the edges, at the trip edge and on either side of the chunk seams; a `from`
behind bytes that differ; folding of exactly A..Z; bad input), the rounds with the skip on and off, on poisoned / misaligned / guarded
memory (tests/arena.py), and on stores with POINTER and DELTA records against re.finditer and sorted().  All results are compared bit
for bit.  The shapes are the smallest at which the kernels can go wrong."""
import bisect
import collections
import os
import re

import numpy as np
import pytest

import arena as A_
import lines_ref
import order_ref as ref
from test_sync_host import SEG, corpora

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc", "order.hip")).read()
T = int(re.search(r"constexpr uint32_t ORDER_TRIP = (\d+);", _SRC).group(1))             # bytes one trip of the LCP walk looks at
FIELDS = ("ptr", "index", "start", "end", "first", "count", "distinct", "total", "rank_of")


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
    raw, raw_off, slot = lines_ref.tables(corpus, cuts)
    i64 = lambda v: np.asarray(v, np.int64).reshape(-1)
    return place(np.frombuffer(raw, np.uint8).copy(), side="raw"), place(i64(raw_off)), place(i64(cuts)), place(i64(slot))


# ---- 1. keys: every range of a small corpus ------------------------------------------------------------------------------------------------
BLOCK = 20                                               # one record placed at three corpus positions


def _keys_corpus():
    rng = np.random.default_rng(1)
    n = 3 * T + 37
    c = rng.integers(0, 256, n, dtype=np.uint8)
    up = rng.random(n) < 0.3
    c[up] = rng.integers(65, 91, int(up.sum()), dtype=np.uint8)                            # enough A..Z for the folding to matter
    c[rng.random(n) < 0.05] = 0                                                            # and true zero bytes, which r tells from padding
    for at in (70, 150):
        c[at: at + BLOCK] = c[5: 5 + BLOCK]
    return c.tobytes()


@pytest.fixture(scope="module")
def every_range():
    """-> (corpus, starts, ends, {which: depths}, {(which, fold): keys}): the 26 335 non-empty ranges of the corpus and a few empty ones,
    at depth 0, at depth L and at a seeded depth in between, their reference keys once"""
    corpus = _keys_corpus()
    n = len(corpus)
    assert n == 3 * T + 37 == 229 and corpus[5: 5 + BLOCK] == corpus[70: 70 + BLOCK] == corpus[150: 150 + BLOCK] and 0 in corpus
    pairs = [(s, e) for s in range(n) for e in range(s + 1, n + 1)]
    assert len(pairs) == 26335
    pairs += [(0, 0), (n, n), (T, T), (70, 70)]
    starts, ends = [p[0] for p in pairs], [p[1] for p in pairs]
    rng = np.random.default_rng(8)
    lens = np.asarray(ends) - np.asarray(starts)
    near = np.maximum(lens - rng.integers(0, 10, len(pairs)), 0)                           # half of the sample within nine bytes of the end
    depths = {"zero": [0] * len(pairs), "end": lens.tolist(), "between": np.where(rng.random(len(pairs)) < 0.5, near, rng.integers(0, lens + 1)).tolist()}
    want = {(w, f): ref.keys(corpus, starts, ends, d, f) for w, d in depths.items() for f in (False, True)}
    assert sum(a != b for a, b in zip(want["zero", False], want["zero", True])) > 15000 and set(want["end", False]) == {0}
    assert {k & 15 for k in want["between", False]} == set(range(9)) and max(want["zero", True]) < 1 << 60
    return corpus, starts, ends, depths, want


def _key_chunkings(n):
    rng = np.random.default_rng(5)
    tiny = [0]
    while tiny[-1] < n:
        tiny.append(min(tiny[-1] + int(rng.integers(0, 3)), n))
    edges = sorted({0, n, *(k * T + d for k in range(1, 4) for d in (-1, 0, 1))})
    return {"one": [0, n], "bytes": list(range(n + 1)), "tiny-and-empty": tiny + [n, n], "trip-edges": edges,
            "one-record-three-places": [0, 5, 5 + BLOCK, 70, 70 + BLOCK, 150, 150 + BLOCK, n]}


def _seams_in_windows(cuts, starts, ends, depths):
    """the largest number of chunk seams strictly inside a key's window [p, p + m) over the cases, m = min(L - d, 7)"""
    inner = sorted(set(cuts[1:-1]))
    most = 0
    for s, e, d in zip(starts, ends, depths):
        p, m = s + d, min(e - s - d, 7)
        most = max(most, bisect.bisect_left(inner, p + m) - bisect.bisect_right(inner, p))     # the cuts c with p < c < p + m
    return most


@pytest.mark.parametrize("name", ["one", "bytes", "tiny-and-empty", "trip-edges", "one-record-three-places"])
def test_keys_of_every_range_of_a_small_corpus_at_three_depths(dev, every_range, name):
    """The window of a key crosses one seam in every chunking that has a seam and two seams in every chunking that has two within six
    bytes (all but the single chunk and the three places of one record, whose seams lie at least twenty bytes apart)."""
    import torch
    from hmse_amd import ops
    corpus, starts, ends, depths, want = every_range
    cuts = _key_chunkings(len(corpus))[name]
    assert cuts[0] == 0 and cuts[-1] == len(corpus) and cuts == sorted(cuts)
    if name == "tiny-and-empty":
        assert set(np.diff(cuts).tolist()) == {0, 1, 2}
    if name == "one-record-three-places":
        slot = lines_ref.tables(corpus, cuts)[2]
        assert slot[1] == slot[3] == slot[5]
    for which in ("zero", "between"):
        seams = _seams_in_windows(cuts, starts, ends, depths[which])
        assert seams >= {"one": 0, "one-record-three-places": 1}.get(name, 2), (which, seams)
    tabs = _tables(dev, corpus, cuts)
    s, e = _t(np.asarray(starts, np.int64), dev), _t(np.asarray(ends, np.int64), dev)
    for which, d in depths.items():
        dd = _t(np.asarray(d, np.int64), dev)
        for fold in (False, True):
            key = ops.order_keys(*tabs, s, e, dd, fold)
            assert key.dtype == torch.int64 and key.numel() == len(starts)
            got = key.tolist()
            w = want[which, fold]
            assert got == w, next((starts[i], ends[i], d[i], hex(g), hex(x)) for i, (g, x) in enumerate(zip(got, w)) if g != x)


# ---- 2. lcp ----------------------------------------------------------------------------------------------------------------------------------
def _lcp_case():
    """Segments of L bytes back to back: 0 = the text (the rep, cut at 30), then copies cut at 70 — 1: equal, 2..7: one byte changed (the
    first, the last, the bytes on either side of the copy's seam and of the rep's seam), 8: equal in 1-byte chunks, 9: equal and uncut
    (the rep of 10 and 11), 10 and 11: uncut, byte 63 and byte 64 changed — lane 63 of the first trip and lane 0 of the second."""
    L = 2 * T + 22
    rng = np.random.default_rng(2)
    text = rng.integers(97, 123, L, dtype=np.uint8)
    changed = {2: 0, 3: L - 1, 4: 69, 5: 70, 6: 29, 7: 30, 10: T - 1, 11: T}
    segs, cuts = [], [0]
    for k in range(12):
        sgm = text.copy()
        if k in changed:
            sgm[changed[k]] ^= 0x01
        segs.append(sgm.tobytes())
        base = k * L
        inner = [30] if k == 0 else list(range(1, L)) if k == 8 else [] if k >= 9 else [70]
        cuts += [base + c for c in inner] + [base + L]
    return b"".join(segs), cuts, L, changed


def test_lcp_first_difference_at_the_edges_the_trip_edge_and_the_seams(dev):
    import torch
    from hmse_amd import ops
    corpus, cuts, L, changed = _lcp_case()
    assert T == 64 and L == 150
    tabs = _tables(dev, corpus, cuts)
    seg = lambda k, a=0, b=None: (k * L + a, k * L + (L if b is None else b))
    cases = [(*seg(k), 0, 0) for k in range(9)]                              # 0..8: segment k against the rep, segment 0 (0: the very range)
    cases += [(*seg(9), 0, 0), (*seg(10), 9, 0), (*seg(11), 9, 0)]           # 9: the uncut copy; 10, 11 against it: lane 63, lane 0 of the second trip
    cases += [(*seg(1, 0, 100), 0, 0), (*seg(0), 12, 0)]                     # 12, 13: a proper prefix against the text, the text against its prefix
    cases += [(*seg(1, 0, 0), 0, 0), (*seg(5, 7, 7), 14, 0)]                 # 14, 15: the empty text against the text, against the empty text
    cases += [(*seg(2), 16, 0), (*seg(3, 0, 0), 17, 0)]                      # 16, 17: rep[i] == i — the length, no byte read
    cases += [(*seg(2), 0, 1), (*seg(6), 0, 30), (*seg(10), 9, T), (*seg(4), 0, 70)]       # 18..21: from behind a byte that DIFFERS: it is not looked at
    cases += [(*seg(1), 0, L), (*seg(1, 0, 100), 0, 100), (*seg(3), 0, L - 1), (*seg(5), 0, 70)]   # 22..25: from == min(L); from ON the first difference
    cases += [(*seg(8), 1, 40), (*seg(1), 8, 69)]                            # 26, 27: equal texts under different chunk splits, from inside a chunk
    starts, ends, rep, frm = ([c[j] for c in cases] for j in range(4))
    want = ref.lcp(corpus, starts, ends, rep, frm)
    assert want == [L, L, 0, L - 1, 69, 70, 29, 30, L] + [L, T - 1, T] + [100, 100] + [0, 0] + [L, 0] + [L, L, L, L] + [L, 100, L - 1, 70] + [L, L]
    i64 = lambda v: _t(np.asarray(v, np.int64), dev)
    for fold in (False, True):
        got = ops.order_lcp(*tabs, i64(starts), i64(ends), i64(rep), i64(frm), fold)
        assert got.dtype == torch.int64 and got.tolist() == want, fold
    # the other way round: the answer is symmetric in i and rep
    back = list(range(12)), [1, 0, 0, 0, 0, 0, 0, 0, 1, 10, 9, 9]
    s2, e2 = [seg(k)[0] for k in back[0]], [seg(k)[1] for k in back[0]]
    got = ops.order_lcp(*tabs, i64(s2), i64(e2), i64(back[1]), i64([0] * 12)).tolist()
    assert got == ref.lcp(corpus, s2, e2, back[1], [0] * 12) == [L, L, 0, L - 1, 69, 70, 29, 30, L, T - 1, T - 1, T]


def test_folding_of_exactly_a_to_z(dev):
    from hmse_amd import ops
    upper = bytes(range(65, 91)) + b"@[\xc1\x00_"                             # and five bytes whose | 0x20 form is another byte, no letter
    corpus = upper + bytes(b | 0x20 for b in upper)
    n = len(upper)
    for cuts in ([0, 2 * n], list(range(2 * n + 1)), [0, n, 2 * n]):
        tabs = _tables(dev, corpus, cuts)
        i64 = lambda v: _t(np.asarray(v, np.int64), dev)
        # every byte against its | 0x20 form (and back); the whole upper half against the lower one, and the five others alone
        s = list(range(2 * n)) + [0, n, 26, n + 26]
        e = [p + 1 for p in range(2 * n)] + [n, 2 * n, n, 2 * n]
        rep = [(p + n) % (2 * n) for p in range(2 * n)] + [2 * n + 1, 2 * n, 2 * n + 3, 2 * n + 2]
        zero = [0] * len(s)
        folded = ops.order_lcp(*tabs, i64(s), i64(e), i64(rep), i64(zero), True).tolist()
        exact = ops.order_lcp(*tabs, i64(s), i64(e), i64(rep), i64(zero), False).tolist()
        assert folded == ref.lcp(corpus, s, e, rep, zero, True) and exact == ref.lcp(corpus, s, e, rep, zero, False)
        assert folded[:n] == folded[n: 2 * n] == [1] * 26 + [0] * 5 and folded[2 * n:] == [26, 26, 0, 0] and exact == [0] * len(s)
        kf, ke = ops.order_keys(*tabs, i64(s), i64(e), i64(zero), True).tolist(), ops.order_keys(*tabs, i64(s), i64(e), i64(zero), False).tolist()
        assert kf == ref.keys(corpus, s, e, zero, True) and ke == ref.keys(corpus, s, e, zero, False)
        assert [kf[p] == kf[p + n] for p in range(n)] == [True] * 26 + [False] * 5 and len(set(ke[: 2 * n])) == 2 * n


# ---- 3. the rounds ---------------------------------------------------------------------------------------------------------------------------
def _finder(dev, corpus, cuts):
    """a StoreFinder over a synthetic chunk map (no store behind it): what sort reads"""
    from hmse_amd import find
    fd = find.StoreFinder.__new__(find.StoreFinder)
    fd.dev = dev
    fd.raw, fd.raw_off, fd.cuts, fd.slot = _tables(dev, corpus, cuts)
    fd.n_bytes, fd.n_records = len(corpus), int(fd.raw_off.numel()) - 1
    return fd


def _same_sorted(got, want):
    import torch
    for f in FIELDS:
        t = getattr(got, f)
        assert t.dtype == (torch.bool if f == "first" else torch.int64) and t.device.type == "cuda" and t.tolist() == want[f], f


def _equal(a, b):
    import torch
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


@pytest.fixture(scope="module")
def grouped():
    """a corpus of words from a vocabulary of 36 (some differ in case only, some are prefixes of others, three are longer than a trip and
    differ behind it), 3000 ranges over whole words, three word pairs and empty texts, in three groups (one of them empty)
    -> (corpus, cuts, starts, ends, ptr, {(ic, unique): reference})"""
    rng = np.random.default_rng(4)
    vocab = [bytes([97 + j // 5, 97 + j % 5]) + bytes(rng.integers(97, 123, int(rng.integers(0, 10)), dtype=np.uint8)) for j in range(24)]
    vocab += [w.upper() for w in vocab[:8]] + [b"x" * (T + 3), b"x" * (T + 2) + b"y", b"X" * (T + 3), b"q"]
    assert len(set(vocab)) == 36
    words, bounds = [], [0]
    for _ in range(1500):
        w = vocab[int(rng.integers(0, 36) if rng.random() < 0.5 else rng.integers(0, 5))]
        words.append(w)
        bounds.append(bounds[-1] + len(w))
    corpus = b"".join(words)
    cuts = sorted({0, len(corpus), *rng.integers(1, len(corpus), 400).tolist()})
    starts, ends = [], []
    for _ in range(3000):
        k = int(rng.integers(0, 1500))
        r = rng.random()
        if r >= 0.93:
            k = (10, 500, 1200)[k % 3]                                        # three two-word texts, whatever lies there
        s, e = (bounds[k], bounds[k + 1]) if r < 0.9 else (bounds[k], bounds[k]) if r < 0.93 else (bounds[k], bounds[k + 2])
        starts.append(s); ends.append(e)
    ptr = [0, 1700, 1700, 3000]
    refs = {(ic, u): ref.order(corpus, starts, ends, ptr, ic, u) for ic in (False, True) for u in (False, True)}
    assert 40 >= max(refs[False, False]["distinct"]) > max(refs[True, False]["distinct"]) >= 25
    return corpus, cuts, starts, ends, ptr, refs


@pytest.mark.parametrize("ic", [False, True])
def test_sort_is_the_reference_s_with_the_skip_on_and_off(dev, grouped, ic):
    corpus, cuts, starts, ends, ptr, refs = grouped
    fd = _finder(dev, corpus, cuts)
    i64 = lambda v: _t(np.asarray(v, np.int64), dev)
    what = (i64(starts), i64(ends), i64(ptr))
    s = fd.sort(what, ignore_case=ic)                                      # 3000 ranges, at most 40 distinct values per group
    _same_sorted(s, refs[ic, False])
    assert s.total.tolist() == [1700, 0, 1300] and s.ptr.tolist() == ptr and int(s.first.sum()) == int(s.distinct.sum())
    slow = fd.sort(what, ignore_case=ic, _skip=False)
    assert _equal(s, slow) and 2 <= s.rounds < slow.rounds                 # the x..x words agree for more than a trip: 64 / 7 rounds without the skip
    u = fd.sort(what, ignore_case=ic, unique=True)
    _same_sorted(u, refs[ic, True])
    assert _equal(u, fd.sort(what, ignore_case=ic, unique=True, _skip=False))
    assert int(u.count.sum()) == 3000 and u.ptr.tolist() == [0, int(u.distinct[0]), int(u.distinct[0]), int(u.distinct.sum())]
    data, off = fd.text(u)                                                 # text() takes a Sorted: the ranges in order
    want = lines_ref.text(corpus, refs[ic, True]["start"], refs[ic, True]["end"])
    assert data.cpu().numpy().tobytes() == want[0] and off.tolist() == want[1]
    texts = [ref.text_of(want[0], a, b, ic) for a, b in zip(want[1][:-1], want[1][1:])]
    for j in range(3):
        part = texts[u.ptr[j]: u.ptr[j + 1]]
        assert part == sorted(set(part))                                   # sort -u


def test_sort_of_one_range_of_empty_ranges_and_max_rounds(dev, grouped):
    import torch
    corpus, cuts, starts, ends, ptr, refs = grouped
    fd = _finder(dev, corpus, cuts)
    i64 = lambda v: _t(np.asarray(v, np.int64), dev)
    one = fd.sort((i64([5]), i64([9])))
    _same_sorted(one, ref.order(corpus, [5], [9], [0, 1]))
    assert (one.ptr.tolist(), one.index.tolist(), one.start.tolist(), one.end.tolist(), one.first.tolist(), one.rank_of.tolist(), one.rounds) == ([0, 1], [0], [5], [9], [True], [0], 1)
    n = len(corpus)
    s, e, p = [7, 0, n, 3, 7], [7, 0, n, 3, 8], [0, 2, 5]                  # empty texts equal each other and come first of all, in their own group
    empties = fd.sort((i64(s), i64(e), i64(p)))
    _same_sorted(empties, ref.order(corpus, s, e, p))
    assert empties.index.tolist() == [1, 0, 3, 2, 4] and empties.first.tolist() == [True, False, True, False, True] and empties.rounds == 1
    chain = fd.sort((i64([0] * 30), i64([bounds for bounds in range(1, 31)])))          # prefixes of one text: eight lengths finish a round
    assert chain.index.tolist() == list(range(30)) and chain.rounds >= 4
    with pytest.raises(RuntimeError, match=r"sort: \d+ of 30 ranges are unresolved after max_rounds = 2 rounds"):
        fd.sort((i64([0] * 30), i64(list(range(1, 31)))), max_rounds=2)
    with pytest.raises(ValueError, match="descends or leaves the corpus"):
        fd.sort((i64([0]), i64([n + 1])))
    assert torch.cuda.is_available()


# ---- 4. bad input ----------------------------------------------------------------------------------------------------------------------------
def _raw_calls(dev, raw, raw_off, cuts, slot, starts, ends, depth, rep, frm):
    """hmse_order_keys and hmse_order_lcp through ctypes on outputs and status words that start as sentinels
    -> (keys, keys status, lcps, lcp status)."""
    import torch
    from hmse_amd import _lib
    i64 = lambda v: _t(np.asarray(v, np.int64).reshape(-1), dev)
    raw_d, ro, cu, sl, s, e, d, r, f = _t(raw, dev), i64(raw_off), i64(cuts), i64(slot), i64(starts), i64(ends), i64(depth), i64(rep), i64(frm)
    n = len(starts)
    key = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    lcp = torch.full((n + 1,), -9, dtype=torch.int64, device=dev)
    st = torch.full((2,), -1, dtype=torch.int32, device=dev)
    lib, stream = _lib.hip_lib(), torch.cuda.current_stream().cuda_stream
    common = (raw_d.data_ptr(), raw_d.numel(), ro.data_ptr(), len(raw_off) - 1, cu.data_ptr(), sl.data_ptr(), len(slot), s.data_ptr(), e.data_ptr())
    assert lib.hmse_order_keys(*common, d.data_ptr(), n, 1, key.data_ptr(), st.data_ptr(), stream) == 0
    assert lib.hmse_order_lcp(*common, r.data_ptr(), f.data_ptr(), n, 1, lcp.data_ptr(), st.data_ptr() + 4, stream) == 0
    torch.cuda.synchronize()
    assert key[n].item() == -7 and lcp[n].item() == -9                       # nothing behind the end
    return key[:n].tolist(), int(st[0].item()), lcp[:n].tolist(), int(st[1].item())


def test_refused_calls_set_status_bit_1_and_write_zeros(dev):
    from hmse_amd import ops
    rng = np.random.default_rng(6)
    corpus = rng.integers(65, 123, 300, dtype=np.uint8).tobytes()
    cuts = [0, 100, 100, 250, 300]
    raw, raw_off, slot = lines_ref.tables(corpus, cuts)
    starts, ends, depth, rep, frm = [0, 5, 90, 300], [50, 5, 260, 300], [0, 0, 170, 0], [0, 0, 2, 1], [0, 0, 170, 0]
    good = _raw_calls(dev, raw, raw_off, cuts, slot, starts, ends, depth, rep, frm)
    assert good == (ref.keys(corpus, starts, ends, depth, True), 0, ref.lcp(corpus, starts, ends, rep, frm, True), 0) and good[2] == [50, 0, 170, 0]
    zeros = ([0] * 4, 2, [0] * 4, 2)
    for s2, e2, d2, r2, f2, which in (([0, 5, 260, 300], [50, 5, 90, 300], depth, rep, frm, "both"),      # a range that descends
                                      (starts, [50, 5, 260, 301], depth, rep, frm, "both"),               # end > N
                                      (starts, [50, 5, 260, 1 << 62], depth, rep, frm, "both"),
                                      ([-1, 5, 90, 300], [-1, 5, 260, 300], depth, rep, frm, "both"),     # 2^64 - 1
                                      (starts, ends, [51, 0, 170, 0], rep, frm, "keys"),                  # depth > L
                                      (starts, ends, [0, 1, 170, 0], rep, frm, "keys"),                   # ... of an empty text
                                      (starts, ends, [0, 0, -1, 0], rep, frm, "keys"),
                                      (starts, ends, depth, [0, 0, 2, 4], frm, "lcp"),                    # rep >= n
                                      (starts, ends, depth, [0, -1, 2, 1], frm, "lcp"),
                                      (starts, ends, depth, rep, [51, 0, 170, 0], "lcp"),                 # from > L_i (rep[i] == i)
                                      (starts, ends, depth, rep, [0, 1, 170, 0], "lcp"),                  # from > L_i = 0
                                      (starts, ends, depth, [2, 0, 0, 1], [0, 0, 51, 0], "lcp"),          # from > L_rep = 50 < L_i
                                      (starts, ends, depth, rep, [0, 0, 170, -1], "lcp")):
        got = _raw_calls(dev, raw, raw_off, cuts, slot, s2, e2, d2, r2, f2)
        assert (got[:2] == zeros[:2]) if which in ("both", "keys") else (got[:2] == good[:2]), (which, s2, e2, d2)
        assert (got[2:] == zeros[2:]) if which in ("both", "lcp") else (got[2:] == good[2:]), (which, r2, f2)
    i64 = lambda v: _t(np.asarray(v, np.int64), dev)
    for bad_cuts, bad_slot, bad_off in (([0, 100, 90, 250, 300], slot, raw_off),               # cuts descend
                                        (cuts, [0, 1, len(raw_off) - 1, 3], raw_off),          # a slot outside the index
                                        ([0, 100, 100, 250, 301], slot, raw_off),              # a chunk longer than its record
                                        ([1, 100, 100, 250, 300], slot, raw_off),              # the corpus does not start at 0
                                        (cuts, slot, raw_off[:-1] + [raw_off[-1] + 50])):      # records beyond raw
        assert _raw_calls(dev, raw, bad_off, bad_cuts, bad_slot, starts, ends, depth, rep, frm) == zeros
        with pytest.raises(ops.HmseError, match="inconsistent tables"):
            ops.order_keys(_t(raw, dev), i64(bad_off), i64(bad_cuts), i64(bad_slot), i64(starts), i64(ends), i64(depth))
        with pytest.raises(ops.HmseError, match="inconsistent tables"):
            ops.order_lcp(_t(raw, dev), i64(bad_off), i64(bad_cuts), i64(bad_slot), i64(starts), i64(ends), i64(rep), i64(frm))
    tabs = _tables(dev, corpus, cuts)
    with pytest.raises(ops.HmseError, match="a depth beyond its text's end"):
        ops.order_keys(*tabs, i64(starts), i64(ends), i64([51, 0, 170, 0]))
    with pytest.raises(ops.HmseError, match="a from beyond the shorter of the two texts"):
        ops.order_lcp(*tabs, i64(starts), i64(ends), i64(rep), i64([51, 0, 170, 0]))
    # no chunks at all: N = 0, only (0, 0) is a range; then the run is still clean
    assert _raw_calls(dev, b"", [0], [0], [], [0, 0], [0, 0], [0, 0], [1, 0], [0, 0]) == ([0, 0], 0, [0, 0], 0)
    assert _raw_calls(dev, b"", [0], [0], [], [0, 0], [0, 1], [0, 0], [1, 0], [0, 0]) == ([0, 0], 2, [0, 0], 2)
    assert _raw_calls(dev, raw, raw_off, cuts, slot, starts, ends, depth, rep, frm) == good
    e = _t(np.zeros(0, np.int64), dev)
    assert ops.order_keys(*tabs, e, e, e).numel() == 0 and ops.order_lcp(*tabs, e, e, e, e).numel() == 0


# ---- 5. arguments only -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["random", "ones", "zero"])
def test_both_calls_on_poisoned_misaligned_guarded_memory(dev, monkeypatch, pattern):
    """Inputs off their alignment between guard bands (the last record ends at raw's guarded end), outputs and status words from poisoned
    memory: every output is fully determined and no guard band is touched."""
    ar = A_.Arena(dev, pattern, seed=11).install(monkeypatch, distrust_zeros=True, byte_misalign=3)
    from hmse_amd import ops
    place = lambda x, side=None: ar.place(x, misalign=5 if side == "raw" else 0)
    rng = np.random.default_rng(7)
    corpus = (rng.integers(60, 100, 2 * T + 9, dtype=np.uint8).tobytes()) * 2 + b"!"       # two copies: long common prefixes, up to the corpus' last byte
    n, half = len(corpus), 2 * T + 9
    tiny = [0]
    while tiny[-1] < n:
        tiny.append(min(tiny[-1] + int(rng.integers(0, 3)), n))
    for cuts in (tiny, sorted({0, n, *rng.integers(1, n, 12).tolist()}), [0, n]):
        tabs = _tables(dev, corpus, cuts, place)
        s = [0, 3, 17, n, 40, half, n - 1, half + 17, n - 8]
        e = [half, 3, 2 * T, n, 41, n, n, n, n]
        d = [0, 0, T, 0, 1, half - 3, 0, 9, 1]
        rep = [5, 3, 7, 1, 4, 0, 6, 2, 8]
        frm = [0, 0, 5, 0, 0, half, 0, 0, 0]
        i64 = lambda v: place(np.asarray(v, np.int64))
        for fold in (False, True):
            assert ops.order_keys(*tabs, i64(s), i64(e), i64(d), fold).tolist() == ref.keys(corpus, s, e, d, fold)
            assert ops.order_lcp(*tabs, i64(s), i64(e), i64(rep), i64(frm), fold).tolist() == ref.lcp(corpus, s, e, rep, frm, fold)
        assert ref.lcp(corpus, s, e, rep, frm)[0] == half and ref.lcp(corpus, s, e, rep, frm)[2] == 2 * T - 17
    ar.check()


# ---- 6. stores -------------------------------------------------------------------------------------------------------------------------------
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


def _host_sort(corpus, spans_per_group, ic=False):
    """re.finditer / line slices and sorted() -> per group the (text, start) of every range in order"""
    return [sorted(((corpus[s:e].lower() if ic else corpus[s:e]), s) for s, e in spans) for spans in spans_per_group]


def _as_lists(fd, srt, ic=False):
    data, off = fd.text(srt, max_bytes=1 << 30)
    data, off, ptr, st = data.cpu().numpy().tobytes(), off.tolist(), srt.ptr.tolist(), srt.start.tolist()
    texts = [data[off[i]: off[i + 1]] for i in range(len(off) - 1)]
    return [[(texts[i].lower() if ic else texts[i], st[i]) for i in range(ptr[j], ptr[j + 1])] for j in range(len(ptr) - 1)]


WORD, NUM = rb"[A-Za-z]+", rb"[0-9]+|== [A-Za-z ]+ =="


@pytest.mark.parametrize("name", ["A", "B"])
def test_sort_regex_sort_unique_and_sort_of_a_tally_on_stores(dev, stores, name):
    import torch
    from hmse_amd import KIND_DELTA, KIND_POINTER, find
    from hmse_amd.regex import Regex
    cfg, out = stores
    m, fd, corpus = out[name]
    assert (m.chunk_map["kind"] == KIND_DELTA).any() and (m.chunk_map["kind"] == KIND_POINTER).any()
    rxs = [Regex(WORD, device=dev), Regex(NUM, device=dev)]
    spans = [[mt.span() for mt in re.finditer(p, corpus)] for p in (WORD, NUM)]
    assert len(spans[0]) > 10000 and len(spans[1]) > 10
    base = [0, len(spans[0])]
    for ic in (False, True):
        s = fd.sort_regex(rxs, ignore_case=ic)
        want = _host_sort(corpus, spans, ic)
        assert _as_lists(fd, s, ic) == want                                  # grep -o RX | sort, equal texts by their start
        assert s.total.tolist() == [len(x) for x in spans] and s.distinct.tolist() == [len({t for t, _ in w}) for w in want]
        idx, rank = s.index.tolist(), s.rank_of.tolist()
        assert all(rank[idx[p]] == p - int(s.ptr[j]) for j in range(2) for p in range(int(s.ptr[j]), int(s.ptr[j + 1]), 53))
        assert all(spans[j][idx[p] - base[j]][0] == want[j][p - int(s.ptr[j])][1] for j in range(2) for p in range(int(s.ptr[j]), int(s.ptr[j + 1]), 53))
        u = fd.sort_regex(rxs, ignore_case=ic, unique=True)                  # sort -u, and with count: sort | uniq -c
        got = _as_lists(fd, u, ic)
        cnt = u.count.tolist()
        for j in range(2):
            distinct = sorted({t for t, _ in want[j]})
            assert [t for t, _ in got[j]] == distinct
            runs = collections.Counter(t for t, _ in want[j])
            assert cnt[int(u.ptr[j]): int(u.ptr[j + 1])] == [runs[v] for v in distinct]
        assert torch.equal(u.rank_of, s.rank_of)
        # a Tally: its values in lexicographic order, t.count[s.index] their counts
        t = fd.tally_regex(rxs, ignore_case=ic)
        st = fd.sort(t, ignore_case=ic)
        assert [[x for x, _ in g] for g in _as_lists(fd, st, ic)] == [[x for x, _ in g] for g in got] and bool(st.first.all())
        assert t.count[st.index].tolist() == cnt and st.ptr.tolist() == u.ptr.tolist() == t.ptr.tolist()
    # with and without the skip; the lines grep finds (duplicated lines: long equal texts)
    ln = fd.grep([b"the", b"== "])
    a = fd.sort(ln)
    clipped = (ln.start, torch.minimum(ln.end, ln.start + 100), ln.ptr)      # (whole lines without the skip: a round for every seven bytes)
    b, c = fd.sort(clipped), fd.sort(clipped, _skip=False)
    assert _equal(b, c) and b.rounds <= c.rounds <= 16 and a.rounds < 64
    lines, pos = [[], []], 0
    for line in corpus.split(b"\n"):
        for j, p in enumerate((b"the", b"== ")):
            if p in line:
                lines[j].append((pos, pos + len(line)))
        pos += len(line) + 1
    dedup = [sorted(set(x)) for x in lines]                                  # every extent of a Lines once
    assert _as_lists(fd, a) == _host_sort(corpus, dedup) and int(a.distinct[0]) < len(dedup[0])
    one = find.sort_regex(m, rxs[1], dev, unique=True)                       # the one-off form
    assert _as_lists(fd, one) == [[(t, s) for t, s in _as_lists(fd, fd.sort_regex(rxs[1], unique=True))[0]]]
    assert [t for t, _ in _as_lists(fd, one)[0]] == sorted({t for t, _ in _host_sort(corpus, spans[1:])[0]})
    with pytest.raises(ValueError, match="has offsets but no lengths"):
        fd.sort(fd.find([b"the"]))


def test_two_shard_merged_store_and_an_empty_one(dev, stores):
    import torch
    from hmse_amd import find, ingest, manifest
    from hmse_amd.regex import Regex
    cfg, out = stores
    m, fd1, corpus = out["A"]
    d = np.frombuffer(corpus, np.uint8)
    half = 3 * SEG
    rs = ingest.ingest_shards_local([torch.from_numpy(d[:half].copy()).to(dev), torch.from_numpy(d[half:].copy()).to(dev)], cfg)
    st = manifest.Store.from_bytes(manifest.merge_manifests([manifest.build_manifest(r, i, 2) for i, r in enumerate(rs)]).to_bytes())
    assert len(st.shards) == 2
    fd2 = find.StoreFinder(st, dev)
    rx = Regex(WORD, device=dev)
    assert _equal(fd1.sort_regex(rx), fd2.sort_regex(rx)) and _equal(fd1.sort_regex(rx, unique=True), fd2.sort_regex(rx, unique=True))
    assert _equal(fd1.sort(fd1.grep([b"the"])), fd2.sort(fd2.grep([b"the"])))
    s, e = [half - 3, 0, half - 3, half - 2], [half + 3, 6, half + 3, half + 9]
    across = fd2.sort((torch.tensor(s, dtype=torch.int64, device=dev), torch.tensor(e, dtype=torch.int64, device=dev)))
    _same_sorted(across, ref.order(corpus, s, e, [0, 4]))                    # ranges across the shards, two of them the same range
    empty = find.StoreFinder(manifest.Store([]), dev)
    for z, G in ((empty.sort_regex(rx), 1), (empty.sort_regex([rx, rx], unique=True), 2), (empty.sort(empty.grep([b"a", b"bc", b"d"])), 3),
                 (empty.sort(empty.tally_regex([rx, rx])), 2)):
        assert z.ptr.tolist() == [0] * (G + 1) and z.distinct.tolist() == [0] * G == z.total.tolist() and z.rounds == 0
        assert all(getattr(z, f).numel() == 0 and getattr(z, f).device.type == "cuda" for f in ("index", "start", "end", "first", "count", "rank_of"))
        assert empty.text(z)[0].numel() == 0
    z = empty.sort((torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)))      # two empty texts of an empty corpus
    assert (z.index.tolist(), z.first.tolist(), z.distinct.tolist(), z.rank_of.tolist(), z.rounds) == ([0, 1], [True, False], [1], [0, 1], 1)
