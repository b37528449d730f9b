"""GPU: the tally of search results (hmse_amd.find tally / tally_regex; hmse_tally_keys / hmse_tally_same) against the plain-Python
reference of tests/tally_ref.py — the two kernels on synthetic chunk maps (every range of a small corpus under five chunkings, pairs
that differ in one byte at the edges and at the chunk seams, folding of exactly A..Z, bad input), the grouping under keys narrow enough
to collide, on poisoned / misaligned / guarded memory (tests/arena.py), and on stores with POINTER and DELTA records.  All results are
compared bit for bit.  The shapes are the smallest at which the kernels can go wrong."""
import collections
import os
import re

import numpy as np
import pytest

import arena as A_
import lines_ref
import tally_ref as ref
from test_sync_host import SEG, corpora

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc", "tally.hip")).read()
T = int(re.search(r"constexpr uint32_t TALLY_TRIP = (\d+);", _SRC).group(1))             # bytes one trip looks at
FIELDS = ("ptr", "start", "end", "count", "distinct", "total", "value_of")


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


def _u64(t):
    return [v & ((1 << 64) - 1) for v in t.tolist()]


# ---- 1. keys: every range of a small corpus ------------------------------------------------------------------------------------------------
BLOCK = 20                                               # one record placed at three corpus positions


def _keys_corpus():
    rng = np.random.default_rng(1)
    n = 3 * T + 37
    c = rng.integers(0, 256, n, dtype=np.uint8)
    up = rng.random(n) < 0.3
    c[up] = rng.integers(65, 91, int(up.sum()), dtype=np.uint8)                            # enough A..Z for the folding to matter
    for at in (70, 150):
        c[at: at + BLOCK] = c[5: 5 + BLOCK]
    return c.tobytes()


@pytest.fixture(scope="module")
def every_range():
    """-> (corpus, starts, ends, {fold: keys}): the 26 335 non-empty ranges of the corpus and a few empty ones, their reference keys once"""
    corpus = _keys_corpus()
    n = len(corpus)
    assert n == 3 * T + 37 and corpus[5: 5 + BLOCK] == corpus[70: 70 + BLOCK] == corpus[150: 150 + BLOCK]
    pairs = [(s, e) for s in range(n) for e in range(s + 1, n + 1)]
    assert len(pairs) == 26335
    pairs += [(0, 0), (n, n), (T, T), (70, 70)]
    starts, ends = [p[0] for p in pairs], [p[1] for p in pairs]
    want = {f: ref.keys(corpus, starts, ends, f, seed=3) for f in (False, True)}
    assert sum(a != b for a, b in zip(want[False], want[True])) > 20000
    return corpus, starts, ends, want


def _key_chunkings(n):
    rng = np.random.default_rng(5)
    tiny = [0]
    while tiny[-1] < n:
        tiny.append(min(tiny[-1] + int(rng.integers(0, 3)), n))
    edges = sorted({0, n, *(k * T + d for k in range(1, 4) for d in (-1, 0, 1))})
    return {"one": [0, n], "bytes": list(range(n + 1)), "tiny-and-empty": tiny + [n, n], "trip-edges": edges,
            "one-record-three-places": [0, 5, 5 + BLOCK, 70, 70 + BLOCK, 150, 150 + BLOCK, n]}


@pytest.mark.parametrize("name", ["one", "bytes", "tiny-and-empty", "trip-edges", "one-record-three-places"])
def test_keys_of_every_range_of_a_small_corpus(dev, every_range, name):
    import torch
    from hmse_amd import ops
    corpus, starts, ends, want = every_range
    cuts = _key_chunkings(len(corpus))[name]
    assert cuts[0] == 0 and cuts[-1] == len(corpus) and cuts == sorted(cuts)
    if name == "tiny-and-empty":
        assert set(np.diff(cuts).tolist()) == {0, 1, 2}
    if name == "one-record-three-places":
        slot = lines_ref.tables(corpus, cuts)[2]
        assert slot[1] == slot[3] == slot[5]
    tabs = _tables(dev, corpus, cuts)
    s, e = _t(np.asarray(starts, np.int64), dev), _t(np.asarray(ends, np.int64), dev)
    for fold in (False, True):
        key = ops.tally_keys(*tabs, s, e, fold, seed=3)
        assert key.dtype == torch.int64 and key.numel() == len(starts)
        got = _u64(key)
        assert got == want[fold], next((starts[i], ends[i], hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want[fold])) if g != w)
    # another seed and narrow keys: a sample
    idx = list(range(0, len(starts), 97))
    si, ei = s[idx].contiguous(), e[idx].contiguous()
    for seed, bits in ((0, 64), (1 << 63, 64), (7, 8), (7, 1), ((1 << 64) - 1, 63)):
        got = _u64(ops.tally_keys(*tabs, si, ei, True, seed=seed, key_bits=bits))
        assert got == [ref.key(corpus, starts[i], ends[i], True, seed, bits) for i in idx], (seed, bits)


# ---- 2. same ---------------------------------------------------------------------------------------------------------------------------------
def _same_case():
    """Segments of L bytes back to back: 0 = the text (the rep, cut at 30), then copies cut at 70 — 1: equal, 2..7: one byte changed (the
    first, the last, the bytes on either side of the copy's seam and of the rep's seam), 8: equal in 1-byte chunks, 9: equal, uncut."""
    L = 2 * T + 22
    rng = np.random.default_rng(2)
    text = rng.integers(97, 123, L, dtype=np.uint8)
    changed = {2: 0, 3: L - 1, 4: 69, 5: 70, 6: 29, 7: 30}
    segs, cuts = [], [0]
    for k in range(10):
        sgm = text.copy()
        if k in changed:
            sgm[changed[k]] ^= 0x01
        segs.append(sgm.tobytes())
        base = k * L
        inner = [30] if k == 0 else list(range(1, L)) if k == 8 else [] if k == 9 else [70]
        cuts += [base + c for c in inner] + [base + L]
    return b"".join(segs), cuts, L, changed


def test_same_pairs_that_differ_in_one_byte_at_the_edges_and_at_the_seams(dev):
    import torch
    from hmse_amd import ops
    corpus, cuts, L, changed = _same_case()
    tabs = _tables(dev, corpus, cuts)
    cases = [(k * L, (k + 1) * L, 0) for k in range(10)]                     # 0..9: segment k against the rep, segment 0
    cases += [(L, 2 * L - 1, 0), (L, 2 * L + 1, 0)]                          # 10, 11: one byte shorter, one byte longer
    cases += [(0, 0, 13), (5 * L, 5 * L, 12)]                                # 12, 13: two empty texts
    cases += [(2 * L + 1, 3 * L, 15), (L + 1, 2 * L, 14)]                    # 14, 15: segment 2 without its changed first byte, segment 1 without its own
    cases += [(4 * L, 5 * L, 4), (7 * L, 8 * L, 7)]                          # 16, 17: the very range of another index
    cases += [(2 * L, 3 * L, 18)]                                            # 18: rep[i] == i
    starts, ends, rep = ([c[j] for c in cases] for j in range(3))
    want = ref.same(corpus, starts, ends, rep)
    assert want == [1, 1, 0, 0, 0, 0, 0, 0, 1, 1] + [0, 0] + [1, 1] + [1, 1] + [1, 1] + [1]
    i64 = lambda v: _t(np.asarray(v, np.int64), dev)
    for fold in (False, True):
        got = ops.tally_same(*tabs, i64(starts), i64(ends), i64(rep), fold)
        assert got.dtype == torch.uint8 and got.tolist() == want, fold
    # every other order of rep and member: symmetric
    got = ops.tally_same(*tabs, i64(starts[:10]), i64(ends[:10]), i64([9, 8, 1, 0, 3, 4, 7, 6, 5, 2]))
    assert got.tolist() == ref.same(corpus, starts[:10], ends[:10], [9, 8, 1, 0, 3, 4, 7, 6, 5, 2]) == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]


def test_folding_of_exactly_a_to_z(dev):
    from hmse_amd import ops
    upper = bytes(range(65, 91)) + b"@[\xc1\x00_"                             # and five bytes whose | 0x20 form is another byte, no letter
    corpus = upper + bytes(b | 0x20 for b in upper)
    n = len(upper)
    for cuts in ([0, 2 * n], list(range(2 * n + 1)), [0, n, 2 * n]):
        tabs = _tables(dev, corpus, cuts)
        i64 = lambda v: _t(np.asarray(v, np.int64), dev)
        # every byte against its | 0x20 form (and back); the 26 letters as one text and the five others as one, against theirs
        s = list(range(2 * n)) + [0, 26, n, n + 26]
        e = [p + 1 for p in range(2 * n)] + [26, n, n + 26, 2 * n]
        rep = [(p + n) % (2 * n) for p in range(2 * n)] + [2 * n + 2, 2 * n + 3, 2 * n, 2 * n + 1]
        folded = ops.tally_same(*tabs, i64(s), i64(e), i64(rep), True).tolist()
        exact = ops.tally_same(*tabs, i64(s), i64(e), i64(rep), False).tolist()
        assert folded == ref.same(corpus, s, e, rep, True) and exact == ref.same(corpus, s, e, rep, False)
        assert folded[:n] == folded[n: 2 * n] == [1] * 26 + [0] * 5 and folded[2 * n:] == [1, 0, 1, 0] and exact == [0] * len(s)
        kf, ke = _u64(ops.tally_keys(*tabs, i64(s), i64(e), True)), _u64(ops.tally_keys(*tabs, i64(s), i64(e), False))
        assert kf == ref.keys(corpus, s, e, True) and ke == ref.keys(corpus, s, e, False)
        assert [kf[p] == kf[p + n] for p in range(n)] == [True] * 26 + [False] * 5 and len(set(ke)) == len(ke)


# ---- 3. the grouping -------------------------------------------------------------------------------------------------------------------------
def _finder(dev, corpus, cuts):
    """a StoreFinder over a synthetic chunk map (no store behind it): what tally reads"""
    from hmse_amd import find
    fd = find.StoreFinder.__new__(find.StoreFinder)
    fd.dev = dev
    fd.raw, fd.raw_off, fd.cuts, fd.slot = _tables(dev, corpus, cuts)
    fd.n_bytes, fd.n_records = len(corpus), int(fd.raw_off.numel()) - 1
    return fd


def _same_tally(got, want):
    import torch
    for f in FIELDS:
        t = getattr(got, f)
        assert t.dtype == torch.int64 and t.device.type == "cuda" and t.tolist() == want[f], f


@pytest.fixture(scope="module")
def grouped():
    """a corpus of words from a vocabulary of 36 (some differ in case only), 3000 ranges over whole words, three word pairs and empty texts,
    in three groups (one of them empty) -> (corpus, cuts, starts, ends, ptr, {(ic, top): reference})"""
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
    refs = {(ic, top): ref.tally(corpus, starts, ends, ptr, ic, top) for ic in (False, True) for top in (None, 3)}
    assert 40 >= max(refs[False, None]["distinct"]) > max(refs[True, None]["distinct"]) >= 25
    return corpus, cuts, starts, ends, ptr, refs


@pytest.mark.parametrize("key_bits", [1, 2, 8, 64])
def test_tally_is_the_reference_s_whatever_the_keys_width(dev, grouped, key_bits):
    corpus, cuts, starts, ends, ptr, refs = grouped
    fd = _finder(dev, corpus, cuts)
    i64 = lambda v: _t(np.asarray(v, np.int64), dev)
    what = (i64(starts), i64(ends), i64(ptr))
    t = fd.tally(what, ignore_case=True, _key_bits=key_bits)               # at most 40 distinct values per group
    _same_tally(t, refs[True, None])
    assert (t.rounds == 1) if key_bits == 64 else (t.rounds > 1 if key_bits <= 2 else t.rounds >= 1)
    assert int(t.count.sum()) == 3000 and t.total.tolist() == [1700, 0, 1300] and bool((t.value_of >= 0).all())
    cut = fd.tally(what, ignore_case=True, top=3, _key_bits=key_bits)
    _same_tally(cut, refs[True, 3])
    assert cut.ptr.tolist() == [0, 3, 3, 6] and cut.distinct.tolist() == t.distinct.tolist() and int((cut.value_of == -1).sum()) == 3000 - int(cut.count.sum()) > 0
    if key_bits in (1, 64):
        _same_tally(fd.tally(what, _key_bits=key_bits), refs[False, None])
        _same_tally(fd.tally(what, top=3, _key_bits=key_bits), refs[False, 3])
    data, off = fd.text(cut)                                               # text() takes a Tally: the representatives
    want = lines_ref.text(corpus, refs[True, 3]["start"], refs[True, 3]["end"])
    assert data.cpu().numpy().tobytes() == want[0] and off.tolist() == want[1]


def test_tally_of_one_range_of_empty_ranges_and_max_rounds(dev, grouped):
    import torch
    corpus, cuts, starts, ends, ptr, refs = grouped
    fd = _finder(dev, corpus, cuts)
    i64 = lambda v: _t(np.asarray(v, np.int64), dev)
    one = fd.tally((i64([5]), i64([9])))
    _same_tally(one, ref.tally(corpus, [5], [9], [0, 1]))
    assert (one.ptr.tolist(), one.start.tolist(), one.end.tolist(), one.count.tolist(), one.value_of.tolist(), one.rounds) == ([0, 1], [5], [9], [1], [0], 1)
    n = len(corpus)
    s, e, p = [7, 0, n, 3, 7], [7, 0, n, 3, 8], [0, 2, 5]                  # empty texts equal each other, in their own group only
    empties = fd.tally((i64(s), i64(e), i64(p)))
    _same_tally(empties, ref.tally(corpus, s, e, p))
    assert empties.count.tolist() == [2, 2, 1] and empties.start.tolist() == [0, 3, 7] and empties.value_of.tolist() == [0, 0, 1, 1, 2]
    with pytest.raises(RuntimeError, match=r"unresolved after max_rounds = 1 rounds"):
        fd.tally((i64(starts), i64(ends), i64(ptr)), max_rounds=1, _key_bits=1)
    with pytest.raises(ValueError, match="descends or leaves the corpus"):
        fd.tally((i64([0]), i64([n + 1])))
    assert torch.cuda.is_available()


# ---- 4. bad input ----------------------------------------------------------------------------------------------------------------------------
def _raw_calls(dev, raw, raw_off, cuts, slot, starts, ends, rep, sentinel=0x5A):
    """hmse_tally_keys and hmse_tally_same through ctypes on outputs and status words that start as `sentinel`
    -> (keys, keys status, same, same status)."""
    import torch
    from hmse_amd import _lib
    i64 = lambda v: _t(np.asarray(v, np.int64).reshape(-1), dev)
    raw_d, ro, cu, sl, s, e, r = _t(raw, dev), i64(raw_off), i64(cuts), i64(slot), i64(starts), i64(ends), i64(rep)
    n = len(starts)
    key = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    same = torch.full((n + 1,), sentinel, dtype=torch.uint8, device=dev)
    st = torch.full((2,), -1, dtype=torch.int32, device=dev)
    lib, stream = _lib.hip_lib(), torch.cuda.current_stream().cuda_stream
    common = (raw_d.data_ptr(), raw_d.numel(), ro.data_ptr(), len(raw_off) - 1, cu.data_ptr(), sl.data_ptr(), len(slot), s.data_ptr(), e.data_ptr())
    assert lib.hmse_tally_keys(*common, n, 1, 5, 64, key.data_ptr(), st.data_ptr(), stream) == 0
    assert lib.hmse_tally_same(*common, r.data_ptr(), n, 1, same.data_ptr(), st.data_ptr() + 4, stream) == 0
    torch.cuda.synchronize()
    assert key[n].item() == -7 and same[n].item() == sentinel                # nothing behind the end
    return _u64(key[:n]), int(st[0].item()), same[:n].tolist(), int(st[1].item())


def test_refused_calls_set_status_bit_1_and_write_zeros(dev):
    from hmse_amd import ops
    rng = np.random.default_rng(6)
    corpus = rng.integers(65, 123, 300, dtype=np.uint8).tobytes()
    cuts = [0, 100, 100, 250, 300]
    raw, raw_off, slot = lines_ref.tables(corpus, cuts)
    starts, ends, rep = [0, 5, 90, 300], [50, 5, 260, 300], [0, 0, 2, 1]
    good = _raw_calls(dev, raw, raw_off, cuts, slot, starts, ends, rep)
    assert good == (ref.keys(corpus, starts, ends, True, 5), 0, ref.same(corpus, starts, ends, rep, True), 0) and good[2] == [1, 0, 1, 1]
    zeros = ([0] * 4, 2, [0] * 4, 2)
    for s2, e2, r2, which in (([0, 5, 260, 300], [50, 5, 90, 300], rep, "both"),               # a range that descends
                              (starts, [50, 5, 260, 301], rep, "both"),                        # end > N
                              (starts, [50, 5, 260, 1 << 62], rep, "both"),
                              ([-1, 5, 90, 300], [-1, 5, 260, 300], rep, "both"),              # 2^64 - 1
                              (starts, ends, [0, 0, 2, 4], "same"),                            # rep >= n
                              (starts, ends, [0, -1, 2, 1], "same")):
        got = _raw_calls(dev, raw, raw_off, cuts, slot, s2, e2, r2)
        assert got[2:] == zeros[2:] and (got[:2] == zeros[:2] if which == "both" else got[:2] == good[:2]), (s2, e2, r2)
    for bad_cuts, bad_slot, bad_off in (([0, 100, 90, 250, 300], slot, raw_off),               # cuts descend
                                        (cuts, [0, 1, len(raw_off) - 1, 3], raw_off),          # a slot outside the index
                                        ([0, 100, 100, 250, 301], slot, raw_off),              # a chunk longer than its record
                                        ([1, 100, 100, 250, 300], slot, raw_off),              # the corpus does not start at 0
                                        (cuts, slot, raw_off[:-1] + [raw_off[-1] + 50])):      # records beyond raw
        assert _raw_calls(dev, raw, bad_off, bad_cuts, bad_slot, starts, ends, rep) == zeros
        i64 = lambda v: _t(np.asarray(v, np.int64), dev)
        with pytest.raises(ops.HmseError, match="inconsistent tables"):
            ops.tally_keys(_t(raw, dev), i64(bad_off), i64(bad_cuts), i64(bad_slot), i64(starts), i64(ends))
        with pytest.raises(ops.HmseError, match="inconsistent tables"):
            ops.tally_same(_t(raw, dev), i64(bad_off), i64(bad_cuts), i64(bad_slot), i64(starts), i64(ends), i64(rep))
    # no chunks at all: N = 0, only (0, 0) is a range; then the run is still clean
    assert _raw_calls(dev, b"", [0], [0], [], [0, 0], [0, 0], [1, 0]) == ([ref.key(b"", 0, 0, True, 5)] * 2, 0, [1, 1], 0)
    assert _raw_calls(dev, b"", [0], [0], [], [0, 0], [0, 1], [1, 0]) == ([0, 0], 2, [0, 0], 2)
    assert _raw_calls(dev, raw, raw_off, cuts, slot, starts, ends, rep) == good
    tabs = _tables(dev, corpus, cuts)
    e = _t(np.zeros(0, np.int64), dev)
    assert ops.tally_keys(*tabs, e, e).numel() == 0 and ops.tally_same(*tabs, e, e, e).numel() == 0


# ---- 5. arguments only -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["random", "ones", "zero"])
def test_both_calls_on_poisoned_misaligned_guarded_memory(dev, monkeypatch, pattern):
    """Inputs off their alignment between guard bands (the last record ends at raw's guarded end), outputs and status words from poisoned
    memory: every output is fully determined and no guard band is touched."""
    ar = A_.Arena(dev, pattern, seed=11).install(monkeypatch, distrust_zeros=True, byte_misalign=3)
    from hmse_amd import ops
    place = lambda x, side=None: ar.place(x, misalign=5 if side == "raw" else 0)
    rng = np.random.default_rng(7)
    corpus = rng.integers(60, 100, 5 * T + 9, dtype=np.uint8).tobytes()
    n = len(corpus)
    tiny = [0]
    while tiny[-1] < n:
        tiny.append(min(tiny[-1] + int(rng.integers(0, 3)), n))
    for cuts in (tiny, sorted({0, n, *rng.integers(1, n, 12).tolist()}), [0, n]):
        tabs = _tables(dev, corpus, cuts, place)
        s = [0, 3, 17, n, 40, 0, n - 1, 2 * T]
        e = [n, 3, 2 * T + 30, n, 41, 16, n, 4 * T + 1]
        rep = [0, 3, 2, 1, 4, 0, 6, 2]
        i64 = lambda v: place(np.asarray(v, np.int64))
        for fold in (False, True):
            assert _u64(ops.tally_keys(*tabs, i64(s), i64(e), fold, seed=9)) == ref.keys(corpus, s, e, fold, 9)
            assert ops.tally_same(*tabs, i64(s), i64(e), i64(rep), fold).tolist() == ref.same(corpus, s, e, rep, fold)
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


def _counter_tally(corpus, spans_per_group, ic=False, top=None):
    """re.finditer / line slices and collections.Counter -> per group [(text, count, first start)] in the tally's order"""
    out = []
    for spans in spans_per_group:
        texts = [corpus[s:e].lower() if ic else corpus[s:e] for s, e in spans]
        cnt, first = collections.Counter(texts), {}
        for (s, _), t in zip(spans, texts):
            first.setdefault(t, s)                                           # spans ascend: the first seen has the smallest start
        order = sorted(cnt, key=lambda t: (-cnt[t], first[t]))[:top]
        out.append([(t, cnt[t], first[t]) for t in order])
    return out


def _as_lists(fd, t, ic=False):
    data, off = fd.text(t)
    data, off, ptr = data.cpu().numpy().tobytes(), off.tolist(), t.ptr.tolist()
    texts = [data[off[i]: off[i + 1]] for i in range(len(off) - 1)]
    return [[(texts[i].lower() if ic else texts[i], c, s) for i, c, s in zip(range(ptr[j], ptr[j + 1]), t.count[ptr[j]: ptr[j + 1]].tolist(),
                                                                            t.start[ptr[j]: ptr[j + 1]].tolist())] for j in range(len(ptr) - 1)]


WORD, NUM = rb"[A-Za-z]+", rb"[0-9]+|== [A-Za-z ]+ =="


@pytest.mark.parametrize("name", ["A", "B"])
def test_tally_regex_and_tally_of_grepped_lines_on_stores(dev, stores, name):
    from hmse_amd import KIND_DELTA, KIND_POINTER, find
    from hmse_amd.regex import Regex
    cfg, out = stores
    m, fd, corpus = out[name]
    assert (m.chunk_map["kind"] == KIND_DELTA).any() and (m.chunk_map["kind"] == KIND_POINTER).any()
    rxs = [Regex(WORD, device=dev), Regex(NUM, device=dev)]
    spans = [[mt.span() for mt in re.finditer(p, corpus)] for p in (WORD, NUM)]
    assert len(spans[0]) > 10000 and len(spans[1]) > 10
    for ic, top in ((False, None), (True, None), (False, 10), (True, 1)):
        t = fd.tally_regex(rxs, ignore_case=ic, top=top)
        want = _counter_tally(corpus, spans, ic, top)
        assert _as_lists(fd, t, ic) == want and t.rounds == 1
        assert t.total.tolist() == [len(s) for s in spans] and t.distinct.tolist() == [len(w) for w in _counter_tally(corpus, spans, ic)]
        vo = t.value_of.tolist()
        for j, sp in enumerate(spans):                                       # value_of: every occurrence's own text, or -1 where top cut
            base = sum(len(s) for s in spans[:j])
            for i in range(0, len(sp), 101):
                txt = corpus[sp[i][0]: sp[i][1]].lower() if ic else corpus[sp[i][0]: sp[i][1]]
                kept = [w[0] for w in want[j]]
                assert (vo[base + i] == -1 and txt not in kept) or vo[base + i] == int(t.ptr[j]) + kept.index(txt)
    assert want[0][0][1] > 100                                               # (True, 1): the most frequent word
    # duplicated lines: every extent of grep counts once
    ln = fd.grep([b"the", b"== "])
    lines, pos = [[], []], 0
    for line in corpus.split(b"\n"):
        for j, p in enumerate((b"the", b"== ")):
            if p in line:
                lines[j].append((pos, pos + len(line)))
        pos += len(line) + 1
    assert ln.counts.tolist() == [len(x) for x in lines]
    t = fd.tally(ln)
    want = _counter_tally(corpus, lines)
    assert _as_lists(fd, t) == want and want[0][0][1] > 1 and sum(c for _, c, _ in want[0]) == len(lines[0])
    one = find.tally_regex(m, rxs[1], dev, top=2)                            # the one-off form
    assert _as_lists(fd, one) == [_counter_tally(corpus, spans[1:], top=2)[0]]
    with pytest.raises(ValueError, match="has offsets but no lengths"):
        fd.tally(fd.find([b"the"]))


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
    a, b = fd1.tally_regex(rx, top=50), fd2.tally_regex(rx, top=50)
    assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS) and a.start.numel() == 50
    a, b = fd1.tally(fd1.grep([b"the"])), fd2.tally(fd2.grep([b"the"]))
    assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS)
    across = fd2.tally((torch.tensor([half - 3, 0], dtype=torch.int64, device=dev), torch.tensor([half + 3, 6], dtype=torch.int64, device=dev)))
    _same_tally(across, ref.tally(corpus, [half - 3, 0], [half + 3, 6], [0, 2]))    # a range across the shards
    empty = find.StoreFinder(manifest.Store([]), dev)
    for z, G in ((empty.tally_regex(rx), 1), (empty.tally_regex([rx, rx], top=3), 2), (empty.tally(empty.grep([b"a", b"bc", b"d"])), 3)):
        assert z.ptr.tolist() == [0] * (G + 1) and z.distinct.tolist() == [0] * G == z.total.tolist() and z.rounds == 0
        assert all(getattr(z, f).numel() == 0 and getattr(z, f).dtype == torch.int64 and getattr(z, f).device.type == "cuda" for f in ("start", "end", "count", "value_of"))
        assert empty.text(z)[0].numel() == 0
    z = empty.tally((torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)))     # two empty texts of an empty corpus
    assert (z.count.tolist(), z.start.tolist(), z.end.tolist(), z.value_of.tolist()) == ([2], [0], [0], [0, 0])
