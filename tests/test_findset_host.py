"""CPU: the compiled pattern set of hmse_amd.find.PatternSet (include/hmse.h `hmse_findset`) — its layout, its refusals, a numpy
restatement of lookup + verify + partition over the built arrays against tests/find_ref.py (the layout loses nothing, independently of
the kernels), the entry points' own refusals (HMSE_EINVAL in front of every HIP call), and the kernels on the CPU (tools/findset_emu.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import find_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH = 0x9E3779B1


def h32(key):
    return (int(key) * HASH) & 0xFFFFFFFF


def _entries(ps):
    return [ps.upat[ps.uoff[i]: ps.uoff[i + 1]].tobytes() for i in range(ps.n_entries)]


def _word_patterns(rng, n, lo=4, hi=40):
    return [bytes(rng.integers(97, 123, int(rng.integers(lo, hi + 1)), dtype=np.uint8)) for _ in range(n)]


# ---- the layout --------------------------------------------------------------------------------------------------------------------------
def test_every_unique_pattern_is_reachable_through_its_directory_cell():
    from hmse_amd import find, ops
    rng = np.random.default_rng(1)
    pats = _word_patterns(rng, 3000) + [b"sharedprefix" + bytes([97 + i % 26, 97 + i // 26]) for i in range(300)] + [b"ab", b"c", b"xyz"]
    ps = find.PatternSet(pats)
    assert ps.n_patterns == len(pats) and ps.n_unique == len(set(pats)) and ps.n_entries == len({p for p in pats if len(p) >= 4})
    assert (1 << ps.dir_bits) >= 2 * ps.n_entries and ps.dir.size == (1 << ps.dir_bits) + 1
    assert ps.dir[0] == 0 and ps.dir[-1] == ps.n_entries and (np.diff(ps.dir.astype(np.int64)) >= 0).all()   # ascending, covers all of ukey
    assert ps.bitmap.size == 1 << (ops.FINDSET_BITMAP_BITS - 5) and ps.max_len == max(len(p) for p in pats)
    ents = _entries(ps)
    keys = []
    for i, e in enumerate(ents):
        key = int.from_bytes(e[:4], "little")
        assert 4 <= len(e) <= 256 and key == int(ps.ukey[i]) and ps.unique[ps.uid[i]] == e
        cell, bit = h32(key) >> (32 - ps.dir_bits), h32(key) >> 13
        assert ps.dir[cell] <= i < ps.dir[cell + 1]
        assert (int(ps.bitmap[bit >> 5]) >> (bit & 31)) & 1
        keys.append((h32(key), key, len(e), e))
    assert keys == sorted(keys) and len(set(ents)) == len(ents)
    assert sorted(ps.uid.tolist() + ps.short_ids.tolist()) == list(range(ps.n_unique))               # every unique pattern is somewhere
    assert [ps.unique[u] for u in ps.short_ids] == ps.short_patterns and set(ps.short_patterns) == {b"ab", b"c", b"xyz"}
    # no bit in the bitmap that no key set
    want = np.zeros_like(ps.bitmap)
    for hk, *_ in keys:
        want[(hk >> 13) >> 5] |= np.uint32(1 << ((hk >> 13) & 31))
    assert (want == ps.bitmap).all()


def test_duplicates_and_case_equal_patterns_collapse_and_expand_back():
    from hmse_amd import find
    pats = [b"Hello", b"hello", b"HELLO", b"Hello", b"he", b"HE", b"world", b"\xc1bcd", b"\xe1bcd", b"[ABC", b"{abc", b"[abc"]
    exact = find.PatternSet(pats)
    assert exact.n_patterns == 12 and exact.n_unique == 11 and exact.index.tolist() == [0, 1, 2, 0, 3, 4, 5, 6, 7, 8, 9, 10]
    fold = find.PatternSet(pats, ignore_case=True)
    assert fold.n_unique == 7 and fold.index.tolist() == [0, 0, 0, 0, 1, 1, 2, 3, 4, 5, 6, 5]
    assert fold.unique == [b"hello", b"he", b"world", b"\xc1bcd", b"\xe1bcd", b"[abc", b"{abc"]       # only A-Z fold
    assert [fold.unique[u] for u in fold.index] == [p.lower() for p in pats]
    assert fold.n_entries == 6 and fold.short_patterns == [b"he"]
    many = find.PatternSet([b"same-pattern"] * 50 + [b"other"])
    assert many.n_patterns == 51 and many.n_unique == 2 and many.n_entries == 2 and many.index.tolist() == [0] * 50 + [1]
    empty = find.PatternSet([])
    assert empty.n_patterns == 0 and empty.n_unique == 0 and empty.n_entries == 0 and empty.resident_bytes == 0 and empty.dir.tolist() == [0, 0, 0]
    assert exact.resident_bytes == 0 and exact.set is None                                            # device=None keeps the numpy arrays


def test_the_build_is_deterministic():
    from hmse_amd import find
    rng = np.random.default_rng(2)
    pats = _word_patterns(rng, 2000, 1, 30)
    pats += pats[:100]
    a, b = find.PatternSet(pats, ignore_case=True), find.PatternSet(list(pats), ignore_case=True)
    for f in ("upat", "uoff", "ukey", "uid", "dir", "bitmap", "index", "short_ids"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f
    assert a.short_patterns == b.short_patterns and (a.dir_bits, a.max_len, a.n_unique) == (b.dir_bits, b.max_len, b.n_unique)


def test_pattern_set_refuses_what_pack_patterns_refuses_and_too_many(monkeypatch):
    from hmse_amd import find
    for bad in (["ab"], [b""], [b"x" * 257], [b"ok", "no"], [np.zeros(3, np.int32)], [np.zeros((2, 2), np.uint8)], [17], b"ab", "ab"):
        with pytest.raises(ValueError) as e1:
            find.pack_patterns(bad)
        with pytest.raises(ValueError) as e2:
            find.PatternSet(bad)
        assert str(e1.value) == str(e2.value)
    ok = find.PatternSet([b"ab", bytearray(b"cdef"), memoryview(b"ghijk"), np.frombuffer(b"lmnopq", np.uint8)])
    assert ok.unique == [b"ab", b"cdef", b"ghijk", b"lmnopq"]
    assert find.HMSE_FINDSET_MAX_PATTERNS == 1 << 20
    monkeypatch.setattr(find, "HMSE_FINDSET_MAX_PATTERNS", 100)                                       # (2^20 patterns take seconds to build)
    pats = [b"p%04d" % i for i in range(101)]
    with pytest.raises(ValueError, match=r"\b101 distinct patterns.*100\b"):
        find.PatternSet(pats)
    assert find.PatternSet(pats[:100] + pats[:50]).n_unique == 100                                    # distinct ones count, not the list
    assert find.PatternSet([p.upper() for p in pats[:60]] + pats[:100], ignore_case=True).n_unique == 100    # ... after folding


# ---- the layout loses nothing: lookup + verify + partition in numpy --------------------------------------------------------------------
def _lookup(ps, text, p, end):
    """Entries of the set matching text at p and ending at or before `end`: bitmap, directory cell, key walk, verify."""
    if p + 4 > end:
        return []
    key = int.from_bytes(text[p: p + 4], "little")
    hk = h32(key)
    if not (int(ps.bitmap[(hk >> 13) >> 5]) >> ((hk >> 13) & 31)) & 1:
        return []
    cell = hk >> (32 - ps.dir_bits)
    out = []
    for i in range(int(ps.dir[cell]), int(ps.dir[cell + 1])):
        if int(ps.ukey[i]) == key:
            a, e = int(ps.uoff[i]), int(ps.uoff[i + 1])
            if p + (e - a) <= end and text[p: p + e - a] == ps.upat[a:e].tobytes():
                out.append(int(ps.uid[i]))
    return out


def _host_split(ps, corpus, cuts):
    """(in-record, seam) hits as (offset, caller's pattern) through the set's arrays; the 1..3-byte patterns by plain comparison."""
    text = corpus.lower() if ps.ignore_case else corpus
    n = len(text)
    users = {}
    for j, u in enumerate(ps.index.tolist()):
        users.setdefault(u, []).append(j)
    inr, seam = [], []
    for k in range(len(cuts) - 1):
        for o in range(cuts[k], cuts[k + 1]):
            ids = _lookup(ps, text, o, n) + [int(u) for u, s in zip(ps.short_ids, ps.short_patterns) if text[o: o + len(s)] == s]
            for u in ids:
                for j in users[u]:
                    (inr if o + len(ps.unique[u]) <= cuts[k + 1] else seam).append((o, j))
    return sorted(inr), sorted(seam)


@pytest.mark.parametrize("ic", [False, True])
def test_host_lookup_over_the_built_arrays_equals_the_reference(ic):
    from hmse_amd import find
    rng = np.random.default_rng(5 + ic)
    seen_seam = seen_hits = 0
    for _ in range(40):
        n = int(rng.integers(0, 300))
        alpha = np.frombuffer(b"abAB\xc1\xe1[{" if ic else b"abc", np.uint8)
        corpus = bytes(alpha[rng.integers(0, len(alpha), n)])
        lens = []
        while sum(lens) < n:
            lens.append(int(rng.choice([0, 1, 2, 1, 2, 7, 30])))
        if lens:
            lens[-1] -= sum(lens) - n
        lens += [0] * int(rng.integers(0, 3))
        cuts = [0] + [int(c) for c in np.cumsum(lens)] if lens else [0]
        pats = []
        for _ in range(int(rng.integers(1, 40))):
            m = int(rng.choice([1, 2, 3, 4, 5, 6, 9, 17]))
            if n >= m and rng.random() < 0.7:
                o = int(rng.integers(0, n - m + 1))
                p = corpus[o: o + m]
            else:
                p = bytes(alpha[rng.integers(0, len(alpha), m)])
            pats.append(p.swapcase() if ic and rng.random() < 0.5 else p)
        pats += pats[:3]
        ps = find.PatternSet(pats, ignore_case=ic)
        inr, seam = _host_split(ps, corpus, cuts)
        assert (inr, seam) == ref.split(corpus, pats, cuts, ic)
        want = ref.find(corpus, pats, ic)
        everything = sorted(inr + seam)
        assert [o for q in range(len(pats)) for o, j in everything if j == q] == want[2]
        seen_seam += len(seam); seen_hits += len(inr)
    assert seen_seam > 200 and seen_hits > 1000


# ---- the entry points' own refusals come before any HIP call -----------------------------------------------------------------------------
def test_entry_points_refuse_null_arrays_bad_headers_and_flags_with_no_gpu_present():
    """HMSE_EINVAL (-1), never HMSE_EHIP (-3), before anything is cleared or launched.  (The pointers are host addresses; nothing may
    touch them.)"""
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr()
    size = C.sizeof(_lib.HmseFindset)

    def hdr(**kw):
        f = dict(struct_size=size, flags=0, n_entries=2, n_ids=2, dir_bits=2, max_len=8, pat_bytes=12, upat=b, uoff=b, ukey=b, uid=b, dir=b, bitmap=b)
        f.update(kw)
        return _lib.HmseFindset(*[f[n] for n, _ in _lib.HmseFindset._fields_])

    def calls(h, flags=0, **kw):
        a = dict(raw=b, raw_bytes=100, raw_off=b, cuts=b, slot=b, n_hits=b, counts=b, status=b)
        a.update(kw)
        hp = C.byref(h) if h is not None else None
        return (lib.hmse_findset_scan(a["raw"], a["raw_bytes"], a["raw_off"], 1, None, hp, flags, b, 4, a["n_hits"], a["counts"], a["status"], None),
                lib.hmse_findset_seams(a["raw"], a["raw_bytes"], a["raw_off"], 1, a["cuts"], a["slot"], 1, hp, flags, b, 4, a["n_hits"], a["counts"],
                                       a["status"], None))

    bad_headers = [dict(struct_size=size - 8), dict(flags=2), dict(flags=1), dict(n_entries=(1 << 20) + 1, pat_bytes=8 << 20), dict(n_ids=(1 << 20) + 1),
                   dict(n_ids=0), dict(dir_bits=0), dict(dir_bits=22), dict(max_len=3), dict(max_len=257), dict(pat_bytes=7), dict(pat_bytes=513),
                   dict(upat=None), dict(uoff=None), dict(ukey=None), dict(uid=None), dict(dir=None), dict(bitmap=None)]
    for kw in bad_headers:
        assert calls(hdr(**kw)) == (-1, -1), kw
    assert calls(None) == (-1, -1)
    for flags in (2, 0x80000000, 1):                                                                   # unknown bits; a folded call of an exact set
        assert calls(hdr(), flags) == (-1, -1), flags
    for kw in (dict(n_hits=None), dict(status=None), dict(counts=None), dict(raw_bytes=1 << 40)):
        assert calls(hdr(), **kw) == (-1, -1), kw
    assert calls(hdr(), raw_off=None) == (-1, -1) and calls(hdr(), raw=None) == (-1, -1)
    assert calls(hdr(), cuts=None)[1] == -1 and calls(hdr(), slot=None)[1] == -1
    assert lib.hmse_findset_place(b, 1, b, 1, b, b, 1, b, b, 4, None, None) == -1                      # status missing
    assert lib.hmse_findset_place(None, 1, b, 1, b, b, 1, b, b, 4, b, None) == -1                      # hits missing
    assert lib.hmse_findset_place(b, 1, b, 1, b, b, 1, None, b, 4, b, None) == -1                      # chunk_out missing
    assert lib.hmse_findset_place(b, 1, b, 1, b, b, 1, b, None, 4, b, None) == -1                      # out missing
    assert mem.sum().item() == 0


def test_wrappers_refuse_host_tensors_and_sets_that_do_not_match_their_header():
    from hmse_amd import find, ops
    ps = find.PatternSet([b"abcd", b"efghi"])
    t = lambda a: torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else a.dtype).copy())
    fs = ops.FindSet(t(ps.upat), t(ps.uoff), t(ps.ukey), t(ps.uid), t(ps.dir), t(ps.bitmap), ps.n_unique, ps.dir_bits, ps.max_len, False)
    raw, off = torch.zeros(16, dtype=torch.uint8), torch.tensor([0, 16])
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.findset_scan(raw, off, None, fs)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.findset_seams(raw, off, off, torch.tensor([0]), fs)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.findset_place(torch.zeros(1, dtype=torch.int64), off, off, torch.tensor([0]), torch.tensor([0, 1]), 1)


def test_every_pointer_the_findset_wrappers_hand_to_the_library_comes_from_the_arena(monkeypatch):
    """hmse_findset_* replaced by recorders of their arguments (tests/arena.py: RecordingLib)."""
    import arena as A
    from hmse_amd import _lib, find, ops
    lib = A.record(monkeypatch, ("hmse_findset_scan", "hmse_findset_seams", "hmse_findset_place"))
    ar = A.Arena(torch.device("cpu"), "random", seed=5).install(monkeypatch)
    p = ar.place
    i64 = lambda *v: p(np.array(v, np.int64))
    i32 = lambda a: p(a.view(np.int32).copy())
    ps = find.PatternSet([b"abcd", b"efghij", b"abcdef"], True)
    fs = ops.FindSet(p(ps.upat.copy(), misalign=1), i32(ps.uoff), i32(ps.ukey), i32(ps.uid), i32(ps.dir), i32(ps.bitmap), ps.n_unique, ps.dir_bits,
                     ps.max_len, True)
    raw = p(np.arange(100, dtype=np.uint8), misalign=3)
    raw_off, cuts, slot = i64(0, 40, 100), i64(0, 40, 100, 140), i64(0, 1, 0)
    calls = {"findset_scan": lambda: ops.findset_scan(raw, raw_off, p(np.array([2, 1], np.int32)), fs),
             "findset_scan count only": lambda: ops.findset_scan(raw, raw_off, None, fs, hits_cap=0),
             "findset_seams": lambda: ops.findset_seams(raw, raw_off, cuts, slot, fs, hits_cap=8),
             "findset_place": lambda: ops.findset_place(i64(5 << 24, 50 << 24), raw_off, cuts, slot, i64(0, 1, 2, 3), 3)}
    for name, fn in calls.items():
        n_call = len(lib.calls)
        fn()
        made = lib.calls[n_call:]
        assert made, name
        for call, ptrs, args in made:
            assert ptrs and all(ar.contains(q) for q in ptrs), (name, [hex(q) for q in ptrs if not ar.contains(q)])
            if call != "hmse_findset_place":                                         # the header: a host struct naming arena memory only
                hdr = [a for a in args if not isinstance(a, int) and a is not None][0]._obj
                assert (hdr.struct_size, hdr.flags, hdr.n_entries, hdr.n_ids, hdr.dir_bits, hdr.max_len) == (C.sizeof(_lib.HmseFindset), 1, 3, 3, ps.dir_bits, 6)
                assert hdr.pat_bytes == 16 and all(ar.contains(getattr(hdr, f)) for f in ("upat", "uoff", "ukey", "uid", "dir", "bitmap"))
                assert args[[t for t in getattr(lib._real, call).argtypes].index(C.c_uint32)] == 1          # the call's flags are the set's
    assert not [k for k, _ in ar.requests if k != "buf"]                             # no workspace anywhere
    ar.check()


# ---- the kernels on the CPU --------------------------------------------------------------------------------------------------------------
def test_the_emulator_builds_and_its_cases_pass():
    """tools/findset_emu.py: the kernels cut out of findset.hip, one std::thread per lane, against brute force (no sanitizer here)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "findset_emu.py"), "--iters", "6", "--seed", "4242"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "6 cases ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
