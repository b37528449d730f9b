"""CPU: the reference of the exact search (tests/find_ref.py) against hand-written cases, the partition rule (in-record hits of the
unique records laid out at every chunk + seam hits == every occurrence, once) on random corpora with chunks of 0, 1 and 2 bytes, the
argument validation of hmse_amd.find, and the wrappers ops.find_*: no host tensors, every buffer from ops._buf / ops._ws, and the
entry points' own refusals (HMSE_EINVAL) in front of every HIP call.  None of hmse_find_* takes a workspace, so there is no
misaligned-workspace refusal to check."""
import ctypes as C

import numpy as np
import pytest
import torch

import arena as A
import find_ref as ref

CPU = torch.device("cpu")
DEVICE_CALLS = ("hmse_find_scan", "hmse_find_seams", "hmse_find_place")


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_reference_on_hand_written_cases():
    assert ref.occurrences(b"aaaa", b"aa") == [0, 1, 2]                          # overlapping occurrences all count
    assert ref.occurrences(b"abcabc", b"abc") == [0, 3] and ref.occurrences(b"abcabc", b"c") == [2, 5]
    assert ref.occurrences(b"abc", b"abcd") == [] and ref.occurrences(b"", b"a") == []
    assert ref.occurrences(b"xAbCx", b"abc") == [] and ref.occurrences(b"xAbCx", b"aBc", ignore_case=True) == [1]
    assert ref.occurrences(b"\xc1\xe1", b"\xe1", ignore_case=True) == [1]          # 0xC1 / 0xE1 are not a letter and its capital
    assert ref.occurrences(b"[{", b"{", ignore_case=True) == [1]                   # neither are the neighbours of the letters
    assert ref.find(b"abab", [b"ab", b"b", b"ab", b"zz"]) == ([2, 2, 2, 0], [0, 2, 4, 6, 6], [0, 2, 1, 3, 0, 2])   # equal patterns: each answered
    assert ref.find(b"abab", []) == ([], [0], [])
    # the partition rule by hand: cuts 0 | 3 | 3 | 4 | 8, "abcdabcd"
    inr, seam = ref.split(b"abcdabcd", [b"cd", b"abcd", b"d"], [0, 3, 3, 4, 8])
    assert inr == [(3, 2), (4, 1), (6, 0), (7, 2)] and seam == [(0, 1), (2, 0)]
    hits, counts = ref.scan_hits(b"abcdab", [0, 2, 2, 4, 6], [b"ab", b"abcd", b"b"], mult=[3, 9, 0, 2])
    assert hits == [(0, 0), (1, 2), (4, 0), (5, 2)] and counts == [5, 0, 5]     # "ab" | "cd": abcd across records is no hit


def _random_case(rng):
    n = int(rng.integers(0, 200))
    corpus = bytes(rng.integers(97, 100, n, dtype=np.uint8))                      # three letters: many occurrences
    lens = []
    while sum(lens) < n:
        lens.append(int(rng.choice([0, 1, 2, 1, 2, 7, 30])))
    if lens:
        lens[-1] -= sum(lens) - n
    lens += [0] * int(rng.integers(0, 3))                                         # empty chunks at the end, too
    cuts = [0] + list(np.cumsum(lens)) if lens else [0]
    return corpus, [int(c) for c in cuts]


def test_partition_rule_against_the_plain_loop():
    """300 random corpora with tiny and empty chunks: scanning the UNIQUE chunks once (scan_hits over the records), laying every hit
    out at every chunk that maps to its record (what hmse_find_place does) and adding the seam hits gives every occurrence exactly once."""
    rng = np.random.default_rng(7)
    seen_seam = seen_dup = 0
    for _ in range(300):
        corpus, cuts = _random_case(rng)
        m = int(rng.choice([1, 2, 3, 5, 9]))
        pats = [bytes(rng.integers(97, 100, m, dtype=np.uint8)), bytes(rng.integers(97, 100, int(rng.integers(1, 4)), dtype=np.uint8))]
        if len(corpus) >= m and rng.random() < 0.7:
            o = int(rng.integers(0, len(corpus) - m + 1))
            pats[0] = corpus[o: o + m]
        chunks = [corpus[cuts[k]: cuts[k + 1]] for k in range(len(cuts) - 1)]
        recs = sorted(set(chunks))                                                # exact dedupe: one record per distinct chunk
        slot = [recs.index(c) for c in chunks]
        raw_off = [0] + list(np.cumsum([len(r) for r in recs])) if recs else [0]
        mult = [slot.count(r) for r in range(len(recs))]
        hits, counts = ref.scan_hits(b"".join(recs), raw_off, pats, mult=mult)
        placed = sorted((cuts[k] + p - raw_off[slot[k]], j) for k in range(len(chunks)) for p, j in hits
                        if raw_off[slot[k]] <= p < raw_off[slot[k] + 1])
        inr, seam = ref.split(corpus, pats, cuts)
        assert placed == inr
        assert counts == [sum(1 for _, j in inr if j == q) for q in range(len(pats))]
        everything = sorted(inr + seam)
        assert len(set(everything)) == len(everything)
        want = ref.find(corpus, pats)
        assert [o for q in range(len(pats)) for o, j in everything if j == q] == want[2]
        seen_seam += len(seam); seen_dup += len(chunks) - len(recs)
    assert seen_seam > 300 and seen_dup > 300


# ---- hmse_amd.find: arguments ------------------------------------------------------------------------------------------------------------
def test_patterns_are_validated_without_a_gpu():
    from hmse_amd import find
    flat, off = find.pack_patterns([b"ab", bytearray(b"c"), memoryview(b"def"), np.frombuffer(b"gh", np.uint8)])
    assert flat.tobytes() == b"abcdefgh" and off == [0, 2, 3, 6, 8] and flat.dtype == np.uint8
    assert find.pack_patterns([])[1] == [0]
    assert find.pack_patterns([b"x" * 256])[1] == [0, 256]
    for bad in (["ab"], [b""], [b"x" * 257], [b"ok", "no"], [np.zeros(3, np.int32)], [np.zeros((2, 2), np.uint8)], [17], b"ab", "ab"):
        with pytest.raises(ValueError):
            find.pack_patterns(bad)
    assert find.GROUP == 32 and find.MAX_PATTERN_LEN == 256


def test_wrappers_refuse_host_tensors():
    from hmse_amd import ops
    raw = torch.zeros(16, dtype=torch.uint8)
    off = torch.tensor([0, 16])
    pat = torch.zeros(2, dtype=torch.uint8)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.find_scan(raw, off, None, pat, [0, 2])
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.find_seams(raw, off, off, torch.tensor([0]), pat, [0, 2])
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.find_place(torch.zeros(1, dtype=torch.int64), off, off, torch.tensor([0]), torch.tensor([0, 1]), 1)


# ---- the wrappers allocate through _ws / _buf only ---------------------------------------------------------------------------------------
def test_every_pointer_the_find_wrappers_hand_to_the_library_comes_from_the_arena(monkeypatch):
    """hmse_find_* replaced by recorders of their arguments (tests/arena.py: RecordingLib)."""
    from hmse_amd import ops
    lib = A.record(monkeypatch, DEVICE_CALLS, banned=("empty", "zeros", "empty_like", "empty_strided", "full", "zeros_like"))
    ar = A.Arena(CPU, "random", seed=5).install(monkeypatch)
    p = ar.place
    i64 = lambda *v: p(np.array(v, np.int64))
    raw = p(np.arange(100, dtype=np.uint8), misalign=3)
    pat = p(np.frombuffer(b"abcd", np.uint8).copy(), misalign=1)
    raw_off, cuts, slot = i64(0, 40, 100), i64(0, 40, 100, 140), i64(0, 1, 0)
    calls = {
        "find_scan": (lambda: ops.find_scan(raw, raw_off, p(np.array([2, 1], np.int32)), pat, [0, 1, 4]), 3),
        "find_scan count only": (lambda: ops.find_scan(raw, raw_off, None, pat, [0, 4], ignore_case=True, hits_cap=0), 3),
        "find_scan list": (lambda: ops.find_scan(raw, raw_off, None, pat, [0, 4], hits_cap=16), 3),
        "find_seams": (lambda: ops.find_seams(raw, raw_off, cuts, slot, pat, [0, 2, 4], hits_cap=8), 3),
        "find_place": (lambda: ops.find_place(i64(5 << 8, 50 << 8), raw_off, cuts, slot, i64(0, 1, 2, 3), 3), 2),
    }
    for name, (fn, least) in calls.items():
        n_req, n_call = len(ar.requests), len(lib.calls)
        fn()
        made = lib.calls[n_call:]
        assert made and all(c[0] in DEVICE_CALLS for c in made), name
        for call, _, args in made:
            host = [a for a, t in zip(args, getattr(lib._real, call).argtypes) if t is not C.c_void_p and not isinstance(a, int)]
            assert all(isinstance(h, C.Array) for h in host), (name, host)           # the patterns' bounds: a host array
        ptrs = [q for _, ps, _ in made for q in ps]
        assert ptrs and all(ar.contains(q) for q in ptrs), (name, [hex(q) for q in ptrs if not ar.contains(q)])
        assert len(ar.requests) - n_req >= least, (name, len(ar.requests) - n_req)
        assert not [k for k, _ in ar.requests[n_req:] if k != "buf"]                # no workspace anywhere
    ar.check()


# ---- the entry points' own refusals come before any HIP call -----------------------------------------------------------------------------
def test_entry_points_refuse_bad_patterns_and_flags_with_no_gpu_present():
    """HMSE_EINVAL (-1), never HMSE_EHIP (-3): n_pat of 0 or above 32, a pattern length of 0 or above 256 and unknown flag bits are
    refused in front of every clear and launch.  (The pointers are host addresses; nothing may touch them.)"""
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr()
    arr = lambda *v: (C.c_uint32 * len(v))(*v)
    cases = [(arr(0), 0, 0), (arr(*range(34)), 33, 0), (arr(0, 0), 1, 0), (arr(0, 3, 3), 2, 0), (arr(0, 257), 1, 0), (arr(5, 2), 1, 0),
             (arr(0, 4), 1, 2), (arr(0, 4), 1, 0x80000000), (None, 1, 0)]
    for off, n_pat, flags in cases:
        assert lib.hmse_find_scan(b, 100, b, 1, None, b, off, n_pat, flags, b, 4, b, b, b, None) == -1, (n_pat, flags)
        assert lib.hmse_find_seams(b, 100, b, 1, b, b, 1, b, off, n_pat, flags, b, 4, b, b, b, None) == -1, (n_pat, flags)
    assert lib.hmse_find_scan(b, 100, b, 1, None, b, arr(0, 4), 1, 0, b, 4, None, b, b, None) == -1      # n_hits missing
    assert lib.hmse_find_place(b, 1, b, 1, b, b, 1, b, b, 4, None, None) == -1                          # status missing
    assert mem.sum().item() == 0
