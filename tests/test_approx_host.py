"""CPU: the oracle of the approximate search (tests/approx_ref.py) against brute force, the window fact and the partition rule the
kernels rest on, k = 0 against the exact search, the entry points' own refusals (HMSE_EINVAL in front of every HIP call), the wrappers'
pointers, best_ends, find_approx's argument refusals, and the kernels on the CPU (tools/approx_emu.py).

Every randomised case plants noisy copies of its patterns (0 .. k + 1 random edits each) and asserts that the oracle finds at least one
occurrence of every pattern with k >= 1: a test that compares empty lists shows nothing."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import approx_ref as ref
import find_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = b"abcAB\n"


def case(rng, n, n_pat, max_m=9, copies=3):
    """-> (corpus with noisy copies planted, patterns, ks)"""
    pats = [bytes(np.frombuffer(ALPHA, np.uint8)[rng.integers(0, 4, int(rng.integers(1, max_m + 1)))]) for _ in range(n_pat)]
    ks = [int(rng.integers(0, min(len(p) - 1, 3) + 1)) for p in pats]
    corpus = bytearray(np.frombuffer(ALPHA, np.uint8)[rng.integers(0, len(ALPHA), n)].tobytes())
    return bytes(ref.plant(rng, corpus, pats, ks, ALPHA, copies)), pats, ks


def chunking(rng, n, W):
    lens = []
    while sum(lens) < n:
        lens.append(int(rng.choice([0, 1, 2, 1, 1, W - 1, W, W + 1, 2 * W + 3, 40])))
    if lens:
        lens[-1] -= sum(lens) - n
    lens += [0] * int(rng.integers(0, 3))
    return [0] + [int(c) for c in np.cumsum(lens)]


def tables(corpus, cuts):
    recs, slot = [], []
    for k in range(len(cuts) - 1):
        c = corpus[cuts[k]: cuts[k + 1]]
        if c not in recs:
            recs.append(c)
        slot.append(recs.index(c))
    return b"".join(recs), [0] + [int(v) for v in np.cumsum([len(x) for x in recs])], slot


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
def test_the_oracle_equals_brute_force_on_small_inputs():
    rng = np.random.default_rng(3)
    seen = 0
    for trial in range(60):
        corpus, pats, ks = case(rng, int(rng.integers(20, 41)), 2, max_m=6, copies=1)
        for p, k in zip(pats, ks):
            ic = bool(trial & 1)
            fp, fc = ref.fold(p, ic), ref.fold(corpus, ic)
            brute = [min(ref.ed(fp, fc[s:e]) for s in range(e + 1)) for e in range(1, len(corpus) + 1)]
            assert ref.distances(fp, fc) == brute
            got = ref.find(corpus, p, k, ic)
            assert got == [(e - 1, d) for e, d in enumerate(brute, 1) if d <= k]
            assert got or k == 0, (corpus, p, k)
            seen += len(got)
            for o, d in got[:4]:                                                      # the span: the largest start whose text has d errors
                s = ref.span(corpus, p, o, d, ic)
                assert s == max(s for s in range(o + 2) if ref.ed(fp, fc[s: o + 1]) == d) and len(p) - d <= o + 1 - s <= len(p) + d
    assert seen > 300
    assert ref.ed(b"kitten", b"sitting") == 3 and ref.find(b"xxabcxx", b"abc", 0) == [(4, 0)] and ref.find(b"ABC", b"abc", 0, True) == [(2, 0)]
    assert ref.find(b"\xc1bc", b"\xe1bc", 0, True) == [] and ref.span(b"xabc", b"abc", 3, 2) == 3 and ref.span(b"xabc", b"abc", 3, 0) == 1


def test_a_fresh_column_w_bytes_in_front_gives_the_same_thresholded_answer():
    """The window fact: start the column fresh (D[i] = i) at e - W or anywhere in front of it, with arbitrary junk in between — the
    value at e is d(e) whenever that is <= k, and above k otherwise."""
    rng = np.random.default_rng(9)
    seen = 0
    for trial in range(120):
        corpus, pats, ks = case(rng, int(rng.integers(60, 200)), 2)
        for p, k in zip(pats, ks):
            W = len(p) + k
            true = ref.distances(p, corpus)
            assert any(d <= k for d in true) or k == 0
            for e in range(1, len(corpus) + 1):
                extra = int(rng.integers(0, 4))
                junk = bytes(np.frombuffer(ALPHA, np.uint8)[rng.integers(0, len(ALPHA), extra)].tobytes())
                window = junk + corpus[max(e - W, 0): e]                               # junk INSTEAD of what lies in front of the window
                got = ref.distances(p, window)[-1]
                if e >= W:
                    assert (got == true[e - 1]) if true[e - 1] <= k else got > k, (corpus, p, k, e)
                    seen += true[e - 1] <= k
    assert seen > 500


def test_the_oracle_s_numpy_forms_equal_its_plain_loops():
    """find_np (blocks stepped side by side, each from a fresh column W bytes in front: the window fact at work) and spans_np are what
    the GPU tests use on long texts; here they equal find and span, with blocks far smaller than the texts."""
    rng = np.random.default_rng(12)
    seen = 0
    for trial in range(40):
        corpus, pats, ks = case(rng, int(rng.integers(60, 400)), 2)
        for p, k in zip(pats, ks):
            ic = bool(trial & 1)
            want = ref.find(corpus, p, k, ic)
            for block in (1, 7, 64, 1024):
                assert ref.find_np(corpus, p, k, ic, block) == want
            assert want or k == 0
            occ = want[:40] + [(len(corpus) - 1, 0), (0, 1)]
            got = ref.spans_np(corpus, p, occ, ic)
            for (o, d), g in zip(occ, got):
                s = ref.span(corpus, p, o, d, ic)
                assert g == (o + 1 if s is None else s)
            seen += len(want)
    assert seen > 1000 and ref.find_np(b"", b"ab", 1) == [] and ref.spans_np(b"abc", b"abc", []) == []


def test_k_0_is_the_exact_search_shifted_to_the_last_byte():
    rng = np.random.default_rng(4)
    seen = 0
    for trial in range(50):
        corpus, pats, _ = case(rng, 300, 3, max_m=5)
        for ic in (False, True):
            for p in pats:
                got = ref.find(corpus, p, 0, ic)
                assert got == [(o + len(p) - 1, 0) for o in find_ref.occurrences(corpus, p, ic)] and got
                seen += len(got)
    assert seen > 1000


def test_scan_ends_placed_plus_seam_ends_are_every_occurrence_once():
    rng = np.random.default_rng(5)
    seen_scan = seen_seam = 0
    for trial in range(150):
        corpus, pats, ks = case(rng, int(rng.integers(27, 300)), 1)
        p, k = pats[0], ks[0]
        W = len(p) + k
        cuts = chunking(rng, len(corpus), W) if trial % 5 else [0] + list(range(1, len(corpus) + 1))   # (every fifth: a chain of 1-byte chunks)
        raw, raw_off, slot = tables(corpus, cuts)
        words, counts = ref.scan_hits(raw, raw_off, [p], [k])
        rec_of = lambda w: max(r for r in range(len(raw_off) - 1) if raw_off[r] <= (w >> 8) < raw_off[r + 1])
        placed = sorted((cuts[c] + (w >> 8) - raw_off[s], (w >> 3) & 31) for c, s in enumerate(slot) for w in words if rec_of(w) == s)
        # the seam ends: walked from max(cuts[c] + 1 - W, 0) on, through whatever chunks lie there
        seams = []
        for c in range(len(cuts) - 1):
            s0 = max(cuts[c] + 1 - W, 0)
            d = ref.distances(p, corpus[s0: min(cuts[c + 1], cuts[c] + W - 1)])
            assert len(d) <= max(2 * W - 2, 0)
            seams += [(s0 + i, v) for i, v in enumerate(d) if s0 + i >= cuts[c] and v <= k]
        want = ref.find(corpus, p, k)
        assert sorted(placed + seams) == want and len(set(placed + seams)) == len(want)
        assert (placed, sorted(seams)) == ref.split(want, W, cuts)
        assert want or k == 0
        seen_scan += len(placed)
        seen_seam += len(seams)
    assert seen_scan > 300 and seen_seam > 300


# ---- the entry points' own refusals come before any HIP call -----------------------------------------------------------------------------
def test_entry_points_refuse_bad_patterns_and_null_arrays_with_no_gpu_present():
    """HMSE_EINVAL (-1), never HMSE_EHIP (-3), before anything is cleared or launched.  (The pointers are host addresses; nothing may
    touch them.)"""
    from hmse_amd import _lib, ops
    lib = _lib.hip_lib()
    assert lib.hmse_abi_version() == 3
    assert (ops.APPROX_MAX_PATTERNS, ops.APPROX_MAX_LEN, ops.APPROX_MAX_K) == (8, 64, 16)
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr()
    u32 = lambda v: (C.c_uint32 * len(v))(*v)
    u8 = lambda v: (C.c_uint8 * max(len(v), 1))(*v)

    def calls(off=(0, 5, 9), k=(1, 0), flags=0, spans=True, **kw):
        a = dict(raw=b, raw_bytes=100, raw_off=b, cuts=b, slot=b, pat=b, n_hits=b, counts=b, status=b, hits=b, start=b, n_pat=len(off) - 1 if off else 2)
        a.update(kw)
        po, kk = (u32(off) if off is not None else None), (u8(k) if k is not None else None)
        return (lib.hmse_approx_scan(a["raw"], a["raw_bytes"], a["raw_off"], 1, None, a["pat"], po, kk, a["n_pat"], flags, b, 4, a["n_hits"],
                                     a["counts"], a["status"], None),
                lib.hmse_approx_seams(a["raw"], a["raw_bytes"], a["raw_off"], 1, a["cuts"], a["slot"], 1, a["pat"], po, kk, a["n_pat"], flags, b, 4,
                                      a["n_hits"], a["counts"], a["status"], None),
                lib.hmse_approx_spans(a["raw"], a["raw_bytes"], a["raw_off"], 1, a["cuts"], a["slot"], 1, a["pat"], po, a["n_pat"], flags,
                                      a["hits"], 3, a["start"], a["status"], None) if spans else None)

    for kw in (dict(off=(0,), k=()), dict(off=tuple(range(10)), k=(0,) * 9), dict(off=(0, 0), k=(0,)), dict(off=(0, 65), k=(3,)), dict(off=(0, 5, 4), k=(0, 0)),
               dict(flags=2), dict(flags=0x80000001), dict(off=None), dict(pat=None), dict(status=None), dict(raw_bytes=1 << 56)):
        assert calls(**kw) == (-1, -1, -1), kw
    for kw in (dict(k=(5, 0)), dict(k=(1, 4)), dict(off=(0, 64), k=(17,)), dict(k=None), dict(n_hits=None), dict(counts=None)):      # what only scan and seams take
        assert calls(spans=False, **kw) == (-1, -1, None), kw                          # (spans would accept these and launch)
    assert calls(raw_off=None) == (-1, -1, -1) and calls(raw=None) == (-1, -1, -1)
    assert calls(cuts=None)[1:] == (-1, -1) and calls(slot=None)[1:] == (-1, -1)
    assert calls(hits=None)[2] == -1 and calls(start=None)[2] == -1
    assert mem.sum().item() == 0


def test_wrappers_refuse_host_tensors():
    from hmse_amd import ops
    raw, off, pat = torch.zeros(16, dtype=torch.uint8), torch.tensor([0, 16]), torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.approx_scan(raw, off, None, pat, [0, 4], [1])
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.approx_seams(raw, off, off, torch.tensor([0]), pat, [0, 4], [1])
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.approx_spans(raw, off, off, torch.tensor([0]), pat, [0, 4], False, torch.tensor([3 << 8]))


def test_every_pointer_the_approx_wrappers_hand_to_the_library_comes_from_the_arena(monkeypatch):
    """hmse_approx_* and hmse_find_place replaced by recorders of their arguments (tests/arena.py: RecordingLib)."""
    import arena as A
    from hmse_amd import ops
    lib = A.record(monkeypatch, ("hmse_approx_scan", "hmse_approx_seams", "hmse_approx_spans", "hmse_find_place"))
    ar = A.Arena(torch.device("cpu"), "random", seed=5).install(monkeypatch)
    p = ar.place
    i64 = lambda *v: p(np.array(v, np.int64))
    pat = p(np.frombuffer(b"abcdefgh", np.uint8).copy(), misalign=1)
    raw = p(np.arange(100, dtype=np.uint8), misalign=3)
    raw_off, cuts, slot = i64(0, 40, 100), i64(0, 40, 100, 140), i64(0, 1, 0)
    calls = {"approx_scan": lambda: ops.approx_scan(raw, raw_off, p(np.array([2, 1], np.int32)), pat, [0, 5, 8], [2, 0]),
             "approx_scan count only": lambda: ops.approx_scan(raw, raw_off, None, pat, [0, 5, 8], [2, 0], True, hits_cap=0),
             "approx_seams": lambda: ops.approx_seams(raw, raw_off, cuts, slot, pat, [0, 5, 8], [2, 0], hits_cap=8),
             "approx_spans": lambda: ops.approx_spans(raw, raw_off, cuts, slot, pat, [0, 5, 8], False, i64(5 << 8, 50 << 8 | 1 << 3 | 1)),
             "find_place": lambda: ops.find_place(i64(5 << 8, 50 << 8 | 3), raw_off, cuts, slot, i64(0, 1, 2, 3), 3)}
    for name, fn in calls.items():
        n_call = len(lib.calls)
        fn()
        made = lib.calls[n_call:]
        assert made, name
        for call, ptrs, args in made:
            assert ptrs and all(ar.contains(q) for q in ptrs), (name, [hex(q) for q in ptrs if not ar.contains(q)])
            if call in ("hmse_approx_scan", "hmse_approx_seams"):                     # the host arrays: the bounds and the error bounds
                host = [a for a in args if not isinstance(a, int) and a is not None]
                assert [list(h) for h in host] == [[0, 5, 8], [2, 0]]
    assert not [k for k, _ in ar.requests if k != "buf"]                             # no workspace anywhere
    ar.check()


# ---- one end per fuzzy match -------------------------------------------------------------------------------------------------------------
def test_best_ends_equals_the_plain_loop():
    from hmse_amd import find
    rng = np.random.default_rng(1)
    for trial in range(200):
        P = int(rng.integers(0, 4))
        offs, errs, counts, want_o, want_e, want_c = [], [], [], [], [], []
        for _ in range(P):
            k = int(rng.integers(0, 60))
            o = np.sort(rng.choice(90, k, replace=False)).tolist()
            e = rng.integers(0, 4, k).tolist()
            keep = ref.best_ends(list(zip(o, e)))
            offs += o
            errs += e
            counts.append(k)
            want_o += [x for x, _ in keep]
            want_e += [x for _, x in keep]
            want_c.append(len(keep))
        c = torch.tensor(counts, dtype=torch.int64)
        ptr = torch.zeros(P + 1, dtype=torch.int64)
        ptr[1:] = torch.cumsum(c, 0)
        got = find.best_ends(find.ApproxFound(ptr, torch.tensor(offs, dtype=torch.int64), c, torch.tensor(errs, dtype=torch.int64), (b"x",) * P))
        assert (got.offsets.tolist(), got.errors.tolist(), got.counts.tolist()) == (want_o, want_e, want_c)
        assert got.ptr.tolist() == [0] + np.cumsum(want_c).astype(int).tolist() and len(got.patterns) == P
    assert ref.best_ends([(3, 2), (4, 1), (5, 1), (7, 0), (9, 3), (10, 3)]) == [(4, 1), (7, 0), (9, 3)]
    run = find.ApproxFound(torch.tensor([0, 5000]), torch.arange(5000), torch.tensor([5000]), torch.full((5000,), 2), (b"x",))
    assert find.best_ends(run).offsets.tolist() == [0]                               # one run of 5000 ends: no host loop


# ---- find_approx's own refusals ----------------------------------------------------------------------------------------------------------
def test_find_approx_refuses_its_arguments_before_any_device_work(monkeypatch):
    from hmse_amd import find, ops
    fd = find.StoreFinder.__new__(find.StoreFinder)                                  # no store, no device: nothing may be reached
    fd.dev, fd.n_records = torch.device("cpu"), 0
    for name in ("approx_scan", "approx_seams", "approx_spans", "find_place"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("device work"))
    for pats, k, msg in (([b"a" * 65], 1, "65 bytes"), ([b"abc"], -1, "outside 0.."), ([b"a" * 40], 17, "outside 0.."), ([b"abc"], 3, "not below its length"),
                         ([b"a"], 1, "not below its length"), ([b"abc", b"abcd"], [1], "1 entries for 2 patterns"), ([b"abc"], [1, 1], "2 entries for 1"),
                         ([b""], 0, "0 bytes"), (["abc"], 0, "str"), (b"abc", 0, "LIST")):
        for call in (fd.count_approx, fd.find_approx, fd.grep_approx):
            with pytest.raises(ValueError, match=msg):
                call(pats, k)
    with pytest.raises(ValueError, match="delim"):
        fd.grep_approx([b"abc"], 1, delim=b"ab")
    f = fd.find_approx([b"abc", b"de"], [2, 1])                                      # an empty store: an empty answer
    assert isinstance(f, find.ApproxFound) and isinstance(f, find.Found) and f.counts.tolist() == [0, 0] and f.errors.numel() == 0
    assert fd.count_approx([b"a" * 64], 16).tolist() == [0] and f.patterns == (b"abc", b"de")
    with pytest.raises(ValueError, match="ApproxFound"):
        fd.spans(find.Found(f.ptr, f.offsets, f.counts))
    s, e = fd.spans(f)
    assert s.numel() == 0 and e.numel() == 0


# ---- the kernels on the CPU --------------------------------------------------------------------------------------------------------------
def test_the_emulator_builds_and_its_cases_pass():
    """tools/approx_emu.py: the kernels cut out of approx.hip (and the validate and place kernels of chunkmap.h), one std::thread per
    lane, against Sellers' dynamic programme (no sanitizer here)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "approx_emu.py"), "--iters", "6", "--seed", "4242"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "6 cases ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
