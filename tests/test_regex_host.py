"""CPU: the regex compiler of hmse_amd.regex (include/hmse.h `hmse_regex`) against the `re` oracle of tests/regex_ref.py on a seeded
random-pattern generator, its hand-picked sizes, its refusals, determinism and minimality, the partition rule on the host, the entry
points' own refusals (HMSE_EINVAL in front of every HIP call), the wrappers' pointers, nonoverlapping, and the kernels on the CPU
(tools/regex_emu.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import regex_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOMS = [b"a", b"b", b"c", b"\\n", b".", b"[ab]", b"[^a]", b"[a-c]", b"[^\\nb]", b"[c\\n]"]
N_PATTERNS, BUDGET = 300, 11


def loop_body(rng, budget):
    """A group for under * + {m,}: one to three alternatives that begin with DIFFERENT literal bytes, each followed by up to two
    plain atoms — no alternative is empty, none starts like another, nothing inside is quantified -> (pattern, positions)."""
    firsts = [b"a", b"b", b"c", b"\\n"]
    rng.shuffle(firsts)
    alts, used = [], 0
    for f in firsts[: int(rng.integers(1, 4))]:
        if budget - used < 1:
            break
        k = min(int(rng.integers(0, 3)), budget - used - 1)
        alts.append(f + b"".join(ATOMS[int(rng.integers(0, len(ATOMS)))] for _ in range(k)))
        used += 1 + k
    return (b"(?:" if rng.random() < 0.5 else b"(") + b"|".join(alts) + b")", used


def gen(rng, depth, budget):
    """A random pattern over a b c \\n with classes, `.`, groups, |, ? * + and {m,n}, nested to `depth`, of at most `budget`
    literal / class positions after expanding the counted repeats -> (pattern, positions).  Built inside its budget: nothing is ever
    drawn again or refused.  `re` — the oracle — backtracks exponentially when a match must FAIL under an unbounded repeat whose body
    can be split in several ways ((a*)*, (a?b?|b)*), and both the definition's fullmatch loop and Longest ask for such failures.  So
    an unbounded repeat holds either one atom or a group that `re` walks without choice (loop_body); optional and counted groups
    nest freely.  The compiler does not care either way."""
    parts, used = [], 0
    for _ in range(int(rng.integers(1, 4))):
        left = budget - used
        if left < 1:
            break
        q = int(rng.integers(0, 8))                  # 0-3 none, 4 ?, 5 *, 6 +, 7 counted
        mult, suffix = 1, b""
        if q == 4:
            suffix = b"?"
        elif q == 5:
            suffix = b"*"
        elif q == 6:
            suffix = b"+"
        elif q == 7:
            n = int(rng.integers(1, 4))
            m = int(rng.integers(0, n + 1))
            form = int(rng.integers(0, 3))
            if form == 1:
                suffix, mult = b"{%d,%d}" % (m, n), n
            elif form == 2:
                suffix, mult = b"{%d,}" % m, max(m, 1)
            else:
                suffix, mult = b"{%d}" % n, n
        if mult > left:
            mult, suffix = 1, b""
        unbounded = suffix in (b"*", b"+") or suffix.endswith(b",}")
        if depth > 0 and unbounded and rng.random() < 0.4:
            p, iu = loop_body(rng, left // mult)
            parts.append(p + suffix)
            used += iu * mult
        elif depth > 0 and not unbounded and rng.random() < 0.4:
            inner, alts, iu = left // mult, [], 0
            for _ in range(int(rng.integers(1, 4))):
                if inner - iu < 1:
                    break
                p, u = gen(rng, depth - 1, inner - iu)
                alts.append(p)
                iu += u
            if rng.random() < 0.15:
                alts.append(b"")                      # an empty alternative
            parts.append((b"(?:" if rng.random() < 0.5 else b"(") + b"|".join(alts) + b")" + suffix)
            used += iu * mult
        else:
            parts.append(ATOMS[int(rng.integers(0, len(ATOMS)))] + suffix)
            used += mult
    return b"".join(parts), used


# ---- the compiler against the oracle -----------------------------------------------------------------------------------------------------
def test_random_patterns_equal_the_oracle_at_every_start():
    """300 generated patterns x the four flag combinations: none is refused, and match_at equals the oracle's length at EVERY start
    of a 2 KB corpus.  The oracle's lengths come from regex_ref.Longest (re alone, see there); on a sample of starts it is checked
    against the definition's own descending fullmatch loop."""
    from hmse_amd.regex import Regex
    rng = np.random.default_rng(7)
    corpus = bytes(np.frombuffer(b"abc\n", np.uint8)[rng.integers(0, 4, 2048)])
    seen_cyclic = seen_hits = 0
    for i in range(N_PATTERNS):
        p, used = gen(rng, 3, BUDGET)
        assert 1 <= used <= BUDGET, p
        for ic in (False, True):
            for dotall in (False, True):
                r = Regex(p, ic, dotall)                                               # RegexError here: the generator or the compiler is wrong
                assert r.n_states * r.n_classes <= (2 ** BUDGET + 1) * 5
                lg = ref.Longest(p, ic, dotall)
                want = [lg.length_at(corpus, o, r.reach) for o in range(len(corpus))]
                got = [r.match_at(corpus, o) for o in range(len(corpus))]
                assert got == want, (p, ic, dotall, [o for o in range(len(corpus)) if got[o] != want[o]][:3])
                assert r.match_all(corpus).tolist() == got
                seen_cyclic += r.reach == 256
                seen_hits += sum(1 for v in want if v)
                if i % 16 == 0:
                    for o in [k for k in range(len(corpus)) if want[k]][:2] + [len(corpus) - 3]:
                        assert ref.length_at(lg.rx, corpus, o, r.reach) == want[o], (p, o)
    assert seen_cyclic > 200 and seen_hits > 100000


SIZES = [(b"abc", 5, 4, 3, 3), (b"q", 3, 2, 1, 1), (rb"\d{4}-\d\d-\d\d", 12, 3, 10, 10), (b"a+", 3, 2, 256, 1), (b"(a|aa)*b", 3, 3, 256, 1),
         (rb"\W", 3, 2, 1, 1), (rb"[\x00-\x01\xfe-\xff]", 3, 2, 1, 1), (b"x.*y", 4, 4, 256, 2), (b"a{256}", 258, 2, 256, 256), (b"a{0,256}", 258, 2, 256, 1),
         (b"(ab|cd){2,3}", 11, 5, 6, 4)]


@pytest.mark.parametrize("pat,n_states,n_classes,reach,min_len", SIZES)
def test_hand_picked_patterns_have_their_sizes(pat, n_states, n_classes, reach, min_len):
    from hmse_amd.regex import Regex
    r = Regex(pat)
    assert (r.n_states, r.n_classes, r.reach, r.min_len) == (n_states, n_classes, reach, min_len)
    assert r.table.dtype == np.uint16 and r.table.size == n_states * n_classes and r.classmap.dtype == np.uint8 and r.classmap.size == 256
    assert not r.table[:n_classes].any() and int(r.classmap.max()) == n_classes - 1 and ((r.table & 0x7FFF) < n_states).all()
    assert r.classmap[0] == 0 and (np.diff([int(np.nonzero(r.classmap == c)[0][0]) for c in range(n_classes)]) > 0).all()   # by smallest byte
    assert r.resident_bytes == 0 and r.rx is None


def test_case_folding_and_the_ends_of_the_byte_range():
    from hmse_amd.regex import Regex
    r = Regex(b"[^a]", ignore_case=True)
    assert [r.match_at(bytes([b]), 0) for b in b"aAb\xe1\xc1\n"] == [0, 0, 1, 1, 1, 1]                 # closed under case BEFORE negation
    r = Regex(rb"[\x00-\x01\xfe-\xff]+")
    assert [r.match_at(b"\x00\x01\xff\xfe\x02", o) for o in range(5)] == [4, 3, 2, 1, 0] and r.classmap[0] == r.classmap[255] != r.classmap[2]
    r = Regex(b"stra\xdfe", ignore_case=True)
    assert r.match_at(b"STRA\xdfE", 0) == 6 and r.match_at(b"stra\xffe", 0) == 0 and r.match_at(b"STRA\xfFE", 0) == 0   # >= 0x80 untouched
    assert Regex(b".", dotall=True).match_at(b"\n", 0) == 1 and Regex(b".").match_at(b"\n", 0) == 0
    assert Regex(b"a+").match_all(b"aaaa").tolist() == [4, 3, 2, 1]
    long = Regex(b"x.*y")
    assert long.match_at(b"x" + b"-" * 254 + b"y" + b"y", 0) == 256 and long.match_at(b"x" + b"-" * 255 + b"y", 0) == 0


REFUSED = [(rb"a\b", 1), (rb"\Bx", 0), (rb"\Aa", 0), (rb"a\Z", 1), (rb"(a)\1", 3), (rb"\0", 0), (rb"a\07", 1), (rb"\e", 0), (rb"\8", 0), (rb"\xg1", 0),
           (rb"ab\x4", 2), (b"a\\", 1), (b"^a", 0), (b"a$", 1), (b"a|^b", 2), (b"[]", 0), (b"[^]", 0), (b"[z-a]", 1), (b"[a-]", 2), (b"[-a]", 1), (b"[a^]", 2),
           (b"[a[b]", 2), (b"[ab", 0), (rb"[\d-z]", 3), (rb"[a-\d]", 3), (b"a]", 1), (b"a}", 1), (b"a{", 1), (b"a{x}", 1), (b"a{,3}", 1), (b"a{3,2}", 1),
           (b"a{257}", 1), (b"a{2,300}", 1), (b"(?=a)", 0), (b"(?P<n>a)", 0), (b"(?i)a", 0), (b"(?#c)a", 0), (b"(a", 0), (b"a)", 1), (b"a*?", 2),
           (b"a+?", 2), (b"a??", 2), (b"a{2}?", 4), (b"a*+", 2), (b"a**", 2), (b"a+*", 2), (b"a{2}{3}", 4), (b"a?{2}", 2), (b"*a", 0), (b"a|+b", 2),
           (b"(?:?a)", 3), (b"(*a)", 1), (b"{2}", 0)]


@pytest.mark.parametrize("pat,offset", REFUSED)
def test_everything_outside_the_syntax_is_refused_with_its_offset(pat, offset):
    from hmse_amd.regex import Regex, RegexError
    with pytest.raises(RegexError, match=rf"at offset {offset}$") as e:
        Regex(pat)
    assert e.value.offset == offset and isinstance(e.value, ValueError)


def test_caps_and_empty_languages_are_refused():
    from hmse_amd.regex import Regex, RegexError
    with pytest.raises(RegexError, match=r"16385 states x 3 classes = 49155 table entries.*16384"):
        Regex(b"(a|b)*a(a|b){13}")
    assert Regex(b"(a|b)*a(a|b){11}").n_states == 4097
    with pytest.raises(RegexError, match="shortest non-empty match has more than HMSE_REGEX_MAX_LEN = 256"):
        Regex(b"a{200}b{57}")
    assert Regex(b"a{200}b{56}").min_len == 256
    for only_empty in (b"", b"()", b"(|)", b"a{0}", b"(a{0,0})*"):
        with pytest.raises(RegexError, match="nothing but the empty string"):
            Regex(only_empty)
    for not_bytes in ("ab", 17, None, [b"a"]):
        with pytest.raises(RegexError, match="bytes"):
            Regex(not_bytes)
    assert Regex(bytearray(b"ab")).pattern == b"ab" and Regex(memoryview(b"ab")).reach == 2


def test_the_build_is_deterministic_and_minimal():
    from hmse_amd.regex import Regex
    same = lambda a, b: (a.n_states, a.n_classes, a.reach, a.min_len) == (b.n_states, b.n_classes, b.reach, b.min_len) and \
        a.table.tobytes() == b.table.tobytes() and a.classmap.tobytes() == b.classmap.tobytes()
    for p in (rb"(error|warn)[a-z ]*id=", rb"\d{1,3}(\.\d{1,3}){3}", b"(a|b)*a(a|b){6}"):
        assert same(Regex(p, True), Regex(bytes(p), True))
    for a, b in ((b"(a|b)", b"[ab]"), (b"(a|aa)*b", b"a*b"), (b"ab|ac", b"a[bc]"), (b"a{2,}", b"aaa*"), (b"(a?){3}", b"a{0,3}"), (rb"\d", b"[0-9]"),
                 (b"[a-c]x|bx", b"(?:a|b|c)x")):
        assert same(Regex(a), Regex(b)), (a, b)
    assert same(Regex(b"k", ignore_case=True), Regex(b"[kK]"))


# ---- the partition rule on the host ------------------------------------------------------------------------------------------------------
def test_scan_starts_placed_plus_seam_starts_are_every_occurrence_once():
    from hmse_amd.regex import Regex
    rng = np.random.default_rng(5)
    pats = [Regex(p) for p in (b"ab", b"a+b", b"[ab]{3}", b"(ab|b)c?", b"c", rb"a[^\n]{0,4}c")]
    seen_seam = seen_scan = 0
    for it in range(300):
        r = pats[it % len(pats)]
        n = int(rng.integers(0, 300))
        corpus = bytes(np.frombuffer(b"abc\n", np.uint8)[rng.integers(0, 4, n)])
        lens = []
        while sum(lens) < n:
            lens.append(int(rng.choice([0, 1, 2, 1, 2, max(r.reach - 1, 0), min(r.reach, 9), min(r.reach, 9) + 1, 30])))
        if lens:
            lens[-1] -= sum(lens) - n
        lens += [0] * int(rng.integers(0, 3))
        cuts = [0] + [int(c) for c in np.cumsum(lens)]
        # a tables()-style map: dedupe the chunks into records, the scan's answer per record laid out at every chunk that names it
        recs, slot = [], []
        for k in range(len(cuts) - 1):
            c = corpus[cuts[k]: cuts[k + 1]]
            if c not in recs:
                recs.append(c)
            slot.append(recs.index(c))
        raw = b"".join(recs)
        raw_off = [0] + [int(v) for v in np.cumsum([len(x) for x in recs])]
        per_rec = [[(p, r.match_at(raw[:raw_off[q + 1]], p)) for p in range(raw_off[q], raw_off[q + 1]) if raw_off[q + 1] - p >= r.reach]
                   for q in range(len(recs))]
        placed = [(cuts[k] + p - raw_off[s], l) for k, s in enumerate(slot) for p, l in per_rec[s] if l]
        seams = []
        for k in range(len(cuts) - 1):
            for o in range(max(cuts[k], cuts[k + 1] - (r.reach - 1)), cuts[k + 1]):
                l = r.match_at(corpus, o)
                if l:
                    seams.append((o, l))
        want = ref.find(corpus, r.pattern, r.reach)
        assert sorted(placed + seams) == want and len(set(placed + seams)) == len(want)
        assert (placed, seams) == ref.split(corpus, want, r.reach, cuts) if cuts[-1] else not want
        seen_seam += len(seams)
        seen_scan += len(placed)
    assert seen_seam > 300 and seen_scan > 1000


# ---- the entry points' own refusals come before any HIP call -----------------------------------------------------------------------------
def test_entry_points_refuse_bad_headers_and_null_arrays_with_no_gpu_present():
    """HMSE_EINVAL (-1), never HMSE_EHIP (-3), before anything is cleared or launched.  (The pointers are host addresses; nothing may
    touch them.)"""
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    assert lib.hmse_abi_version() == 3
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr()
    size = C.sizeof(_lib.HmseRegex)
    assert size == 32

    def hdr(**kw):
        f = dict(struct_size=size, n_states=4, n_classes=3, reach=5, table=b, classmap=b)
        f.update(kw)
        return _lib.HmseRegex(*[f[n] for n, _ in _lib.HmseRegex._fields_])

    def calls(h, **kw):
        a = dict(raw=b, raw_bytes=100, raw_off=b, cuts=b, slot=b, n_hits=b, count=b, status=b)
        a.update(kw)
        hp = C.byref(h) if h is not None else None
        return (lib.hmse_regex_scan(a["raw"], a["raw_bytes"], a["raw_off"], 1, None, hp, b, 4, a["n_hits"], a["count"], a["status"], None),
                lib.hmse_regex_seams(a["raw"], a["raw_bytes"], a["raw_off"], 1, a["cuts"], a["slot"], 1, hp, b, 4, a["n_hits"], a["count"], a["status"], None))

    for kw in (dict(struct_size=size - 8), dict(struct_size=0), dict(n_states=1), dict(n_states=0), dict(n_states=32768, n_classes=1), dict(n_classes=0),
               dict(n_classes=257), dict(n_states=129, n_classes=128), dict(n_states=16385, n_classes=1), dict(reach=0), dict(reach=257),
               dict(table=None), dict(classmap=None)):
        assert calls(hdr(**kw)) == (-1, -1), kw
    assert calls(None) == (-1, -1)
    for kw in (dict(n_hits=None), dict(status=None), dict(count=None)):
        assert calls(hdr(), **kw) == (-1, -1), kw
    assert calls(hdr(), raw_off=None) == (-1, -1) and calls(hdr(), raw=None) == (-1, -1)
    assert calls(hdr(), cuts=None)[1] == -1 and calls(hdr(), slot=None)[1] == -1 and calls(hdr(), raw_bytes=1 << 56)[0] == -1
    assert mem.sum().item() == 0


def test_wrappers_refuse_host_tensors_and_arrays_that_do_not_match_their_header():
    from hmse_amd import ops
    from hmse_amd.regex import Regex
    h = Regex(b"ab+")
    rx = ops.Regex(torch.from_numpy(h.table.view(np.int16).copy()), torch.from_numpy(h.classmap.copy()), h.n_states, h.n_classes, h.reach)
    raw, off = torch.zeros(16, dtype=torch.uint8), torch.tensor([0, 16])
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.regex_scan(raw, off, None, rx)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.regex_seams(raw, off, off, torch.tensor([0]), rx)


def test_every_pointer_the_regex_wrappers_hand_to_the_library_comes_from_the_arena(monkeypatch):
    """hmse_regex_* and hmse_find_place replaced by recorders of their arguments (tests/arena.py: RecordingLib)."""
    import arena as A
    from hmse_amd import _lib, ops
    from hmse_amd.regex import Regex
    lib = A.record(monkeypatch, ("hmse_regex_scan", "hmse_regex_seams", "hmse_find_place"))
    ar = A.Arena(torch.device("cpu"), "random", seed=5).install(monkeypatch)
    p = ar.place
    i64 = lambda *v: p(np.array(v, np.int64))
    h = Regex(b"ab+c", True)
    rx = ops.Regex(p(h.table.view(np.int16).copy()), p(h.classmap.copy(), misalign=1), h.n_states, h.n_classes, h.reach)
    raw = p(np.arange(100, dtype=np.uint8), misalign=3)
    raw_off, cuts, slot = i64(0, 40, 100), i64(0, 40, 100, 140), i64(0, 1, 0)
    calls = {"regex_scan": lambda: ops.regex_scan(raw, raw_off, p(np.array([2, 1], np.int32)), rx),
             "regex_scan count only": lambda: ops.regex_scan(raw, raw_off, None, rx, hits_cap=0),
             "regex_seams": lambda: ops.regex_seams(raw, raw_off, cuts, slot, rx, hits_cap=8),
             "find_place": lambda: ops.find_place(i64(5 << 8, 50 << 8 | 3), raw_off, cuts, slot, i64(0, 1, 2, 3), 3)}
    for name, fn in calls.items():
        n_call = len(lib.calls)
        fn()
        made = lib.calls[n_call:]
        assert made, name
        for call, ptrs, args in made:
            assert ptrs and all(ar.contains(q) for q in ptrs), (name, [hex(q) for q in ptrs if not ar.contains(q)])
            if call != "hmse_find_place":                                            # the header: a host struct naming arena memory only
                hdr = [a for a in args if not isinstance(a, int) and a is not None][0]._obj
                assert (hdr.struct_size, hdr.n_states, hdr.n_classes, hdr.reach) == (C.sizeof(_lib.HmseRegex), h.n_states, h.n_classes, 256)
                assert ar.contains(hdr.table) and ar.contains(hdr.classmap)
    assert not [k for k, _ in ar.requests if k != "buf"]                             # no workspace anywhere
    ar.check()


# ---- grep -o's choice --------------------------------------------------------------------------------------------------------------------
def test_nonoverlapping_equals_the_plain_loop():
    from hmse_amd import find
    rng = np.random.default_rng(1)
    for trial in range(200):
        P = int(rng.integers(0, 4))
        offs, lens, counts = [], [], []
        for _ in range(P):
            k = int(rng.integers(0, 40))
            offs += np.sort(rng.choice(120, k, replace=False)).tolist()
            lens += rng.integers(1, 12, k).tolist()
            counts.append(k)
        c = torch.tensor(counts, dtype=torch.int64)
        ptr = torch.zeros(P + 1, dtype=torch.int64)
        ptr[1:] = torch.cumsum(c, 0)
        got = find.nonoverlapping(find.RegexFound(ptr, torch.tensor(offs, dtype=torch.int64), c, torch.tensor(lens, dtype=torch.int64)))
        want_o, want_l, want_c = [], [], []
        for j in range(P):
            a, b = int(ptr[j]), int(ptr[j + 1])
            keep = ref.nonoverlapping(offs[a:b], lens[a:b])
            want_o += [offs[a + i] for i in keep]
            want_l += [lens[a + i] for i in keep]
            want_c.append(len(keep))
        assert (got.offsets.tolist(), got.lengths.tolist(), got.counts.tolist()) == (want_o, want_l, want_c)
        assert got.ptr.tolist() == [0] + np.cumsum(want_c).astype(int).tolist()
    chain = find.RegexFound(torch.tensor([0, 5000]), torch.arange(5000), torch.tensor([5000]), torch.full((5000,), 2))
    assert find.nonoverlapping(chain).offsets.tolist() == list(range(0, 5000, 2))      # a chain of 2500 hops: pointer doubling, no host loop


# ---- the kernels on the CPU --------------------------------------------------------------------------------------------------------------
def test_the_emulator_builds_and_its_cases_pass():
    """tools/regex_emu.py: the kernels of regex_core.h in their plain form (and place_kernel of chunkmap.h), one std::thread per lane, against a
    brute-force walk (no sanitizer here)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "regex_emu.py"), "--iters", "6", "--seed", "4242"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "6 cases ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
