"""CPU: the tally of search results (hmse_amd.find tally / tally_regex; include/hmse_tally.h) without a GPU — the plain-Python reference
of tests/tally_ref.py against collections.Counter, its key against the kernels' own keys (tools/tally_emu.py runs tally.hip's kernels on
CPU threads), the round loop of find.tally_ranges on CPU tensors with plain-Python stand-ins for the two ops calls and with keys narrow
enough to collide, then the new header against _lib (prototypes, exported symbols, the ISA audit), the entry points' own refusals
(HMSE_EINVAL in front of every HIP call) and the wrappers' and methods' refusals."""
import collections
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import tally_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmse_tally.h")
CALLS = ("hmse_tally_keys", "hmse_tally_same")
FIELDS = ("ptr", "start", "end", "count", "distinct", "total", "value_of")


def _random_case(rnd, n_max=60):
    """a corpus over a few words in both cases (and bytes whose | 0x20 form is another byte), ranges in 1..3 groups, some empty"""
    words = [b"ab", b"AB", b"aB", b"abc", b"@", b"`", b"[", b"{", b"\xc1", b"\xe1", b"z", b"Z", b""]
    corpus = b"".join(rnd.choice(words) for _ in range(rnd.randint(0, 40)))
    N = len(corpus)
    n = rnd.randint(0, n_max)
    starts, ends = [], []
    for _ in range(n):
        s = rnd.randint(0, N)
        e = s if rnd.random() < 0.1 else min(N, s + rnd.randint(0, 3))
        starts.append(s); ends.append(e)
    G = rnd.randint(1, 3)
    ptr = [0] + sorted(rnd.randint(0, n) for _ in range(G - 1)) + [n]
    return corpus, starts, ends, ptr


# ---- the reference against Counter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ic", [False, True])
def test_reference_equals_counter_over_slices_with_order_and_representatives(ic):
    rnd = random.Random(11 + ic)
    seen_ties = 0
    for _ in range(300):
        corpus, starts, ends, ptr = _random_case(rnd)
        top = rnd.choice([None, None, 1, 2, 5])
        t = ref.tally(corpus, starts, ends, ptr, ic, top)
        low = lambda b: bytes(c + 32 if 65 <= c <= 90 else c for c in b)           # (bytes.lower is locale-free too: ASCII only)
        assert low(b"AZ@[\xc1") == b"az@[\xc1" == b"AZ@[\xc1".lower()
        for j in range(len(ptr) - 1):
            texts = [low(corpus[starts[i]:ends[i]]) if ic else corpus[starts[i]:ends[i]] for i in range(ptr[j], ptr[j + 1])]
            cnt = collections.Counter(texts)
            lo, hi = t["ptr"][j], t["ptr"][j + 1]
            assert t["distinct"][j] == len(cnt) and t["total"][j] == len(texts) and hi - lo == (len(cnt) if top is None else min(top, len(cnt)))
            first = {}                                                                 # the representative: smallest (start, index)
            for i in range(ptr[j], ptr[j + 1]):
                k = texts[i - ptr[j]]
                if k not in first or (starts[i], i) < (starts[first[k]], first[k]):
                    first[k] = i
            want = sorted(cnt, key=lambda k: (-cnt[k], starts[first[k]], first[k]))[:top]
            got = [low(corpus[s:e]) if ic else corpus[s:e] for s, e in zip(t["start"][lo:hi], t["end"][lo:hi])]
            assert got == want and t["count"][lo:hi] == [cnt[k] for k in want]
            assert [(s, e) for s, e in zip(t["start"][lo:hi], t["end"][lo:hi])] == [(starts[first[k]], ends[first[k]]) for k in want]
            seen_ties += len(set(cnt.values())) < len(cnt)
            for i in range(ptr[j], ptr[j + 1]):
                v = t["value_of"][i]
                assert (v == -1 and texts[i - ptr[j]] not in want) or (lo <= v < hi and got[v - lo] == texts[i - ptr[j]])
    assert seen_ties > 100


def test_reference_key_is_the_formula_of_the_header():
    header = open(HEADER).read()
    consts = {k: int(v, 16) for k, v in re.findall(r"#define HMSE_TALLY_(\w+)\s+0x([0-9A-Fa-f]+)u", header)}
    assert consts == {"M1": ref.M1, "M2": ref.M2, "LEN": ref.K_LEN, "SEED": ref.K_SEED, "MIX1": ref.MIX1, "MIX2": ref.MIX2}
    assert ref.key_of_text(b"") == ref.key_of_text(b"", 0, 64) != ref.key_of_text(b"", 1) and ref.key_of_text(b"\x00") != ref.key_of_text(b"\x00\x00")
    assert ref.key_of_text(b"abc", 5, 8) == ref.key_of_text(b"abc", 5) & 0xFF and ref.key_of_text(b"abc", 5, 1) in (0, 1)
    assert ref.key(b"xABCx", 1, 4, True) == ref.key_of_text(b"abc") != ref.key(b"xABCx", 1, 4)
    assert ref.text_of(b"@[`{\xc1AZ", 0, 7, True) == b"@[`{\xc1az"


# ---- the kernels on the CPU ------------------------------------------------------------------------------------------------------------------
def test_the_emulator_passes_and_its_keys_equal_the_python_restatement_bit_for_bit():
    """A short unsanitised pass of tools/tally_emu.py (the kernels of tally.hip, one std::thread per lane, against the definition on random
    chunk maps), then its KEY lines: ranges of length 0, 1, 63, 64, 65 and 128 of the corpus C[q] = (37 q + 11) & 0xFF under seeds 0, 1
    and 2^63, folded and not, 64 and 8 key bits."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tally_emu.py"), "--iters", "12"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    corpus = bytes((q * 37 + 11) & 0xFF for q in range(300))
    assert any(65 <= b <= 90 for b in corpus[:64])
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("KEY ")]
    seen = set()
    for _, s, e, fold, seed, bits, key in rows:
        s, e, fold, seed, bits = int(s), int(e), int(fold), int(seed), int(bits)
        assert int(key, 16) == ref.key(corpus, s, e, bool(fold), seed, bits), (s, e, fold, seed, bits)
        seen.add((e - s, seed, fold, bits))
    assert seen == {(L, sd, f, b) for L in (0, 1, 63, 64, 65, 128) for sd in (0, 1, 1 << 63) for f in (0, 1) for b in (64, 8)}
    # four starts each; unfolded, the 3 x 5 x 4 non-empty texts and the three seeds' empty text all have keys of their own
    assert len(rows) == 4 * len(seen) and len({r_[6] for r_ in rows if r_[5] == "64" and r_[3] == "0"}) == 3 * 5 * 4 + 3


# ---- the round loop on CPU tensors -------------------------------------------------------------------------------------------------------------
def _stand_ins(corpus, ic, key_bits, calls):
    import torch
    def keys(s, e, seed):
        calls.append(("keys", s.numel(), seed))
        return torch.tensor([ref.signed(k) for k in ref.keys(corpus, s.tolist(), e.tolist(), ic, seed, key_bits)], dtype=torch.int64)
    def same(s, e, rep):
        calls.append(("same", s.numel()))
        assert s.is_contiguous() and e.is_contiguous() and rep.dtype == torch.int64
        return torch.tensor(ref.same(corpus, s.tolist(), e.tolist(), rep.tolist(), ic), dtype=torch.uint8)
    return keys, same


def _run_rounds(corpus, starts, ends, ptr, ic, top, key_bits, max_rounds=64):
    import torch
    from hmse_amd import find
    i64 = lambda v: torch.tensor(v, dtype=torch.int64)
    G = len(ptr) - 1
    group = torch.repeat_interleave(torch.arange(G), i64(ptr[1:]) - i64(ptr[:-1]))
    calls = []
    keys, same = _stand_ins(corpus, ic, key_bits, calls)
    t = find.tally_ranges(i64(starts), i64(ends), group, G, keys, same, top, max_rounds)
    return t, calls


@pytest.mark.parametrize("key_bits", [1, 2, 8, 64])
def test_round_loop_on_cpu_tensors_gives_the_reference_tally_under_colliding_keys(key_bits):
    import torch
    rnd = random.Random(5)
    most = 0
    for it in range(60):
        corpus, starts, ends, ptr = _random_case(rnd, n_max=80)
        ic, top = bool(it & 1), rnd.choice([None, None, 1, 3])
        t, calls = _run_rounds(corpus, starts, ends, ptr, ic, top, key_bits)
        want = ref.tally(corpus, starts, ends, ptr, ic, top)
        for f in FIELDS:
            got = getattr(t, f)
            assert got.dtype == torch.int64 and got.tolist() == want[f], (f, it)
        assert t.rounds == len(calls) // 2 and [c[0] for c in calls] == ["keys", "same"] * t.rounds
        assert [c[2] for c in calls[::2]] == list(range(t.rounds))                     # seed = round
        assert [c[1] for c in calls[::2]] == sorted((c[1] for c in calls[::2]), reverse=True) and (len(starts) == 0) == (t.rounds == 0)
        most = max(most, t.rounds)
    assert (most > 2) if key_bits <= 2 else (most == 1 if key_bits == 64 else most >= 1)


def test_round_loop_raises_when_max_rounds_do_not_resolve_every_range():
    corpus = b"abc"                                   # three distinct values in two buckets at most: one round cannot resolve them
    with pytest.raises(RuntimeError, match=r"tally: \d+ of 6 ranges are unresolved after max_rounds = 1 rounds \(\d+ distinct values so far\)"):
        _run_rounds(corpus, [0, 1, 2, 0, 1, 2], [1, 2, 3, 1, 2, 3], [0, 6], False, None, 1, max_rounds=1)
    t, _ = _run_rounds(corpus, [0, 1, 2, 0, 1, 2], [1, 2, 3, 1, 2, 3], [0, 6], False, None, 1, max_rounds=64)
    assert t.count.tolist() == [2, 2, 2] and t.start.tolist() == [0, 1, 2] and t.value_of.tolist() == [0, 1, 2, 0, 1, 2] and t.rounds >= 2


# ---- the header, the library, the entry points -------------------------------------------------------------------------------------------------
def test_signatures_equal_the_header():
    import test_abi
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    header = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = re.findall(r"^(\w+) (hmse_[a-z0-9_]+)\(([^;]*)\);", plain, re.M)
    assert [name for _, name, _ in protos] == list(_lib.TALLY_SIGNATURES) == list(CALLS)
    assert not set(_lib.TALLY_SIGNATURES) & (set(_lib.PARSED) | set(_lib.PARSED_REGEXA)) and set(_lib.PARSED_TALLY) == set(CALLS)
    for ret, name, params in protos:
        t_ret, _, t_params = _lib.TALLY_SIGNATURES[name].partition(":")
        entries = [e.split() if e.strip() != "stream" else ["stream", "stream"] for e in t_params.split(",")]
        decls = [re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*", d).groups() for d in params.split(",")]
        assert test_abi._C_RETURN[t_ret] == ret and [e[1] for e in entries] == [d[2] for d in decls], name
        assert all(test_abi.kind_agrees(kind, ty, bool(star)) for (kind, _), (ty, star, _) in zip(entries, decls)), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.PARSED_TALLY[name][0] and list(fn.argtypes) == [q.ctype for q in _lib.PARSED_TALLY[name][1]], name
    # the tables are hmse_lines_gather's, the ABI version stays
    assert _lib.TALLY_SIGNATURES["hmse_tally_keys"].split(" u64*? start")[0] == _lib.SIGNATURES["hmse_lines_gather"].split(" u64*? start")[0]
    assert lib.hmse_abi_version() == 3
    assert "Out of scope" in header and "bit 1" in header


def test_the_library_exports_its_header_and_passes_the_isa_audit():
    """libhmse_tally.so beside libhmse_hip.so: exported == declared in include/hmse_tally.h; no divergent loop at all in the two main
    kernels and no cross-lane instruction inside one anywhere; no Async / Graph import, no import the pinned list does not allow.  The
    other libraries gain no symbol."""
    import json
    from hmse_amd import _lib
    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return sorted(x for x in (ln.split()[-1] for ln in out.splitlines() if ln.split()[1:2] and ln.split()[1] in "TW") if not x.startswith("_"))
    assert exported(_lib.TALLY_LIB_PATH) == sorted(CALLS)
    assert exported(_lib.REGEXA_LIB_PATH) == sorted(_lib.REGEXA_SIGNATURES) and exported(_lib.GUNZIP_LIB_PATH) == sorted(_lib.GUNZIP_SIGNATURES)
    assert not [x for x in exported(_lib.HIP_LIB_PATH) if "tally" in x] and not set(CALLS) & set(_lib.EXPORTED_SYMBOLS)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    rep = isa_audit.audit(_lib.TALLY_LIB_PATH)
    assert {"tally_ranges_kernel", "tally_keys_kernel", "tally_same_kernel"} <= set(rep)
    for k in ("tally_keys_kernel", "tally_same_kernel"):
        assert rep[k]["loops"] >= 2 and rep[k]["divergent_loops"] == 0, (k, rep[k])
    assert isa_audit.summary(rep) == {}
    pin = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_audit.json")))
    imports = isa_audit.imported_hip_calls(_lib.TALLY_LIB_PATH)
    assert not [x for x in imports if "Async" in x or "Graph" in x], imports
    assert set(imports) <= set(pin["hip_imports_allowed"]), sorted(set(imports) - set(pin["hip_imports_allowed"]))


def test_entry_points_refuse_bad_arguments_with_no_gpu_present():
    """HMSE_EINVAL (-1), never HMSE_EHIP (-3): refused in front of every clear and launch (the pointers are host addresses)"""
    import torch
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr() + (-mem.data_ptr()) % 256
    keys_names = ("raw", "raw_bytes", "raw_off", "n_rec", "cuts", "slot", "n_chunks", "start", "end", "n", "flags", "seed", "key_bits", "key", "status")
    same_names = ("raw", "raw_bytes", "raw_off", "n_rec", "cuts", "slot", "n_chunks", "start", "end", "rep", "n", "flags", "same", "status")
    dflt = dict(raw=b, raw_bytes=64, raw_off=b, n_rec=1, cuts=b, slot=b, n_chunks=1, start=b, end=b, rep=b, n=2, flags=0, seed=0, key_bits=64, key=b,
                same=b, status=b)

    def call(fn, names, **kw):
        a = {**dflt, **kw}
        return fn(*[a[k] for k in names], None)
    both = ((lib.hmse_tally_keys, keys_names), (lib.hmse_tally_same, same_names))
    for fn, names in both:
        for kw in (dict(status=None), dict(raw=None), dict(raw_off=None), dict(cuts=None), dict(slot=None), dict(start=None), dict(end=None),
                   dict(n=1 << 33), dict(n=(1 << 64) - 1), dict(flags=2), dict(flags=3), dict(flags=1 << 31),
                   dict(raw_off=None, n_chunks=0, n=0), dict(status=None, n=0)):
            assert call(fn, names, **kw) == -1, (names[9], kw)
    for kw in (dict(key_bits=0), dict(key_bits=65), dict(key_bits=1 << 31), dict(key=None), dict(key_bits=0, n=0)):
        assert call(*both[0], **kw) == -1, kw
    for kw in (dict(rep=None), dict(same=None)):
        assert call(*both[1], **kw) == -1, kw
    assert mem.sum().item() == 0


def test_wrappers_and_methods_refuse_what_they_should(monkeypatch):
    import torch
    from hmse_amd import find, ops
    u8 = torch.zeros(8, dtype=torch.uint8)
    z = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.tally_keys(u8, z, z, z[:1], z, z)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.tally_same(u8, z, z, z[:1], z, z, z)
    with pytest.raises(ops.HmseError, match="start must be torch.int64"):
        ops.tally_keys(u8, z, z, z[:1], z.to(torch.int32), z)
    with pytest.raises(ops.HmseError, match="rep must be torch.int64"):
        ops.tally_same(u8, z, z, z[:1], z, z, z.to(torch.int32))
    with pytest.raises(ops.HmseError, match="raw must be torch.uint8"):
        ops.tally_keys(u8.to(torch.int8), z, z, z[:1], z, z)
    with pytest.raises(ops.HmseError, match="do not match"):
        ops.tally_same(u8, z, z, z[:1], z, z, z[:1])
    with pytest.raises(ops.HmseError, match="do not match"):
        ops.tally_keys(u8, z, z, z, z, z)
    with pytest.raises(ops.HmseError, match="key_bits = 65"):
        ops.tally_keys(u8, z, z, z[:1], z, z, key_bits=65)
    with pytest.raises(TypeError, match="takes 15 arguments"):
        ops._call("hmse_tally_keys", 1, 2, 3)
    with pytest.raises(KeyError):
        ops._call("hmse_tally_nothing")
    # the methods, on a finder that no device work made: the refusals come in front of every launch
    fd = find.StoreFinder.__new__(find.StoreFinder)
    fd.dev = torch.device("cpu")
    fd.raw, fd.raw_off, fd.cuts, fd.slot, fd.n_bytes = u8, z, z, z[:1], 8
    pair = (torch.tensor([0, 1]), torch.tensor([1, 2]))
    with pytest.raises(ValueError, match=r"is a Found, which has offsets but no lengths.*spans\(\)"):
        fd.tally(find.Found(z, z[:0], z[:1]))
    with pytest.raises(ValueError, match=r"is a ApproxFound, which has offsets but no lengths.*\(start, end\) pair"):
        fd.tally(find.ApproxFound(z, z[:0], z[:1], z[:0]))
    for top in (0, -1):
        with pytest.raises(ValueError, match=f"top = {top} must be at least 1"):
            fd.tally(pair, top=top)
    with pytest.raises(ValueError, match="int64 tensors on the finder's device"):
        fd.tally((pair[0].to(torch.int32), pair[1]))
    with pytest.raises(ValueError, match="one length"):
        fd.tally((pair[0], pair[1][:1]))
    with pytest.raises(ValueError, match="what is a RegexFound, a Lines"):
        fd.tally([1, 2])
    with pytest.raises(ValueError, match="descends or leaves the corpus of n_bytes = 8"):
        fd.tally((pair[0], torch.tensor([1, 9])))
    with pytest.raises(ValueError, match="descends or leaves"):
        fd.tally((torch.tensor([2, 1]), torch.tensor([1, 2])))
    with pytest.raises(ValueError, match="ptr does not split the 2 ranges"):
        fd.tally((pair[0], pair[1], torch.tensor([0, 1])))
    with pytest.raises(ValueError, match="ptr does not split"):
        fd.tally((pair[0], pair[1], torch.tensor([0, 3, 2])))
    # no ranges, no groups: empty results of the right shapes, no launch (the library is never asked)
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("a launch"))
    e = torch.zeros(0, dtype=torch.int64)
    for what, G in (((e, e), 1), ((e, e, torch.tensor([0, 0, 0])), 2), ((e, e, torch.tensor([0])), 0), (find.RegexFound(torch.zeros(4, dtype=torch.int64), e, z.new_zeros(3), e), 3)):
        t = fd.tally(what, top=2)
        assert t.ptr.tolist() == [0] * (G + 1) and t.distinct.tolist() == [0] * G == t.total.tolist() and t.rounds == 0
        assert all(getattr(t, f).numel() == 0 and getattr(t, f).dtype == torch.int64 for f in ("start", "end", "count", "value_of"))
    with pytest.raises(pytest.fail.Exception, match="a launch"):                  # a host tensor reaches the one call path, which would refuse it
        fd.tally(pair)
