"""CPU: substitute / redact (hmse_amd.find substitute, redact, substitute_regex, redact_regex; include/hmse_subst.h) without a GPU — the
plain-Python reference of tests/subst_ref.py against itself (the splice, the per-position form the kernel computes, the formula of
out_off) and against re.sub, then the new header against _lib (prototype, exported symbols, the ISA audit), the entry point's own
refusals (HMSE_EINVAL in front of every HIP call), the wrapper's and the methods' refusals, translate on CPU tensors, and a short pass of
the kernels on CPU threads (tools/subst_emu.py)."""
import os
import random
import re
import subprocess
import sys

import pytest

import regex_ref
import subst_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmse_subst.h")
CALLS = ("hmse_subst_apply",)


def _random_case(rnd, fill):
    """a small corpus and a legal edit list: ties, insertions (several at one place), deletions, touching edits"""
    N = rnd.choice([0, 1, 2, 5, rnd.randint(3, 60)])
    corpus = bytes(rnd.randrange(97, 123) for _ in range(N))
    reps = [bytes(rnd.randrange(65, 91) for _ in range(1 if fill else rnd.choice([0, 0, 1, 2, 5, 20]))) for _ in range(rnd.randint(1, 4))]
    edits, at = [], 0
    for _ in range(rnd.randint(0, 12)):
        s = at + rnd.choice([0, 0, 1, rnd.randint(0, 8)])
        if s > N:
            break
        e = min(N, s + rnd.choice([0, 0, 1, 1, rnd.randint(0, 9)]))
        edits.append((s, e, rnd.randrange(len(reps))))
        at = e
    return corpus, edits, reps


# ---- the reference against itself and against re.sub ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True])
def test_the_splice_equals_its_per_position_form(fill):
    rnd = random.Random(5 + fill)
    ties = inserts = deletes = 0
    for _ in range(3000):
        corpus, edits, reps = _random_case(rnd, fill)
        out, out_off = ref.splice(corpus, edits, reps, fill)
        assert out_off == ref.out_offsets(len(corpus), edits, reps, fill) and len(out) == out_off[-1]
        assert ref.per_position(corpus, edits, reps, out_off, fill) == out
        assert out_off == sorted(out_off)
        ties += len(set(out_off[:-1])) < len(edits)
        inserts += any(s == e for s, e, _ in edits)
        deletes += any(s < e and not ref.replacement((s, e, r), reps, fill) for s, e, r in edits)
        if fill:
            assert len(out) == len(corpus)
    assert ties > 100 and inserts > 100 and (fill or deletes > 100)
    # by hand: an insertion in front, two at one place in the order given, a deletion, an insertion at the end
    out, off = ref.splice(b"abcdef", [(0, 0, 0), (2, 2, 1), (2, 2, 0), (3, 5, 2), (6, 6, 1)], [b"X", b"yy", b""])
    assert out == b"XabyyXcfyy" and off == [0, 3, 5, 7, 8, 10]
    assert ref.splice(b"abcdef", [(1, 3, 0), (3, 3, 0), (4, 6, 1)], [b"*", b"#"], True) == (b"a**d##", [1, 3, 4, 6])
    assert not ref.edits_ok(6, [(2, 4, 0), (3, 5, 0)], [b"x"], False) and not ref.edits_ok(6, [(2, 7, 0)], [b"x"], False)
    assert not ref.edits_ok(6, [(2, 3, 1)], [b"x"], False) and not ref.edits_ok(6, [(2, 3, 0)], [b"xy"], True) and ref.edits_ok(6, [], [], True)


def test_the_reference_equals_re_sub_where_leftmost_longest_is_pythons_leftmost_first():
    from hmse_amd import corpus as corpus_mod
    text = corpus_mod.wiki_synth(200000, seed=3).tobytes()
    for pattern, repl in ((rb"[0-9]+", b"<N>"), (rb"[A-Z][a-z]+", b""), (rb"the", b"THE "), (rb" +", b"_")):
        found = regex_ref.find(text, pattern, 256)
        kept = ref.leftmost_longest(found)
        spans = [m.span() for m in re.finditer(pattern, text)]
        assert [(s, s + ln) for s, ln in kept] == spans and len(spans) > 10, pattern       # the coincidence, on this input
        edits = [(s, s + ln, 0) for s, ln in kept]
        assert ref.splice(text, edits, [repl])[0] == re.sub(pattern, repl.replace(b"\\", b"\\\\"), text)
        red = ref.splice(text, edits, [b"#"], True)[0]
        assert red == re.sub(pattern, lambda m: b"#" * len(m.group()), text) and len(red) == len(text)


def test_translate_equals_the_reference_on_cpu_tensors():
    import torch
    from hmse_amd import find
    rnd = random.Random(9)
    for it in range(400):
        fill = it % 3 == 0
        corpus, edits, reps = _random_case(rnd, fill)
        N = len(corpus)
        out, out_off = ref.splice(corpus, edits, reps, fill)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64)
        sub = find.Substituted(torch.zeros(0, dtype=torch.uint8), i64([e[0] for e in edits]), i64([e[1] for e in edits]), i64([e[2] for e in edits]),
                               i64(out_off), len(edits), N, len(out))
        qs = list(range(N + 1))
        got = sub.translate(i64(qs))
        want = [ref.translate(N, edits, out_off, q) for q in qs]
        assert got.dtype == torch.int64 and got.tolist() == want, (corpus, edits, reps, fill)
        for q in qs[:N]:                                                         # a kept byte is found where it is said to be
            if not any(s <= q < e for s, e, _ in edits):
                assert out[want[q]] == corpus[q]
        for i, (s, e, _) in enumerate(edits):
            if s < e:
                assert want[s] == out_off[i] == want[e - 1]
        assert sub.translate(i64([[N], [0]])).shape == (2, 1)
        with pytest.raises(ValueError, match="outside 0..n_bytes_in"):
            sub.translate(i64([N + 1]))
    with pytest.raises(ValueError, match="offsets are int64"):
        sub.translate(torch.tensor([0], dtype=torch.int32))


# ---- the header, the library, the entry point ----------------------------------------------------------------------------------------------
def test_signatures_equal_the_header():
    import test_abi
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    header = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = re.findall(r"^(\w+) (hmse_[a-z0-9_]+)\(([^;]*)\);", plain, re.M)
    assert [name for _, name, _ in protos] == list(_lib.SUBST_SIGNATURES) == list(CALLS)
    assert not set(_lib.SUBST_SIGNATURES) & (set(_lib.PARSED) | set(_lib.PARSED_REGEXA) | set(_lib.PARSED_TALLY)) and set(_lib.PARSED_SUBST) == set(CALLS)
    for ret, name, params in protos:
        t_ret, _, t_params = _lib.SUBST_SIGNATURES[name].partition(":")
        entries = [e.split() if e.strip() != "stream" else ["stream", "stream"] for e in t_params.split(",")]
        decls = [re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*", d).groups() for d in params.split(",")]
        assert test_abi._C_RETURN[t_ret] == ret and [e[1] for e in entries] == [d[2] for d in decls], name
        assert all(test_abi.kind_agrees(kind, ty, bool(star)) for (kind, _), (ty, star, _) in zip(entries, decls)), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.PARSED_SUBST[name][0] and list(fn.argtypes) == [q.ctype for q in _lib.PARSED_SUBST[name][1]], name
    # the tables are hmse_lines_gather's, in the same order; the ABI version stays
    assert _lib.SUBST_SIGNATURES["hmse_subst_apply"].split(" u64*? start")[0] == _lib.SIGNATURES["hmse_lines_gather"].split(" u64*? start")[0]
    assert lib.hmse_abi_version() == 3
    assert "Out of scope" in header and "bit 1" in header and "bit 0" in header and "HMSE_EINVAL" in header
    assert int(re.search(r"#define HMSE_SUBST_FILL\s+(\d+)u", header).group(1)) == 1 and int(re.search(r"#define HMSE_SUBST_LITERAL\s+(\d+)u", header).group(1)) == 0
    from hmse_amd import ops
    assert (ops.SUBST_LITERAL, ops.SUBST_FILL) == (0, 1)


def test_the_library_exports_its_header_and_passes_the_isa_audit():
    """libhmse_subst.so beside libhmse_hip.so: exported == declared in include/hmse_subst.h; no cross-lane instruction inside a divergent
    loop anywhere; no Async / Graph import, no import the pinned list does not allow.  The other four libraries gain no symbol."""
    import json
    from hmse_amd import _lib

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return sorted(x for x in (ln.split()[-1] for ln in out.splitlines() if ln.split()[1:2] and ln.split()[1] in "TW") if not x.startswith("_"))
    assert exported(_lib.SUBST_LIB_PATH) == sorted(CALLS)
    assert exported(_lib.TALLY_LIB_PATH) == sorted(_lib.TALLY_SIGNATURES) and exported(_lib.REGEXA_LIB_PATH) == sorted(_lib.REGEXA_SIGNATURES)
    assert exported(_lib.GUNZIP_LIB_PATH) == sorted(_lib.GUNZIP_SIGNATURES)
    assert not [x for x in exported(_lib.HIP_LIB_PATH) if "subst" in x] and not set(CALLS) & set(_lib.EXPORTED_SYMBOLS)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    rep = isa_audit.audit(_lib.SUBST_LIB_PATH)
    names = " ".join(rep)
    assert "subst_edits_kernel" in names and "subst_apply_kernel" in names and "tables_validate_kernel" in names, names
    assert isa_audit.summary(rep) == {}
    pin = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_audit.json")))
    imports = isa_audit.imported_hip_calls(_lib.SUBST_LIB_PATH)
    assert not [x for x in imports if "Async" in x or "Graph" in x], imports
    assert set(imports) <= set(pin["hip_imports_allowed"]), sorted(set(imports) - set(pin["hip_imports_allowed"]))


def test_no_kernel_of_the_library_uses_scratch_or_spills():
    """A fresh gfx950 cross-compile of subst.hip with the Makefile's switches: the compiler's own resource remarks say no scratch and no
    spill for every kernel, and profiles/subst/kernel_resource_usage.txt is what that compile says."""
    import tempfile
    csrc = os.path.join(ROOT, "hmse_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", make, re.M).group(1)
    flags = re.search(r"^HIPFLAGS \?= (.*)$", make, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH \?= (\S+)", make, re.M).group(1)).split()
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", "subst.hip", "-o", os.path.join(td, "subst.o")], cwd=csrc,
                           capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [re.sub(r" \[-Rpass.*$", "", ln.split("remark: ", 1)[1]) for ln in r.stderr.splitlines() if "remark: " in ln]
    kept = [ln for ln in lines if re.match(r"\s*(Function Name|TotalSGPRs|VGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)", ln)]
    names = [ln for ln in kept if "Function Name" in ln]
    assert len(names) == 4 and sum("subst_apply_kernel" in x for x in names) == 2 and any("subst_edits_kernel" in x for x in names), names
    assert sum(ln.strip() == "ScratchSize [bytes/lane]: 0" for ln in kept) == 4
    assert sum(ln.strip() == "SGPRs Spill: 0" for ln in kept) == 4 and sum(ln.strip() == "VGPRs Spill: 0" for ln in kept) == 4
    recorded = open(os.path.join(ROOT, "profiles", "subst", "kernel_resource_usage.txt")).read().splitlines()
    assert [x.strip() for x in recorded] == [x.strip() for x in kept]


NAMES = ("raw", "raw_bytes", "raw_off", "n_rec", "cuts", "slot", "n_chunks", "start", "end", "sel", "n", "rep", "rep_bytes", "rep_off", "n_rep", "flags",
         "out_off", "out", "out_cap", "status")


def test_the_entry_point_refuses_bad_arguments_with_no_gpu_present():
    """HMSE_EINVAL (-1), never HMSE_EHIP (-3): refused in front of every clear and launch (the pointers are host addresses)"""
    import torch
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr() + (-mem.data_ptr()) % 256
    dflt = dict(raw=b, raw_bytes=64, raw_off=b, n_rec=1, cuts=b, slot=b, n_chunks=1, start=b, end=b, sel=b, n=2, rep=b, rep_bytes=4, rep_off=b, n_rep=1,
                flags=0, out_off=b, out=b, out_cap=64, status=b)
    assert tuple(p.name for p in _lib.PARSED_SUBST["hmse_subst_apply"][1][:-1]) == NAMES
    for kw in (dict(status=None), dict(raw=None), dict(raw_off=None), dict(cuts=None), dict(slot=None), dict(start=None), dict(end=None), dict(sel=None),
               dict(rep=None), dict(rep_off=None), dict(out_off=None), dict(out=None), dict(n=1 << 33), dict(n=(1 << 64) - 1), dict(flags=2), dict(flags=3),
               dict(flags=1 << 31), dict(n_rep=0), dict(n_rep=0, rep_off=None), dict(out_off=None, n=0), dict(status=None, n=0),
               dict(raw_off=None, n_chunks=0, n=0), dict(out_cap=(1 << 31) * 16384), dict(n_rep=(1 << 31) * 256), dict(n_chunks=(1 << 31) * 256)):
        a = {**dflt, **kw}
        assert lib.hmse_subst_apply(*[a[k] for k in NAMES], None) == -1, kw
    assert mem.sum().item() == 0


def test_the_wrapper_and_the_methods_refuse_what_they_should(monkeypatch):
    import torch
    from hmse_amd import find, ops
    u8 = torch.zeros(8, dtype=torch.uint8)
    z = torch.zeros(2, dtype=torch.int64)
    off = torch.tensor([0, 1])
    args = lambda **kw: {**dict(raw=u8, raw_off=z, cuts=z, slot=z[:1], start=z, end=z, sel=z, rep=u8[:1], rep_off=off, out_off=torch.zeros(3, dtype=torch.int64),
                                n_out=8), **kw}
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.subst_apply(**args())
    for nm in ("start", "end", "sel", "rep_off", "out_off", "cuts"):
        with pytest.raises(ops.HmseError, match=f"{nm} must be torch.int64"):
            ops.subst_apply(**args(**{nm: args()[nm].to(torch.int32)}))
    with pytest.raises(ops.HmseError, match="raw must be torch.uint8"):
        ops.subst_apply(**args(raw=u8.to(torch.int8)))
    with pytest.raises(ops.HmseError, match="rep must be torch.uint8"):
        ops.subst_apply(**args(rep=u8.to(torch.int8)))
    for kw in (dict(end=z[:1]), dict(sel=z[:1]), dict(out_off=z), dict(rep_off=z[:0]), dict(slot=z)):
        with pytest.raises(ops.HmseError, match="do not match"):
            ops.subst_apply(**args(**kw))
    with pytest.raises(ops.HmseError, match="edits and no replacement"):
        ops.subst_apply(**args(rep_off=z[:1]))
    with pytest.raises(TypeError, match="takes 20 arguments"):
        ops._call("hmse_subst_apply", 1, 2, 3)
    with pytest.raises(KeyError):
        ops._call("hmse_subst_nothing")
    # the methods, on a finder that no device work made: the refusals come in front of every launch
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("a launch"))
    fd = find.StoreFinder.__new__(find.StoreFinder)
    fd.dev = torch.device("cpu")
    fd.raw, fd.raw_off, fd.cuts, fd.slot, fd.n_bytes = u8, z, z, z[:1], 8
    pair = (torch.tensor([0, 4]), torch.tensor([2, 6]))
    for method, word in ((fd.substitute, "substitute"), (fd.redact, "redact")):
        with pytest.raises(ValueError, match=rf"{word}: what is a Found, which has offsets but no lengths.*spans\(\)"):
            method(find.Found(z, z[:0], z[:1]), b"x")
        with pytest.raises(ValueError, match=r"is a ApproxFound, which has offsets but no lengths.*\(start, end\) pair"):
            method(find.ApproxFound(z, z[:0], z[:1], z[:0]), b"x")
        with pytest.raises(ValueError, match="int64 tensors on the finder's device"):
            method((pair[0].to(torch.int32), pair[1]), b"x")
        with pytest.raises(ValueError, match="one length"):
            method((pair[0], pair[1][:1]), b"x")
        with pytest.raises(ValueError, match="what is a RegexFound, a Lines"):
            method([1, 2], b"x")
        with pytest.raises(ValueError, match="descends or leaves the corpus of n_bytes = 8"):
            method((pair[0], torch.tensor([2, 9])), b"x")
        with pytest.raises(ValueError, match="descends or leaves"):
            method((torch.tensor([2, 4]), torch.tensor([1, 6])), b"x")
        with pytest.raises(ValueError, match="descends or leaves"):
            method((torch.tensor([-1, 4]), torch.tensor([1, 6])), b"x")
        with pytest.raises(ValueError, match="ranges overlap"):
            method((torch.tensor([0, 3]), torch.tensor([4, 6])), b"x")
        with pytest.raises(ValueError, match="ranges overlap"):                   # between groups, found after the merge
            method((torch.tensor([0, 5, 3]), torch.tensor([2, 6, 6]), torch.tensor([0, 2, 3])), [b"x", b"y"])
        with pytest.raises(ValueError, match="ranges overlap"):                   # an insertion inside a range
            method((torch.tensor([0, 1]), torch.tensor([2, 1])), b"x")
        with pytest.raises(ValueError, match="ptr does not split the 2 ranges"):
            method((pair[0], pair[1], torch.tensor([0, 1])), b"x")
        with pytest.raises(ValueError, match="has 3 entries, what has 1 groups"):
            method(pair, [b"x", b"y", b"z"])
        with pytest.raises(ValueError, match="is bytes, or a sequence with one bytes per group"):
            method(pair, "x")
        with pytest.raises(ValueError, match="is bytes, or a sequence"):
            method(pair, [b"x", 3])
    for bad in (b"", b"ab", [b"ab"]):
        with pytest.raises(ValueError, match="fill is one byte"):
            fd.redact(pair, bad)
    with pytest.raises(ValueError, match="the output holds 14 bytes, which exceeds max_bytes = 13"):
        fd.substitute(pair, b"12345", max_bytes=13)
    with pytest.raises(ValueError, match="exceeds max_bytes = 7"):
        fd.redact(pair, b"*", max_bytes=7)
    with pytest.raises(pytest.fail.Exception, match="a launch"):                  # a host tensor reaches the one call path, which would refuse it
        fd.substitute(pair, b"x")


def test_what_reaches_the_kernel_for_an_empty_what_and_for_merged_groups(monkeypatch):
    """No edits still goes through the kernel (the corpus itself: out_off = [n_bytes]); groups are merged by start, stably, and the
    caller's out_off is the definition's."""
    import torch
    from hmse_amd import find, ops
    seen = []

    def fake(raw, raw_off, cuts, slot, start, end, sel, rep, rep_off, out_off, n_out, fill=False):
        seen.append(dict(start=start, end=end, sel=sel, rep=rep, rep_off=rep_off, out_off=out_off, n_out=n_out, fill=fill))
        return torch.zeros(n_out, dtype=torch.uint8)
    monkeypatch.setattr(ops, "subst_apply", fake)
    fd = find.StoreFinder.__new__(find.StoreFinder)
    fd.dev = torch.device("cpu")
    z = torch.zeros(2, dtype=torch.int64)
    fd.raw, fd.raw_off, fd.cuts, fd.slot, fd.n_bytes = torch.zeros(20, dtype=torch.uint8), z, z, z[:1], 20
    e = torch.zeros(0, dtype=torch.int64)
    for what in ((e, e), (e, e, torch.tensor([0, 0, 0])), (e, e, torch.tensor([0])), find.RegexFound(torch.zeros(3, dtype=torch.int64), e, z, e)):
        G = what.ptr.numel() - 1 if isinstance(what, find.RegexFound) else 1 if len(what) == 2 else what[2].numel() - 1
        for fill in (False, True):
            sub = (fd.redact if fill else fd.substitute)(what, [b"x"] * G if G != 1 else b"x")
            a = seen.pop()
            assert not seen and a["n_out"] == 20 and a["fill"] == fill and a["out_off"].tolist() == [20] and a["rep_off"].tolist() == list(range(G + 1))
            assert all(a[k].numel() == 0 and a[k].dtype == torch.int64 for k in ("start", "end", "sel"))
            assert (sub.n_edits, sub.n_bytes_in, sub.n_bytes_out) == (0, 20, 20) and sub.data.numel() == 20 and sub.out_off.tolist() == [20]
            assert sub.translate(torch.tensor([0, 7, 20])).tolist() == [0, 7, 20]
    # three groups, merged: insertions at one place keep the order given (group 0's before group 2's), touching edits pass
    start, end, ptr = torch.tensor([5, 9, 12, 2, 5, 5]), torch.tensor([5, 12, 12, 4, 5, 9]), torch.tensor([0, 3, 4, 6])
    reps = [b"AB", b"", b"xyz"]
    sub = fd.substitute((start, end, ptr), reps)
    a = seen.pop()
    edits = [(2, 4, 1), (5, 5, 0), (5, 5, 2), (5, 9, 2), (9, 12, 0), (12, 12, 0)]
    assert list(zip(a["start"].tolist(), a["end"].tolist(), a["sel"].tolist())) == edits
    corpus = bytes(range(100, 120))
    out, out_off = ref.splice(corpus, edits, reps)
    assert a["out_off"].tolist() == out_off == sub.out_off.tolist() and a["n_out"] == len(out) == sub.n_bytes_out and sub.n_edits == 6
    assert a["rep"].tolist() == list(b"ABxyz") and a["rep_off"].tolist() == [0, 2, 2, 5] and not a["fill"]
    sub = fd.redact((start, end, ptr), [b"A", b"B", b"C"])
    a = seen.pop()
    assert a["out_off"].tolist() == ref.splice(corpus, edits, [b"A", b"B", b"C"], True)[1] == [2, 5, 5, 5, 9, 12, 20] and a["fill"] and sub.n_bytes_out == 20
    sub = fd.substitute((start, end, ptr), b"-")                                 # one for all: every sel is 0
    a = seen.pop()
    assert a["sel"].tolist() == [0] * 6 and a["out_off"].tolist() == ref.splice(corpus, [(s, e, 0) for s, e, _ in edits], [b"-"])[1]


def test_a_short_pass_of_the_kernels_on_cpu_threads():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "subst_emu.py"), "--iters", "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "sweep ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    src = open(os.path.join(ROOT, "hmse_amd", "csrc", "subst.hip")).read()
    for word in ("gridDim", "atomicAdd"):                                         # every grid covers its work outright
        assert word not in src.split("// ---- entry points")[0].split("constexpr int SUBST_NT")[1]
