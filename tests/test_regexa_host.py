"""CPU: the regex compiler with assertions (hmse_amd.regex.Regex(assertions=True): ^ $ \\A \\Z \\b \\B) against the `re` oracle of
tests/regexa_ref.py — every start of every small buffer, the refusals with their offsets, the invariants of the compiled form — then the
new header include/hmse_regexa.h against _lib (prototypes, struct layout, exported symbols), the entry points' own refusals (HMSE_EINVAL
in front of every HIP call) and the kernels on the CPU (tools/regexa_emu.py)."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import regexa_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmse_regexa.h")
CALLS = ("hmse_regexa_scan", "hmse_regexa_seams")
ASSERTIONS = [b"^", b"$", rb"\A", rb"\Z", rb"\b", rb"\B"]
ATOMS = [b"a", b"[ab]+", b".", b"-?b"]
GROUPS = [rb"(^|b)a", rb"a($|b)", rb"(\b|a)*b", rb"^.*$", rb"(a|^)(b|$)", rb"(^|-)*a", rb"(?:a\b|-\B)+", rb"^^a$$", rb"a\Z|\Ab", rb"\n^a", rb"a$\n",
          rb"(^a|\bb)+", rb"^\b[ab]{2,3}\b", rb"\w+$", rb"^\W", rb".\b."]
ALPHABET = b"ab-\n"
SMALL = [bytes(t) for n in range(7) for t in itertools.product(ALPHABET, repeat=n)]     # every buffer of length <= 6: 5461


def _regex(pattern, **kw):
    from hmse_amd.regex import Regex
    return Regex(pattern, assertions=True, **kw)


def _built(x):
    """the assertion in front of, behind and inside the atoms"""
    return [x + a for a in ATOMS] + [a + x for a in ATOMS] + [a + x + b for a, b in zip(ATOMS, ATOMS[1:] + ATOMS[:1])]


def _check(pattern, buffers, ic=False, dotall=False):
    """match_all of the compiled pattern against the oracle on every start of every buffer; a pattern the compiler refuses
    as never matching must have no occurrence anywhere.  -> the number of occurrences seen."""
    from hmse_amd.regex import RegexError
    orc = ref.Oracle(pattern, ic, dotall)
    try:
        r = _regex(pattern, ignore_case=ic, dotall=dotall)
    except RegexError as e:
        assert "matches nothing but the empty string" in str(e), (pattern, e)
        for buf in buffers:
            assert not any(orc.length_at(buf, o, 256) for o in range(len(buf))), (pattern, buf)
        return 0
    seen = 0
    for buf in buffers:
        want = [orc.length_at(buf, o, r.reach) for o in range(len(buf))]
        got = r.match_all(buf).tolist()
        assert got == want, (pattern, buf, got, want)
        seen += sum(1 for l in want if l)
    return seen


def _random_buffers(seed, n, alphabet=b"aab--\n\n Ab_"):
    rnd = random.Random(seed)
    return [bytes(rnd.choice(alphabet) for _ in range(rnd.randint(7, 40))) for _ in range(n)]


# ---- the compiler against `re` -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", ASSERTIONS)
def test_every_small_buffer_with_the_assertion_in_front_behind_and_inside(x):
    seen = sum(_check(p, SMALL) for p in _built(x))
    assert seen > 1000


def test_groups_of_assertions_on_every_small_buffer():
    for p in GROUPS:
        assert _check(p, SMALL) > 0, p


def test_match_all_and_match_at_agree_and_longer_buffers_with_the_flags_on_and_off():
    bufs = _random_buffers(5, 40)
    for p in [q for x in ASSERTIONS for q in _built(x)] + GROUPS:
        for ic, dotall in ((False, False), (True, False), (False, True), (True, True)):
            _check(p, bufs[:12] if ic != dotall else bufs, ic, dotall)
    r = _regex(rb"(^|b)a\b")
    for buf in SMALL[:400] + bufs:
        assert r.match_all(buf).tolist() == [r.match_at(buf, o) for o in range(len(buf))]
    assert r.match_all(b"").tolist() == []


def test_long_matches_and_the_look_ahead_at_reach():
    """a{256}$ and friends: the flag of the read at i = reach decides; `re` on the whole buffer is the judge."""
    for p, buf in ((rb"a{256}$", b"a" * 256 + b"\n" + b"a" * 257 + b"-" + b"a" * 256), (rb"a{256}\b", b"-" + b"a" * 256 + b"-" + b"a" * 256 + b"b"),
                   (rb"a{255}\B", b"a" * 300 + b"-" + b"a" * 255), (rb"q+\b", b"q" * 300 + b" " + b"q" * 5 + b"_")):
        r = _regex(p)
        orc = ref.Oracle(p)
        starts = list(range(0, len(buf), 7)) + list(range(max(len(buf) - 300, 0), len(buf)))
        got = r.match_all(buf)
        for o in starts:
            assert got[o] == orc.length_at(buf, o, r.reach), (p, o)
        assert got.max() >= 255


def test_assertion_free_patterns_compile_to_the_plain_answers():
    from hmse_amd.regex import Regex
    bufs = _random_buffers(9, 60, b"abcAB\n q7.") + SMALL[::37]
    for p, ic, dotall in ((b"ab", False, False), (b"a+b*", True, False), (rb"[ab]{2,5}", False, False), (rb"a.{0,7}b", False, True), (rb"\w+\s", False, False),
                          (rb"(ab|b)c?", True, False), (rb"[^\n]*c", False, False), (rb"b{255}a", False, False), (rb".", False, False)):
        plain, asserting = Regex(p, ic, dotall), Regex(p, ic, dotall, assertions=True)
        assert asserting.asserting and not plain.asserting and plain.start == (1, 1, 1, 1) and plain.edge_class is None
        assert (asserting.reach, asserting.min_len) == (plain.reach, plain.min_len), p
        for buf in bufs + [b"b" * 255 + b"a", b"ab" * 200]:
            assert asserting.match_all(buf).tolist() == plain.match_all(buf).tolist(), (p, buf)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_offsets():
    from hmse_amd.regex import Regex, RegexError
    for p, off in ((rb"^*a", 1), (rb"a\b+", 3), (rb"a$?", 2), (rb"\B{2}a", 2), (rb"a[\b]", 2), (rb"a\z", 1), (rb"\Ga", 0), (rb"a(?=b)", 1), (rb"(?<!a)b", 0),
                   (rb"(?m)^a", 0), (rb"^a(", 2), (rb"a\Z*", 3)):
        with pytest.raises(RegexError) as e:
            _regex(p)
        assert e.value.offset == off, (p, str(e.value))
    for p in (rb"a^b", rb"^$", rb"\b\B.", rb"a\Ab", rb"\Z.", rb"(^|$)", rb"\w\b\w"):        # nothing non-empty can match
        with pytest.raises(RegexError, match="matches nothing but the empty string"):
            _regex(p)
    for p, off in ((b"^a", 0), (b"a$", 1), (b"a|^b", 2), (rb"\ba", 0), (rb"a\Z", 1)):       # the default refuses what it refused
        with pytest.raises(RegexError) as e:
            Regex(p)
        assert e.value.offset == off
    _regex(rb"(^|,)*a")                                                                    # a group that holds an assertion may be quantified
    _regex(rb"(\b)+a")
    _regex(rb"\^a\$")                                                                      # escaped: literals


# ---- the compiled form -------------------------------------------------------------------------------------------------------------------
def test_table_invariants():
    from hmse_amd import regex as R
    for p in [q for x in ASSERTIONS for q in _built(x)] + GROUPS + [rb"\bcat\b", rb"^ERROR", rb";$", rb"\A\w+|\w+\Z"]:
        for ic in (False, True):
            try:
                r = _regex(p, ignore_case=ic)
            except R.RegexError:
                continue
            nc, ns = r.n_classes, r.n_states
            tab = r.table.astype(np.int64).reshape(ns, nc)
            assert r.table.dtype == np.uint16 and r.classmap.dtype == np.uint8 and r.classmap.shape == (256,)
            assert (tab[0] == 0).all()                                                     # the dead row, flags included
            assert ((tab[:, nc - 1] & 0x7FFF) == 0).all() and r.edge_class == nc - 1       # the EDGE column leads nowhere
            assert ((tab & 0x7FFF) < ns).all() and int(r.classmap.max()) == nc - 2         # no byte maps to EDGE; every class is used
            kinds = {}
            for b in range(256):
                kinds.setdefault(int(r.classmap[b]), set()).add(R.byte_kind(b))
            assert all(len(k) == 1 for k in kinds.values())                                # classes refine kinds
            assert kinds[int(r.classmap[0x0A])] == {R.NL} and (r.classmap == r.classmap[0x0A]).sum() == 1
            assert len(r.start) == 4 and all(1 <= s < ns for s in r.start)
            # the flag depends on (state, kind of the class) only
            kind_of_class = [next(iter(kinds[c])) for c in range(nc - 1)] + [R.EDGE]
            for k in range(4):
                cols = [c for c in range(nc) if kind_of_class[c] == k]
                assert all(len({int(tab[s, c]) >> 15 for c in cols}) <= 1 for s in range(ns))
            assert 1 <= r.min_len <= r.reach <= 256
            again = _regex(p, ignore_case=ic)                                              # deterministic
            assert again.table.tobytes() == r.table.tobytes() and again.classmap.tobytes() == r.classmap.tobytes()
            assert (again.start, again.reach, again.min_len, again.n_states, again.n_classes) == (r.start, r.reach, r.min_len, ns, nc)
    r = _regex(rb"\Aab")
    assert r.start[0] != r.start[1] == r.start[2] == r.start[3] and not r.table.reshape(r.n_states, -1)[r.start[1]].any()


def test_the_caps():
    from hmse_amd.regex import HMSE_REGEX_MAX_TABLE, RegexError
    r = _regex(rb"\b[a-z]{200,256}\b")
    assert r.n_states * r.n_classes <= HMSE_REGEX_MAX_TABLE and r.reach == 256
    with pytest.raises(RegexError, match="table entries"):
        _regex(rb"^[ab]*a[ab]{11}$")                                                       # 2^12 subsets x 6 classes
    with pytest.raises(RegexError, match="positions"):
        _regex(rb"^(abcdefghijklmnopq){256}$")
    with pytest.raises(RegexError, match="more than HMSE_REGEX_MAX_LEN"):
        _regex(rb"^a{256}b")
    with pytest.raises(RegexError, match="bytes"):
        _regex("^a")


# ---- the header, the library, the entry points ---------------------------------------------------------------------------------------------
def test_prototypes_and_struct_layout_equal_the_header(tmp_path):
    import test_abi
    import test_abi_layout
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    header = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = re.findall(r"^(\w+) (hmse_[a-z0-9_]+)\(([^;]*)\);", plain, re.M)
    assert [name for _, name, _ in protos] == list(_lib.REGEXA_SIGNATURES) == list(CALLS)
    assert not set(_lib.REGEXA_SIGNATURES) & set(_lib.PARSED) and set(_lib.PARSED_REGEXA) == set(CALLS)
    for ret, name, params in protos:
        t_ret, _, t_params = _lib.REGEXA_SIGNATURES[name].partition(":")
        entries = [e.split() if e.strip() != "stream" else ["stream", "stream"] for e in t_params.split(",")]
        decls = [re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*", d).groups() for d in params.split(",")]
        assert test_abi._C_RETURN[t_ret] == ret and [e[1] for e in entries] == [d[2] for d in decls], name
        assert all(test_abi.kind_agrees(kind, ty, bool(star)) for (kind, _), (ty, star, _) in zip(entries, decls)), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.PARSED_REGEXA[name][0] and list(fn.argtypes) == [q.ctype for q in _lib.PARSED_REGEXA[name][1]], name
    # the argument lists are hmse_regex_scan's / hmse_regex_seams' with the other header struct
    for name in CALLS:
        assert _lib.REGEXA_SIGNATURES[name].replace("hmse_regexa*", "hmse_regex*") == _lib.SIGNATURES[name.replace("regexa", "regex")]
    fields = [f.split("[")[0] for f in test_abi_layout._struct_fields(header, "hmse_regexa")]
    assert fields == [f[0] for f in _lib.HmseRegexa._fields_]
    lines = ['#include <stdio.h>', '#include "hmse_regexa.h"', 'int main(void) {', '  printf("sizeof %zu\\n", sizeof(hmse_regexa));']
    lines += [f'  printf("{f} %zu\\n", offsetof(hmse_regexa, {f}));' for f in fields] + ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("sizeof")) == C.sizeof(_lib.HmseRegexa) == 48
    assert {f: int(v) for f, v in got.items()} == {f: getattr(_lib.HmseRegexa, f).offset for f in fields}
    kinds = {k: int(v) for k, v in re.findall(r"#define HMSE_REGEXA_(EDGE|NL|WORD|OTHER)\s+(\d)u", header)}
    from hmse_amd import regex as R
    assert kinds == {"EDGE": R.EDGE, "NL": R.NL, "WORD": R.WORD, "OTHER": R.OTHER} == {"EDGE": 0, "NL": 1, "WORD": 2, "OTHER": 3}


def test_the_library_exports_its_header_and_passes_the_isa_audit():
    """libhmse_regexa.so beside libhmse_hip.so: exported == declared in include/hmse_regexa.h; no cross-lane instruction inside a loop that
    lanes leave at different times; no Async / Graph import, no import the pinned list does not allow.  The two other libraries gain
    no symbol."""
    import json
    from hmse_amd import _lib
    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return sorted(x for x in (ln.split()[-1] for ln in out.splitlines() if ln.split()[1:2] and ln.split()[1] in "TW") if not x.startswith("_"))
    assert exported(_lib.REGEXA_LIB_PATH) == sorted(CALLS)
    assert exported(_lib.GUNZIP_LIB_PATH) == sorted(_lib.GUNZIP_SIGNATURES)
    assert not [x for x in exported(_lib.HIP_LIB_PATH) if "regexa" in x] and not set(CALLS) & set(_lib.EXPORTED_SYMBOLS)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    rep = isa_audit.audit(_lib.REGEXA_LIB_PATH)
    assert {"regexa_validate_kernel", "regexa_scan_kernel", "regexa_seams_kernel"} <= set(rep)
    assert rep["regexa_scan_kernel"]["loops"] > 5 and isa_audit.summary(rep) == {}
    pin = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_audit.json")))
    imports = isa_audit.imported_hip_calls(_lib.REGEXA_LIB_PATH)
    assert not [x for x in imports if "Async" in x or "Graph" in x], imports
    assert set(imports) <= set(pin["hip_imports_allowed"]), sorted(set(imports) - set(pin["hip_imports_allowed"]))


def test_entry_points_refuse_bad_headers_and_null_arguments_with_no_gpu_present():
    """HMSE_EINVAL (-1), never HMSE_EHIP (-3): refused in front of every clear and launch (the pointers are host addresses)"""
    import torch
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr() + (-mem.data_ptr()) % 256
    good = dict(struct_size=C.sizeof(_lib.HmseRegexa), n_states=4, n_classes=5, reach=3, start=(1, 1, 2, 3), table=b, classmap=b)

    def hdr(**kw):
        f = {**good, **kw}
        return _lib.HmseRegexa(f["struct_size"], f["n_states"], f["n_classes"], f["reach"], (C.c_uint32 * 4)(*f["start"]), f["table"], f["classmap"])
    scan_names = ("raw", "raw_bytes", "raw_off", "n_rec", "mult", "rx", "hits", "hits_cap", "n_hits", "count", "status")
    seam_names = ("raw", "raw_bytes", "raw_off", "n_rec", "cuts", "slot", "n_chunks", "rx", "hits", "hits_cap", "n_hits", "count", "status")
    dflt = dict(raw=b, raw_bytes=64, raw_off=b, n_rec=1, mult=None, cuts=b, slot=b, n_chunks=1, hits=b, hits_cap=4, n_hits=b, count=b, status=b)

    def call(fn, names, h, **kw):
        a = {**dflt, **kw, "rx": C.byref(h) if h is not None else None}
        return fn(*[a[k] for k in names], None)
    both = ((lib.hmse_regexa_scan, scan_names), (lib.hmse_regexa_seams, seam_names))
    bad_headers = [dict(struct_size=32), dict(struct_size=24), dict(n_states=1), dict(n_states=32768), dict(n_classes=1), dict(n_classes=0), dict(n_classes=257),
                   dict(n_states=4096, n_classes=5), dict(reach=0), dict(reach=257), dict(table=None), dict(classmap=None),
                   dict(start=(0, 1, 1, 1)), dict(start=(1, 1, 1, 4)), dict(start=(1, 1 << 31, 1, 1)), dict(start=(1, 1, 0, 1))]
    for fn, names in both:
        for kw in bad_headers:
            assert call(fn, names, hdr(**kw)) == -1, kw
        assert call(fn, names, None) == -1
        for kw in (dict(n_hits=None), dict(count=None), dict(status=None)):
            assert call(fn, names, hdr(), **kw) == -1, kw
    assert call(*both[0], hdr(), raw_off=None) == -1 and call(*both[0], hdr(), raw=None) == -1 and call(*both[0], hdr(), raw_bytes=1 << 56) == -1
    for kw in (dict(cuts=None), dict(slot=None), dict(raw_off=None), dict(raw=None), dict(n_chunks=(1 << 40) + 1)):
        assert call(*both[1], hdr(), **kw) == -1, kw
    assert mem.sum().item() == 0


def test_wrappers_refuse_host_tensors_and_go_through_the_one_call_path(monkeypatch):
    import torch
    from hmse_amd import _lib, ops
    from hmse_amd.regex import Regex
    h = Regex(rb"\bab\b", assertions=True)
    rx = ops.RegexA(torch.from_numpy(h.table.view(np.int16).copy()), torch.from_numpy(h.classmap.copy()), h.n_states, h.n_classes, h.reach, h.start)
    hd = rx.header()
    assert (hd.struct_size, hd.n_states, hd.n_classes, hd.reach, tuple(hd.start)) == (48, h.n_states, h.n_classes, h.reach, h.start)
    z = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.regexa_scan(torch.zeros(8, dtype=torch.uint8), z, None, rx)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.regexa_seams(torch.zeros(8, dtype=torch.uint8), z, z, z[:1], rx)
    with pytest.raises(TypeError, match="takes 11 arguments"):
        ops._call("hmse_regexa_scan", 1, 2, 3)
    with pytest.raises(KeyError):
        ops._call("hmse_regexa_nothing")
    assert h.rx is None and h.dev is None and set(_lib.PARSED_REGEXA) == set(CALLS)


# ---- the kernels on the CPU ---------------------------------------------------------------------------------------------------------------
def test_the_emulator_builds_and_its_cases_pass():
    """tools/regexa_emu.py: the kernels of regex_core.h in their asserting form, one std::thread per lane, against a brute-force walk with the real context
    bytes; the first five cases damage the automaton in the five ways status bit 2 names (no sanitizer here)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "regexa_emu.py"), "--iters", "6"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "6 cases ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
