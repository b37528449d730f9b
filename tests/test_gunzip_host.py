"""CPU: the reference of the gzip import (tests/gunzip_ref.py: the zlib chain, the byte filter, the header parser, the measured end of a
candidate) against Python's gzip, the cases the GPU tests rest on (the nested file, the mutation seed), the entry points' own refusals
(HMSE_EINVAL in front of every HIP call), the symbols and prototypes of include/hmse_gunzip.h against _lib.GUNZIP_SIGNATURES, the
wrappers' refusal of host tensors and their pointers, and the kernels on the CPU (tools/gunzip_emu.py)."""
import ctypes as C
import gzip
import io
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import gunzip_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("hmse_gzip_candidates", "hmse_gzip_measure")


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def test_the_chain_reads_what_gzip_writes():
    parts = [ref.text(1, 5000), b"", ref.text(2, 70_000), b"x"]
    buf = io.BytesIO()
    for i, p in enumerate(parts):                                                      # one file, appended to
        with gzip.GzipFile(filename=f"part{i}", fileobj=buf, mode="ab", compresslevel=(1, 6, 9, 6)[i], mtime=i) as f:
            f.write(p)
    blob = buf.getvalue()
    got = ref.chain(blob)
    assert [raw for _, _, raw in got] == parts and gzip.decompress(blob) == b"".join(parts)
    assert got[0][0] == 0 and all(a + s == b for (a, s, _), (b, _, _) in zip(got, got[1:])) and got[-1][0] + got[-1][1] == len(blob)
    assert [o for o, _, _ in got] == [p for p in ref.candidates(blob) if ref.measure(blob, p)["valid"]][:4] == ref.candidates(blob)[:4]
    for (o, size, raw) in got:
        m = ref.measure(blob, o)
        assert (m["valid"], m["fast"], m["end"], m["raw_len"], m["crc"]) == (True, False, o + size, len(raw), zlib.crc32(raw))
        assert blob[m["stream_off"] - 6: m["stream_off"]] == b"part%d\0" % [o for o, _, _ in got].index(o)
    assert ref.chain(b"") == [] and ref.outcome(b"") == []
    for bad, member, offset in ((b"junk" + blob, 0, 0), (blob + b"\0", 4, len(blob)), (blob[:-1], 3, got[3][0]), (blob[:got[2][0] + 100], 2, got[2][0])):
        with pytest.raises(ref.Refused) as e:
            ref.chain(bad)
        assert (e.value.member, e.value.offset) == (member, offset)


def test_the_byte_filter_and_the_header_parser():
    m = ref.member(b"abc")
    assert len(ref.member(b"")) == 20 == ref.MIN_MEMBER and ref.candidates(ref.member(b"")) == [0]
    assert ref.candidates(m + m) == [0, len(m)] and ref.candidates((m + m)[:-1]) == [0, len(m)] and ref.candidates(b"\0" * 3 + m[:19]) == []
    for flg, want in ((0x00, [0]), (0x1F, [0]), (0x20, []), (0x40, []), (0x80, []), (0xE4, [])):
        assert ref.candidates(b"\x1f\x8b\x08" + bytes([flg]) + bytes(16)) == want
    assert ref.candidates(b"\x1f\x8b\x08\x00" * 6) == [0, 4] and ref.candidates(b"\x1f\x8b\x08\x1f\x8b\x08\x00" + bytes(16)) == [0, 3]
    # every combination of the optional fields: the parser finds the stream, zlib agrees with the whole
    raw = ref.text(3, 300)
    for extra in (None, b"", b"AB\x03\x00xyzCD\x00\x00"):
        for name in (None, b"a name"):
            for comment in (None, b"", b"c" * 200):
                for hcrc in (False, True):
                    mem = ref.member(raw, 6, extra=extra, name=name, comment=comment, hcrc=hcrc)
                    why, q, bsize1 = ref.parse_header(mem, 0)
                    assert (why, bsize1) == (0, 0) and zlib.decompress(mem[q:-8], wbits=-15) == raw and zlib.decompress(mem, wbits=31) == raw
                    if hcrc:
                        broken = bytearray(mem); broken[q - 1] ^= 0x10
                        assert ref.parse_header(bytes(broken), 0)[0] == ref.WHY_HEADER
                        with pytest.raises(zlib.error, match="header crc mismatch"):
                            zlib.decompress(bytes(broken), wbits=31)
    with pytest.raises(zlib.error, match="unknown header flags"):
        zlib.decompress(b"\x1f\x8b\x08\x20" + m[4:], wbits=31)
    z = ref.bgzf_member(raw)
    assert ref.parse_header(z, 0) == (0, 18, len(z)) and ref.measure(z, 0)["fast"] and ref.measure(z, 0)["end"] == len(z)
    assert ref.measure(z + z, 0)["end"] == len(z) and not ref.measure(z[:-1], 0)["valid"]
    import export_ref
    assert ref.measure(export_ref.BGZF_EOF, 0) == dict(valid=True, fast=True, why=0, stream_off=18, end=28, raw_len=0, crc=0, flags=3)
    assert ref.measure(ref.bgzf_member(raw, bsize=20), 0)["fast"] is False and ref.measure(ref.bgzf_member(raw, bsize=20), 0)["valid"]


def test_the_nested_file_has_six_candidates_and_four_members():
    blob, raws = ref.nested_case()
    cands, members = ref.candidates(blob), ref.chain(blob)
    assert len(cands) == 6 and len(members) == 4 and [r for _, _, r in members] == raws and gzip.decompress(blob) == b"".join(raws)
    assert all(ref.measure(blob, p)["valid"] for p in cands)                           # the inner members are whole members — elsewhere
    assert len(raws[0]) == len(blob[:members[0][1]]) - 10 - 5 - 8 and raws[3].__len__() == 200_000      # one stored block around them


def test_the_mutation_seed_gives_both_outcomes():
    base = ref.mutation_file()
    assert len(ref.chain(base)) == 6 and b"BC" not in base
    cases = ref.mutations()
    verdicts = [ref.outcome(b) for b, _ in cases]
    assert len(cases) == ref.N_MUTATIONS == 200 and all(len(b) == len(base) and sum(x != y for x, y in zip(b, base)) == 1 for b, _ in cases)
    assert sum(v is not None for v in verdicts) >= 10 and sum(v is None for v in verdicts) >= 10


# ---- the C boundary -----------------------------------------------------------------------------------------------------------------------
def test_symbols_and_prototypes():
    from hmse_amd import _lib, ops
    lib = _lib.hip_lib()
    header = open(os.path.join(ROOT, "include", "hmse_gunzip.h")).read()
    # the table of the import's entry points is that header: names, order, kinds (tests/test_abi.py does the same for include/hmse.h)
    import test_abi
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = re.findall(r"^(\w+) (hmse_[a-z0-9_]+)\(([^;]*)\);", plain, re.M)
    assert [name for _, name, _ in protos] == list(_lib.GUNZIP_SIGNATURES) == ["hmse_gzip_workspace_bytes"] + list(CALLS)
    assert not set(_lib.GUNZIP_SIGNATURES) & set(_lib.SIGNATURES) and set(_lib.PARSED) == set(_lib.SIGNATURES) | set(_lib.GUNZIP_SIGNATURES)
    for ret, name, params in protos:
        t_ret, _, t_params = _lib.GUNZIP_SIGNATURES[name].partition(":")
        entries = [e.split() if e.strip() != "stream" else ["stream", "stream"] for e in t_params.split(",")]
        decls = [re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*", d).groups() for d in params.split(",")]
        assert test_abi._C_RETURN[t_ret] == ret and [e[1] for e in entries] == [d[2] for d in decls], name
        assert all(test_abi.kind_agrees(kind, ty, bool(star)) for (kind, _), (ty, star, _) in zip(entries, decls)), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.PARSED[name][0] and list(fn.argtypes) == [q.ctype for q in _lib.PARSED[name][1]], name
    for name in CALLS:
        fn = getattr(lib, name)
        proto = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M).group(1).split(",")
        assert fn.restype is C.c_int and len(proto) == len(fn.argtypes), name
        assert proto[-1].split()[-1] == "stream"
    assert [len(getattr(lib, n).argtypes) for n in CALLS] == [9, 13]
    consts = {k: int(v) for k, v in re.findall(r"#define HMSE_GZIP_(VALID|FAST|WHY_SHIFT|WHY_HEADER|WHY_STREAM|WHY_LENGTH|WHY_BOUNDS) (\d+)u?", header)}
    assert (consts["VALID"], consts["FAST"], consts["WHY_SHIFT"]) == (ops.GZIP_VALID, ops.GZIP_FAST, ops.GZIP_WHY_SHIFT) == (ref.VALID, ref.FAST, ref.WHY_SHIFT)
    assert {consts["WHY_" + v.upper()]: v for v in ops.GZIP_WHY.values()} == ops.GZIP_WHY
    assert (ref.WHY_HEADER, ref.WHY_STREAM, ref.WHY_LENGTH, ref.WHY_BOUNDS) == (1, 2, 3, 4) and ops.GZIP_MIN_MEMBER == ref.MIN_MEMBER
    assert lib.hmse_abi_version() == 3
    # the workspace: a u32 per tile of 16384 positions and one more, in 256-byte pieces, and the pull counter's piece
    assert [ops.gzip_workspace_bytes(n) for n in (0, 19, 20, 16384 + 19, 16384 + 20, 63 * 16384 + 19, 63 * 16384 + 20)] == [512, 512, 512, 512, 512, 512, 768]
    src = open(os.path.join(ROOT, "hmse_amd", "csrc", "gunzip.hip")).read()
    assert "constexpr int GZ_TILE = GZ_NT * GZ_PER * GZ_TRIPS;" in src and '#include "inflate_core.h"' in src
    core = open(os.path.join(ROOT, "hmse_amd", "csrc", "inflate_core.h")).read()
    inflate = open(os.path.join(ROOT, "hmse_amd", "csrc", "l1_inflate.hip")).read()
    for one_copy in ("struct Bits", "struct LaneCode", "bool build_table(", "uint32_t decode_sym("):     # the decoders share the core
        assert core.count(one_copy) == 1 and one_copy not in src and one_copy not in inflate


def test_the_import_library_exports_its_header_and_passes_the_isa_audit():
    """libhmse_gunzip.so beside libhmse_hip.so: exported == declared in include/hmse_gunzip.h, and what tests/test_host.py asks of the other
    library's kernels — no cross-lane instruction inside a divergent loop (here none at all: nothing is pinned for these kernels in
    tests/golden/isa_audit.json), no Async / Graph import, no import the pinned list does not allow."""
    import json
    from hmse_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.GUNZIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[1:2] and ln.split()[1] in "TW"}
    assert sorted(x for x in exported if not x.startswith("_")) == sorted(_lib.GUNZIP_SIGNATURES)
    assert not set(_lib.GUNZIP_SIGNATURES) & set(_lib.EXPORTED_SYMBOLS)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    rep = isa_audit.audit(_lib.GUNZIP_LIB_PATH)
    assert {"gz::candidates_count_kernel", "gz::candidates_compact_kernel", "gz::measure_kernel"} <= set(rep)
    assert rep["gz::measure_kernel"]["loops"] > 20 and isa_audit.summary(rep) == {}
    pin = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_audit.json")))
    imports = isa_audit.imported_hip_calls(_lib.GUNZIP_LIB_PATH)
    assert not [x for x in imports if "Async" in x or "Graph" in x], imports
    assert set(imports) <= set(pin["hip_imports_allowed"]), sorted(set(imports) - set(pin["hip_imports_allowed"]))


def test_entry_points_refuse_null_and_inconsistent_arguments_with_no_gpu_present():
    """HMSE_EINVAL (-1) / HMSE_ENOSPC, never HMSE_EHIP (-3): refused in front of every clear and launch (the pointers are host addresses)"""
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr() + (-mem.data_ptr()) % 256
    names = ("data", "n", "cand_off", "cap", "count", "status", "ws", "ws_bytes")
    dflt = dict(data=b, n=100, cand_off=b, cap=4, count=b, status=b, ws=b, ws_bytes=1024)
    cand = lambda **kw: lib.hmse_gzip_candidates(*[{**dflt, **kw}[k] for k in names], None)
    for kw in (dict(status=None), dict(count=None), dict(data=None), dict(cand_off=None), dict(n=(1 << 40) + 1), dict(ws=b + 8), dict(status=None, n=0)):
        assert cand(**kw) == -1, kw
    enospc = cand(ws_bytes=256)
    assert enospc not in (0, -1, -3) and cand(ws=None) == enospc
    names = ("data", "n", "cand_off", "n_cand", "stream_off", "end", "raw_len", "crc", "flags", "status", "ws", "ws_bytes")
    dflt = dict(data=b, n=100, cand_off=b, n_cand=2, stream_off=b, end=b, raw_len=b, crc=b, flags=b, status=b, ws=b, ws_bytes=1024)
    meas = lambda **kw: lib.hmse_gzip_measure(*[{**dflt, **kw}[k] for k in names], None)
    for kw in [dict(status=None), dict(data=None), dict(n=(1 << 40) + 1), dict(n_cand=1 << 31), dict(ws=b + 16), dict(status=None, n_cand=0)] + \
              [{k: None} for k in ("cand_off", "stream_off", "end", "raw_len", "crc", "flags")]:
        assert meas(**kw) == -1, kw
    assert meas(ws_bytes=511) == enospc and meas(ws=None) == enospc
    assert mem.sum().item() == 0


def test_wrappers_refuse_host_tensors_and_bad_sources():
    from hmse_amd import gunzip, ops
    data = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.gzip_candidates(data, 4)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.gzip_measure(data, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        gunzip.from_gzip(ref.member(b"abc"), torch.device("cpu"))
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.uint8), np.zeros(4, np.int16)):
        with pytest.raises(TypeError):
            gunzip.from_gzip(bad, torch.device("cpu"))
    assert issubclass(gunzip.GunzipError, ValueError)
    e = gunzip.GunzipError(3, 1234, "CRC-32 mismatch")
    assert (e.member, e.offset) == (3, 1234) and "member 3 at offset 1234" in str(e)
    empty = gunzip.from_gzip(b"", torch.device("cpu"))                                  # no member: nothing to launch
    assert (empty.n_members, empty.n_candidates, empty.n_bgzf, empty.crc32) == (0, 0, 0, 0)
    assert empty.raw.numel() == 0 and empty.cuts.tolist() == [0] and empty.member_off.tolist() == [0]


def test_the_chain_follows_ends_from_offset_zero():
    """gunzip._on_chain on the CPU: successors with the two sentinels at the end; marks = what node 0 reaches"""
    from hmse_amd import gunzip
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    assert gunzip._on_chain(t(2, 2, 4, 5, 5, 5, 6)).tolist() == [True, False, True, False, True, True, False]       # 0 -> 2 -> 4 -> END
    assert gunzip._on_chain(t(1, 3, 2, 3)).tolist() == [True, True, False, True]                                   # 0 -> 1 -> DEAD
    n = 1000                                                                           # a chain of every second node, the others lead into it
    nxt = torch.arange(n + 2, dtype=torch.int64)
    nxt[:n] = torch.arange(n) + 2 - (torch.arange(n) % 2)
    nxt[n - 2], nxt[n - 1] = n, n
    mark = gunzip._on_chain(nxt)
    assert mark[:n].tolist() == [i % 2 == 0 for i in range(n)] and mark[n].item() and not mark[n + 1].item()


def test_every_pointer_the_wrappers_hand_to_the_library_comes_from_the_arena(monkeypatch):
    import arena as A
    from hmse_amd import ops
    lib = A.record(monkeypatch, CALLS)
    ar = A.Arena(torch.device("cpu"), "zero", seed=5).install(monkeypatch)
    data = ar.place(np.frombuffer(ref.member(b"abc") * 3, np.uint8).copy(), misalign=3)
    ops.gzip_candidates(data, 7)
    ops.gzip_measure(data, ar.place(np.array([0, 23], np.int64)))
    assert [c[0] for c in lib.calls] == list(CALLS)
    for name, ptrs, args in lib.calls:
        assert ptrs and all(ar.contains(q) for q in ptrs), (name, [hex(q) for q in ptrs if not ar.contains(q)])
    assert lib.calls[0][2][1] == 69 and lib.calls[0][2][3] == 7 and lib.calls[0][2][7] == 512 and lib.calls[1][2][3] == 2
    ar.check()


# ---- the kernels on the CPU ---------------------------------------------------------------------------------------------------------------
def test_the_emulator_builds_and_its_cases_pass():
    """tools/gunzip_emu.py: the kernels cut out of gunzip.hip over inflate_core.h, one std::thread per lane, against the byte filter and
    against zlib's answers (no sanitizer here)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gunzip_emu.py"), "--iters", "3", "--seed", "4242"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout and re.search(r"known answers \(zlib\): 14 cases, \d+ candidates, 0 wrong", r.stdout), \
        r.stdout[-2000:] + r.stderr[-2000:]
