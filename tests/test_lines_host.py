"""CPU: lines of a hit (hmse_amd.find lines / text / grep; hmse_lines_extent / hmse_lines_gather) — the plain-Python reference against the
bytes.split statement of the contract, the cut flags, the invariants of Lines, and everything the product refuses before it needs a
device: the entry points' HMSE_EINVAL cases through ctypes, host tensors, bad arguments.  The kernels' source runs on CPU threads against
the brute-force definition (tools/lines_emu.py)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import find_ref
import lines_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def test_reference_equals_the_split_statement_when_nothing_is_cut():
    """1500 random corpora over {a, b, d, d} of 1..60 bytes, EVERY offset, before and after 0..3, a reach no line reaches."""
    rng = np.random.default_rng(1)
    d = ord("d")
    for it in range(1500):
        n = int(rng.integers(1, 61))
        corpus = bytes(rng.choice(np.frombuffer(b"abdd", np.uint8), n))
        b, a = (int(v) for v in rng.integers(0, 4, 2))
        for o in range(n):
            s, e, f = ref.extent(corpus, o, d, b, a, 1 << 16)
            assert (s, e) == ref.split_extent(corpus, o, d, b, a) and f == 0, (corpus, o, b, a)
            assert d not in corpus[s:e] or b + a > 0
            assert corpus[s:e].count(bytes([d])) <= b + a
    # the trailing empty line of a corpus that ends in d is a line; a delimiter AT o closes o's own line
    assert ref.extent(b"xd", 1, d) == (0, 1, 0) and ref.extent(b"ddd", 1, d) == (1, 1, 0)
    assert ref.extent(b"abdcd", 2, d) == (0, 2, 0) and ref.extent(b"abdcd", 3, d) == (3, 4, 0)
    assert ref.extent(b"abdcd", 3, d, 1, 0) == (0, 4, 0) and ref.extent(b"abdcd", 0, d, 0, 1) == (0, 4, 0) and ref.extent(b"abdcd", 0, d, 0, 2) == (0, 5, 0)


@pytest.mark.parametrize("R", [1, 2, 5, 64])
def test_cut_flags_at_distance_reach_minus_one_reach_and_reach_plus_one(R):
    d, o = 0x0A, 200
    for dist, cut in ((R - 1, False), (R, False), (R + 1, True)):
        if dist < 1:
            continue
        c = bytearray(b"." * 400)
        c[o - dist] = d                                     # the opening delimiter `dist` positions in front of o
        s, e, f = ref.extent(bytes(c), o, d, 0, 0, R)
        assert (s, bool(f & ref.START_CUT)) == ((o - R, True) if cut else (o - dist + 1, False))
        assert e == o + R and f & ref.END_CUT
        c = bytearray(b"." * 400)
        c[o + dist - 1] = d                                 # the closing delimiter is the dist-th byte looked at
        s, e, f = ref.extent(bytes(c), o, d, 0, 0, R)
        assert (e, bool(f & ref.END_CUT)) == ((o + R, True) if cut else (o + dist - 1, False))
        assert s == o - R and f & ref.START_CUT
    # the corpus's edges are no cut
    assert ref.extent(b"." * 10, 3, d, 0, 0, 3) == (0, 6, ref.END_CUT) and ref.extent(b"." * 10, 3, d, 0, 0, 2) == (1, 5, 3)
    assert ref.extent(b"." * 10, 7, d, 0, 0, 3) == (4, 10, ref.START_CUT) and ref.extent(b"." * 10, 9, d, 2, 2, 100) == (0, 10, 0)
    assert ref.extent(b"." * 10, 10, d) == (0, 0, ref.BAD) and ref.extent(b"", 0, d) == (0, 0, ref.BAD)


def test_lines_invariants_on_the_reference():
    rng = np.random.default_rng(2)
    for it in range(60):
        corpus = bytes(rng.choice(np.frombuffer(b"ab\n\n ", np.uint8), int(rng.integers(1, 300))))
        pats = [b"a", b"ab", b"a", b"\na", b"zz", b"b "]
        found = find_ref.find(corpus, pats)
        b, a = (int(v) for v in rng.integers(0, 3, 2))
        for reach in (1 << 16, 3):
            ln = ref.lines(corpus, found, 0x0A, b, a, reach)
            assert len(ln["ptr"]) == len(pats) + 1 and ln["ptr"][-1] == len(ln["start"]) == len(ln["end"]) == len(ln["flags"]) == len(ln["hits"])
            for j in range(len(pats)):
                lo, hi = ln["ptr"][j], ln["ptr"][j + 1]
                assert sum(ln["hits"][lo:hi]) == found[0][j] and ln["counts"][j] == hi - lo
                pairs = list(zip(ln["start"][lo:hi], ln["end"][lo:hi]))
                assert pairs == sorted(set(pairs))                                   # ascending, no pair twice
            assert ln["counts"][0] == ln["counts"][2] and ln["counts"][4] == 0
            if reach > 300 and b == a == 0:                                          # grep -c: the lines that hold the pattern
                assert ln["counts"][0] == sum(1 for s in corpus.split(b"\n") if b"a" in s)
                assert not any(ln["flags"])
            data, off = ref.text(corpus, ln["start"], ln["end"])
            assert off[-1] == len(data) and all(data[off[i]: off[i + 1]] == corpus[s:e] for i, (s, e) in enumerate(zip(ln["start"], ln["end"])))


def test_tables_helper_dedupes_in_order_of_first_appearance():
    raw, raw_off, slot = ref.tables(b"abcabcxab", [0, 3, 6, 6, 7, 9, 9])
    assert (raw, raw_off, slot) == (b"abcxab", [0, 3, 3, 4, 6], [0, 0, 1, 2, 3, 1])


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """HMSE_EINVAL before anything is cleared or launched: no device is touched, the pointers are never followed."""
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    MAXR = 1 << 24

    def extent(raw=p, raw_bytes=8, raw_off=p, n_rec=1, cuts=p, slot=p, n_chunks=1, pos=p, n=1, delim=10, before=0, after=0, reach=16,
               start=p, end=p, flags=p, status=p):
        return lib.hmse_lines_extent(raw, raw_bytes, raw_off, n_rec, cuts, slot, n_chunks, pos, n, delim, before, after, reach, start, end,
                                     flags, status, None)

    for kw in (dict(status=None), dict(delim=256), dict(reach=0), dict(reach=MAXR + 1), dict(n=1 << 33), dict(pos=None), dict(start=None),
               dict(end=None), dict(flags=None), dict(raw=None), dict(raw_off=None), dict(cuts=None), dict(slot=None),
               dict(n=0, status=None), dict(n=0, reach=0), dict(n=0, delim=1000)):
        assert extent(**kw) == EINVAL, kw

    def gather(raw=p, raw_bytes=8, raw_off=p, n_rec=1, cuts=p, slot=p, n_chunks=1, start=p, end=p, out_off=p, n=1, out=p, out_cap=8, status=p):
        return lib.hmse_lines_gather(raw, raw_bytes, raw_off, n_rec, cuts, slot, n_chunks, start, end, out_off, n, out, out_cap, status, None)

    for kw in (dict(status=None), dict(n=1 << 33), dict(out=None), dict(start=None), dict(end=None), dict(out_off=None), dict(raw=None),
               dict(raw_off=None), dict(cuts=None), dict(slot=None), dict(n=0, status=None), dict(n=0, out=None)):
        assert gather(**kw) == EINVAL, kw
    hdr = open(os.path.join(ROOT, "include", "hmse.h")).read()
    assert "#define HMSE_LINES_MAX_REACH (1u << 24)" in hdr and "#define HMSE_LINES_BAD       128u" in hdr
    assert lib.hmse_abi_version() == 3


def test_wrappers_refuse_host_tensors():
    import torch
    from hmse_amd import ops
    raw, i64 = torch.zeros(4, dtype=torch.uint8), lambda *v: torch.tensor(v, dtype=torch.int64)
    with pytest.raises(ops.HmseError, match="HBM"):
        ops.lines_extent(raw, i64(0, 4), i64(0, 4), i64(0), i64(1), 0x0A, 0, 0, 16)
    with pytest.raises(ops.HmseError, match="HBM"):
        ops.lines_gather(raw, i64(0, 4), i64(0, 4), i64(0), i64(0), i64(4), i64(0, 4), 4)
    assert (ops.LINES_START_CUT, ops.LINES_END_CUT, ops.LINES_BAD, ops.LINES_MAX_REACH) == (1, 2, 128, 1 << 24)


def test_lines_text_and_grep_refuse_bad_arguments_before_any_device_work():
    from hmse_amd import find
    fd = find.StoreFinder.__new__(find.StoreFinder)              # no store, no device: the refusals below need neither
    found = find.Found(None, None, None)
    for kw, msg in ((dict(delim=b""), "one byte"), (dict(delim=b"\r\n"), "one byte"), (dict(delim="\n"), "one byte"), (dict(delim=10), "one byte"),
                    (dict(before=-1), "negative"), (dict(after=-2), "negative"), (dict(reach=0), "reach"),
                    (dict(reach=find.HMSE_LINES_MAX_REACH + 1), "HMSE_LINES_MAX_REACH")):
        with pytest.raises(ValueError, match=msg):
            fd.lines(found, **kw)
        with pytest.raises(ValueError, match=msg):
            fd.grep([b"x"], **kw)
        with pytest.raises(ValueError, match=msg):
            find.grep(None, [b"x"], "cpu", **kw)
    with pytest.raises(ValueError, match="Found or an int64 tensor"):
        fd.lines([1, 2, 3])
    for bad in (None, [1, 2], (1, 2), "ab"):
        with pytest.raises(ValueError, match="Lines or a"):
            fd.text(bad)
    assert [f for f in find.Lines.__dataclass_fields__] == ["ptr", "start", "end", "flags", "hits", "counts"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ -std=c++20")
def test_kernel_source_on_cpu_threads_equals_the_definition():
    """tools/lines_emu.py: the kernels' source compiled for the host as a stand-alone program (a std::barrier per wavefront under
    __ballot: a loop that is not wave-uniform hangs it), against the brute-force definition on random chunk maps.  Unsanitized, short."""
    probe = subprocess.run(["g++", "-std=c++20", "-x", "c++", "-fsyntax-only", "-"], input="#include <barrier>\nint main(){}\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ has no -std=c++20 <barrier>")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lines_emu.py"), "--iters", "30", "--seed", "3"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
