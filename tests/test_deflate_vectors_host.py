"""CPU: the hand-built DEFLATE streams of tests/deflate_vectors.py — forms zlib's decoder accepts and its encoder never writes, and the
rejections beside them.  Every entry's stated verdict is zlib's (an entry that does not mean what its name says fails here), the flip
family holds both outcomes in quantity, and the decoders that run without a GPU give zlib's decision and bytes on all of it: the CPU
oracle (oracle/hmse_oracle_inflate.c), gz::measure_kernel (tools/gunzip_emu.py) and the two l1_inflate kernels (tools/inflate_emu.py)
with one std::thread per lane."""
import os
import re
import subprocess
import sys

import numpy as np

import deflate_vectors as dv
import gunzip_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_catalogue_verdicts_are_zlibs():
    cat, raws = dv.catalogue(), dv.catalogue_raws()
    wrong = [(name, expect) for (name, _, _, expect), raw in zip(cat, raws) if expect != ("accept" if raw is not None else "reject")]
    assert not wrong, wrong
    assert sum(e[3] == "accept" for e in cat) >= 60 and sum(e[3] == "reject" for e in cat) >= 25
    by = {name: (raw, s) for (name, s, _, _), raw in zip(cat, raws)}
    # the entries say what their names say
    assert len(by["lengths-3-10-11-257-258-and-284+31"][0]) == 4 + 3 + 10 + 11 + 257 + 258 + 258 + 257
    assert len(by["stored-65535"][0]) == 65535 and len(by["300-one-literal-blocks"][0]) == 300
    assert len(by["distances-1-4-5-24577-32768"][0]) == 32768 + 3 + 3 + 4 + 3 + 3 + 5 + 258 + 3
    assert by["eob-only-final"][0] == b"" and by["eob-only-nonfinal-then-data"][0] == b"data" and by["hdist1-length0-literal-only"][0] == b"aaa"
    assert by["empty-blocks-between-data"][0] == b"syncaaaaflush" and by["one-distance-code-used"][0] == b"aaaaaaaa"
    for (name, s, zd, expect), raw in zip(cat, raws):
        if zd is not None and expect == "accept":                                      # the bytes come out of THIS dictionary
            k = re.search(r"258-from-last-(\d+)-bytes@pos(\d+)", name)
            if k:
                src = zd[-int(k[1]):] + b"y" * int(k[2])
                assert raw == b"y" * int(k[2]) + (src * 258)[:258] + b"z", name
            else:
                pos = int(name[-1])
                assert raw == b"x" * pos + ((zd + b"x" * pos) * 3)[:3], name
    # the longest header: 316 single codes of 6 and 7 bits, at each bit offset; the stated length is what a parse of the stream finds
    for k in range(8):
        s, hbits, at = dv.long_header(k, seven=True)
        assert hbits == dv.header_bits(s, at) == 17 + 19 * 3 + 316 * 7 and by[f"longest-header-all-7-bit@{k} ({hbits} header bits)"][1] == s
    longs = [(name, s) for name, s, _, _ in cat if name.startswith("longest-header@")]
    assert len(longs) == 8
    for k, (name, s) in enumerate(longs):
        stream, hbits, at = dv.long_header(k)
        assert stream == s and at % 8 == k and f"({hbits} header bits)" in name
        assert hbits == dv.header_bits(s, at) >= dv.LONG_HEADER_MIN_BITS and hbits >= 2256
    for k in range(8):
        s = by[f"second-dynamic-header@{k}"][1]
        at = 10 + 9 * ((k - 2) % 8)                                                    # behind the fixed block of 9-bit literals
        assert at % 8 == k and (int.from_bytes(s, "little") >> at) & 7 == 5 and dv.header_bits(s, at) > 60       # BFINAL 1, BTYPE 2
    assert by["15-bit-codes-hclen19"][1][305 + 1] >> 5 | (by["15-bit-codes-hclen19"][1][305 + 2] & 1) << 3 == 15      # HCLEN - 4


def test_flip_family_floors():
    fam, raws = dv.flip_family(), dv.family_raws()
    accepted = sum(r is not None for r in raws)
    print(f"flip family: {len(fam)} mutants, zlib accepts {accepted} ({accepted / len(fam):.1%}), refuses {len(fam) - accepted}")
    assert len(fam) == len(raws) > 5000
    assert accepted >= 0.10 * len(fam) and len(fam) - accepted >= 0.30 * len(fam)
    names = {n.split(":")[0] for n, _ in fam}
    assert {"zlib-level9", "zlib-huffman-only", "longest-header", "crossing-run", "15-bit", "two-blocks"} <= names
    s, at = dv.two_blocks()
    assert at % 8 and f"two-blocks:flip{at}" in {n for n, _ in fam} and f"two-blocks:flip{at + dv.header_bits(s, at) + 63}" in {n for n, _ in fam}
    for name, s, spans in dv.seeds():                                                  # every seed is a stream zlib accepts
        assert dv.verdict(s) is not None, name


def _both(orc, vectors, raws, claimed):
    for v, raw in zip(vectors, raws):
        got, rc = orc.inflate(v[1], len(raw or b""), v[2] if len(v) > 2 else None)
        assert (got is None) == (raw is None) and got == raw, (v[0], rc)
    recs, first = dv.records(vectors, raws, claimed)
    streams, off, kind, base, raw_len = dv.pack(recs)
    out, out_off, ok = orc.inflate_chunks(streams, off, kind, base, raw_len)
    want = np.array([True] * first + [r is not None for r in raws] + [False] * (len(recs) - first - len(raws)))      # refused at every claimed length
    assert np.array_equal(ok, want), [(vectors[(i - first) % len(vectors)][0] if i < first + len(raws) else int(i)) for i in np.nonzero(ok != want)[0][:10]]
    for i, raw in enumerate(raws):
        if raw is not None:
            assert out[int(out_off[first + i]): int(out_off[first + i + 1])].tobytes() == raw, vectors[i][0]


def test_the_oracle_on_the_catalogue(orc):
    _both(orc, dv.catalogue(), dv.catalogue_raws(), dv.CLAIMED)


def test_the_oracle_on_the_flip_family(orc):
    _both(orc, dv.flip_family(), dv.family_raws(), (1, 2, 3, 4, 8))


def test_wrapped_entries_measure_as_zlib_decides():
    cat, raws = dv.catalogue(), dv.catalogue_raws()
    for (name, s, zd, expect), raw, mem in zip(cat, raws, dv.wrapped((e[1], r) for e, r in zip(cat, raws))):
        m = ref.measure(mem, 0)
        if zd is None:
            assert m["valid"] == (expect == "accept"), name
            if m["valid"]:
                assert (m["end"], m["raw_len"]) == (len(mem), len(raw)) and ref.chain(mem)[0][2] == raw, name
    assert len(dv.emu_case()[1]) == len(cat) - len(dv.SLOW)


def test_the_measure_emulator_counts_the_catalogue():
    """(the run itself is tests/test_gunzip_host.py::test_the_emulator_builds_and_its_cases_pass)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gunzip_emu
    cases = gunzip_emu.cases()
    assert cases[-1] == dv.emu_case() and len(cases) == 14


def test_the_inflate_emulator_builds_and_agrees_with_zlib():
    """tools/inflate_emu.py: both kernels cut out of l1_inflate.hip, one std::thread per lane, on the catalogue (no sanitizer here)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "inflate_emu.py")], capture_output=True, text=True)
    n = len(dv.catalogue()) - len(dv.SLOW) + len(dv.DICTS) + sum(map(len, dv.WOULD_DECODE.values()))
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    for kernel in ("l1_inflate_kernel", "l1_inflate_lanes_kernel"):
        assert re.search(r"%s: %d records, 0 wrong" % (kernel, n), r.stdout), r.stdout[-3000:]
