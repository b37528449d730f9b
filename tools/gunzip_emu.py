"""The import kernels (hmse_amd/csrc/gunzip.hip) on the CPU against the byte filter and against zlib: no GPU needed.
    python tools/gunzip_emu.py [--iters 6] [--seed 12345] [--sanitize]
Cuts the kernels out of gunzip.hip (everything between its geometry constants and its entry points; the bit reader, the code tables, the
symbol decode and the walk over a stream — ifl::walk_stream, which the measure kernel runs with its counting sink — come with
hmse_amd/csrc/inflate_core.h as they are, the block-sum scan with blockops.h), compiles them with
tools/gunzip_emu.cpp (g++ -std=c++20: one std::thread per lane, std::barrier under __syncthreads, __ballot, readlane and readfirstlane)
and runs the candidate passes on planted buffers and the measure kernel on known answers that this script takes from zlib
(tests/gunzip_ref.py): small members of every block type and header, BGZF blocks, damaged ones, candidates inside other members, and
the catalogue of tests/deflate_vectors.py.
--sanitize builds that program with -fsanitize=address,undefined (host code only).  Exit status 0 = all equal."""
import os
import random
import struct
import sys
import zlib

from emu_common import ROOT, run

sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_vectors  # noqa: E402
import gunzip_ref as ref  # noqa: E402


def _text(rnd, n):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"\x1f\x8b\x08\x00", b" ", b"\n", b"the", b"of"]
    out = b""
    while len(out) < n:
        out += rnd.choice(words)
    return out[:n]


def cases():
    """[(blob, [candidate offsets])]: small on purpose — a symbol costs the emulator several barriers of 64 threads"""
    rnd = random.Random(77)
    out = []
    # every block type and header field
    parts = [ref.member(b""), ref.member(b"a", 0), ref.member(_text(rnd, 70), 1, zlib.Z_FIXED), ref.member(_text(rnd, 300), 6),
             ref.member(bytes(rnd.randrange(256) for _ in range(200)), 9, zlib.Z_HUFFMAN_ONLY), ref.member(b"z" * 600, 6, zlib.Z_RLE),
             ref.member(_text(rnd, 90), 6, extra=b"", name=b"n", comment=b"c" * 70, hcrc=True),
             ref.member(_text(rnd, 90), 6, extra=b"AB\x03\x00xyz", hcrc=True), ref.member(b"q" * 40, 6, name=b"x" * 130),
             ref.bgzf_member(_text(rnd, 400)), ref.bgzf_member(b""), ref.member(_text(rnd, 50), 6, extra=b"XY\x01\x00.BC\x02\x00\x05\x00")]
    blob = b"".join(parts)
    out.append((blob, ref.candidates(blob)))
    # a stored member that holds a whole member and junk: the inner one is a candidate like any other
    inner = ref.member(_text(rnd, 60), 6)
    nested = ref.member(inner + bytes(rnd.randrange(256) for _ in range(40)) + inner[:25], 0) + inner
    out.append((nested, ref.candidates(nested)))
    # damage: a bad FHCRC, a reserved bit (handed over by a caller that filtered nothing), a wrong ISIZE, a lying BSIZE within the data,
    # BSIZE + 1 below header + 10 (the ordinary path), ISIZE above 65536 in a BGZF block (the ordinary path), truncation, junk in front
    m = bytearray(ref.member(_text(rnd, 80), 6, name=b"file", hcrc=True)); m[12] ^= 1
    r = bytearray(ref.member(b"abc", 6)); r[3] |= 0x40
    i = bytearray(ref.member(_text(rnd, 80), 6)); i[-4] ^= 1
    z = ref.bgzf_member(_text(rnd, 100))
    lie = ref.bgzf_member(_text(rnd, 100), bsize=len(z) - 6)
    low = ref.bgzf_member(_text(rnd, 30), bsize=20)
    tr = ref.member(_text(rnd, 500), 6)
    blob = bytes(m) + bytes(r) + bytes(i) + lie + low + b"\x00junk" + tr[:-9]
    offs = [0, len(m), len(m) + len(r), len(m) + len(r) + len(i), len(m) + len(r) + len(i) + len(lie), len(blob) - len(tr) + 9, len(blob) - 5, len(blob) + 7]
    out.append((blob, sorted(set(offs + ref.candidates(blob)))))
    # mutations of one small file: one byte or one bit each
    base = ref.member(_text(rnd, 150), 6) + ref.member(_text(rnd, 120), 9, zlib.Z_FIXED) + ref.member(b"k" * 100, 1)
    for _ in range(10):
        b = bytearray(base)
        at = rnd.randrange(len(b))
        b[at] = rnd.randrange(256) if rnd.random() < 0.5 else b[at] ^ (1 << rnd.randrange(8))
        out.append((bytes(b), sorted(set([0] + ref.candidates(bytes(b))))))
    # hand-built streams zlib's encoder never writes (tests/deflate_vectors.py), each wrapped as a member: the dynamic-header rules,
    # one-code and empty distance sets, 15-bit codes, the longest header, and what zlib refuses beside them
    out.append(deflate_vectors.emu_case())
    return out


def known_answers(td):
    path = os.path.join(td, "gunzip_known.bin")
    with open(path, "wb") as f:
        for blob, offs in cases():
            f.write(struct.pack("<I", len(blob)) + blob + struct.pack("<I", len(offs)))
            for p in offs:
                m = ref.measure(blob, p)
                f.write(struct.pack("<QQQQII", p, m["stream_off"], m["end"], m["raw_len"], m["crc"], m["flags"]))
    return [path]


if __name__ == "__main__":
    sys.exit(run(__doc__, "gunzip", "constexpr int GZ_NT", "// ---- entry points", 6, extra=known_answers))
