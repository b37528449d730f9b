"""What hmse_amd.gunzip must compute, from stock zlib and plain Python (tests/test_gunzip_host.py, tests/test_gpu_gunzip.py, tools/gunzip_emu.py).

  chain(blob)        the definition: a chain of zlib.decompressobj(wbits=31) over what the one before left unused -> [(offset, size, raw)];
                     Refused (member index, offset) where zlib refuses or the data ends inside a member
  candidates(blob)   the byte filter of hmse_gzip_candidates
  parse_header(...)  RFC 1952, the way hmse_gzip_measure reads a header
  measure(blob, p)   what hmse_gzip_measure reports for a candidate at p (the stream walked by zlib's raw inflate)
  member(...)        a gzip member around zlib's raw DEFLATE of `raw` with any header fields; bgzf_member(raw)
"""
import zlib

VALID, FAST, WHY_SHIFT = 1, 2, 2
WHY_HEADER, WHY_STREAM, WHY_LENGTH, WHY_BOUNDS = 1, 2, 3, 4
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16
MIN_MEMBER = 20


class Refused(ValueError):
    def __init__(self, member, offset, why):
        super().__init__(f"member {member} at offset {offset}: {why}")
        self.member, self.offset = member, offset


def _inflate(blob, pos, wbits):
    """one stream from blob[pos:] fed in growing pieces (what is left unused stays small) -> (raw, end) or (None, reason)"""
    d = zlib.decompressobj(wbits=wbits)
    out, q, step = [], pos, 256
    try:
        while not d.eof and q < len(blob):
            piece = blob[q: q + step]
            out.append(d.decompress(piece))
            q += len(piece)
            step = min(step * 2, 1 << 20)
    except zlib.error as e:
        return None, str(e)
    if not d.eof:
        return None, "the data ends inside the member"
    return b"".join(out), q - len(d.unused_data)


def chain(blob: bytes):
    out, pos = [], 0
    while pos < len(blob):
        raw, end = _inflate(blob, pos, 31)
        if raw is None:
            raise Refused(len(out), pos, end)
        out.append((pos, end - pos, raw))
        pos = end
    return out


def candidates(blob: bytes):
    out, p, last = [], blob.find(b"\x1f\x8b\x08"), len(blob) - MIN_MEMBER
    while 0 <= p <= last:
        if not blob[p + 3] & 0xE0:
            out.append(p)
        p = blob.find(b"\x1f\x8b\x08", p + 1)
    return out


def parse_header(blob: bytes, p: int):
    """-> (why, stream_off, BSIZE + 1 of the first BC subfield or 0); why = 0 for a header hmse_gzip_measure accepts"""
    n = len(blob)
    if p > n or n - p < MIN_MEMBER:
        return WHY_BOUNDS, p, 0
    if blob[p: p + 3] != b"\x1f\x8b\x08" or blob[p + 3] & 0xE0:
        return WHY_HEADER, p, 0
    flg, q, bsize1 = blob[p + 3], p + 10, 0
    if flg & FEXTRA:
        xlen = int.from_bytes(blob[q: q + 2], "little")
        s, x1 = q + 2, q + 2 + xlen
        if x1 > n:
            return WHY_BOUNDS, p, 0
        while s + 4 <= x1:
            slen = int.from_bytes(blob[s + 2: s + 4], "little")
            if blob[s: s + 2] == b"BC" and slen == 2 and s + 6 <= x1 and not bsize1:
                bsize1 = int.from_bytes(blob[s + 4: s + 6], "little") + 1
            s += 4 + slen
        q = x1
    for bit in (FNAME, FCOMMENT):
        if flg & bit:
            z = blob.find(b"\0", q)
            if z < 0:
                return WHY_BOUNDS, p, 0
            q = z + 1
    if flg & FHCRC:
        if n - q < 2:
            return WHY_BOUNDS, p, 0
        if zlib.crc32(blob[p: q]) & 0xFFFF != int.from_bytes(blob[q: q + 2], "little"):
            return WHY_HEADER, q, 0
        q += 2
    return 0, q, bsize1


def measure(blob: bytes, p: int) -> dict:
    n = len(blob)
    why, q, bsize1 = parse_header(blob, p)
    bad = lambda w, so=p: dict(valid=False, fast=False, why=w, stream_off=so, end=p, raw_len=0, crc=0, flags=w << WHY_SHIFT)
    if why:
        return bad(why)
    if bsize1 and bsize1 >= (q - p) + 10 and n - p >= bsize1:
        isize = int.from_bytes(blob[p + bsize1 - 4: p + bsize1], "little")
        if isize <= 65536:
            return dict(valid=True, fast=True, why=0, stream_off=q, end=p + bsize1, raw_len=isize, flags=VALID | FAST,
                        crc=int.from_bytes(blob[p + bsize1 - 8: p + bsize1 - 4], "little"))
    raw, end = _inflate(blob, q, -15)
    if raw is None:
        return bad(WHY_BOUNDS if end.startswith("the data ends") else WHY_STREAM, q)
    if n - end < 8:
        return bad(WHY_BOUNDS, q)
    if len(raw) != int.from_bytes(blob[end + 4: end + 8], "little"):
        return bad(WHY_LENGTH, q)
    return dict(valid=True, fast=False, why=0, stream_off=q, end=end + 8, raw_len=len(raw), flags=VALID,
                crc=int.from_bytes(blob[end: end + 4], "little"))


def deflate(raw: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(raw) + co.flush()


def member(raw: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, extra: bytes | None = None, name: bytes | None = None,
           comment: bytes | None = None, hcrc: bool = False, mtime: int = 0, stream: bytes | None = None) -> bytes:
    """one gzip member; extra = the bytes of the FEXTRA field (b"" gives XLEN 0), name / comment without their zero"""
    flg = (FEXTRA if extra is not None else 0) | (FNAME if name is not None else 0) | (FCOMMENT if comment is not None else 0) | (FHCRC if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + mtime.to_bytes(4, "little") + b"\x00\x03"
    if extra is not None:
        h += len(extra).to_bytes(2, "little") + extra
    for s in (name, comment):
        if s is not None:
            h += s + b"\0"
    if hcrc:
        h += (zlib.crc32(h) & 0xFFFF).to_bytes(2, "little")
    body = deflate(raw, level, strategy) if stream is None else stream
    return h + body + zlib.crc32(raw).to_bytes(4, "little") + (len(raw) & 0xFFFFFFFF).to_bytes(4, "little")


def bgzf_member(raw: bytes, level: int = 6, bsize: int | None = None) -> bytes:
    body = deflate(raw, level)
    size = 18 + len(body) + 8
    return member(raw, extra=b"BC\x02\x00" + ((size - 1) if bsize is None else bsize).to_bytes(2, "little"), stream=body)


def text(seed: int, n: int) -> bytes:
    """n bytes with repeats at many distances (matches) and a literal-heavy third; no gzip magic"""
    import numpy as np
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 12, 200)]
    out = bytearray()
    while len(out) < n:
        r = int(rng.integers(0, 10))
        if r < 6:
            out += words[int(rng.integers(0, 200))] + b" "
        elif r < 8 and len(out) > 300:
            a = int(rng.integers(0, len(out) - 200))
            out += out[a: a + int(rng.integers(3, 200))]
        else:
            out += bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8)).replace(b"\x1f\x8b", b"..")
    return bytes(out[:n]).replace(b"\x1f\x8b", b"..")


def nested_case():
    """-> (blob, [raw of every member zlib finds]): a level-0 member whose payload holds two complete members and 1000 random bytes; behind it
    an empty member, the inner member again and a 200 000-byte member.  The inner members are candidates, never members."""
    import numpy as np
    inner_raw, big = text(5, 700), text(6, 200_000)
    inner = member(inner_raw, 6)
    payload = inner + bytes(np.random.default_rng(7).integers(0, 256, 1000, dtype=np.uint8)).replace(b"\x1f\x8b", b"..") + inner
    blob = member(payload, 0) + member(b"") + inner + member(big, 6)
    return blob, [payload, b"", inner_raw, big]


MUTATION_SEED, N_MUTATIONS = 3, 200


def mutation_file() -> bytes:
    """six small generic members (no BC subfield) with names, comments, an FHCRC and an extra field: many bytes zlib ignores"""
    return b"".join([member(text(11, 60), 6, name=b"first-rotation.log", mtime=1700000000), member(text(12, 45), 0, comment=b"stored " * 4),
                     member(b"", 9, name=b"empty"), member(text(13, 80), 9, zlib.Z_FIXED, extra=b"ab\x04\x00wxyz", hcrc=True),
                     member(b"r" * 70, 1, zlib.Z_RLE, name=b"runs", comment=b"of one byte"), member(text(14, 50), 6, zlib.Z_HUFFMAN_ONLY, mtime=12345)])


def mutations(seed: int = MUTATION_SEED, count: int = N_MUTATIONS):
    """`count` copies of mutation_file() with one byte replaced or one bit flipped -> [(blob, position)]"""
    import random
    rnd, base, out = random.Random(seed), mutation_file(), []
    for _ in range(count):
        b = bytearray(base)
        at = rnd.randrange(len(b))
        if rnd.random() < 0.5:
            b[at] = (b[at] + 1 + rnd.randrange(255)) & 0xFF
        else:
            b[at] ^= 1 << rnd.randrange(8)
        out.append((bytes(b), at))
    return out


def outcome(blob: bytes):
    """the zlib chain's verdict: [raw of every member], or None if it refuses"""
    try:
        return [raw for _, _, raw in chain(blob)]
    except Refused:
        return None
