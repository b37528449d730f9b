"""The arithmetic the export kernels (hmse_amd/csrc/export.hip) rest on, in plain Python; the oracle for the results is zlib.

A CRC-32 register is a polynomial over GF(2) modulo P = x^32 + x^26 + ... + 1, REFLECTED: bit 31 is the coefficient of x^0, bit 0 that of
x^31 (P without its x^32 term is 0xEDB88320).  With crc() zlib's CRC-32 (init and final xor 0xFFFFFFFF) and reg() the register after
the same bytes from a register of 0 without the final xor:
    crc(A + B) == mulmod(crc(A), xpow8(len(B))) ^ crc(B)                  (the init terms cancel)
    crc(M)     == reg(M) ^ mulmod(0xFFFFFFFF, xpow8(len(M))) ^ 0xFFFFFFFF
    reg(A + B) == mulmod(reg(A), xpow8(len(B))) ^ reg(B),   reg(zeros + M) == reg(M)
"""
import zlib

POLY = 0xEDB88320
ONE = 0x80000000        # x^0
GZIP_HEADER = bytes.fromhex("1f8b08000000000000ff")                    # 1f 8b 08 00 | MTIME 0 | XFL 0 | OS ff
BGZF_HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")        # FLG.FEXTRA, XLEN 6, 'B' 'C', SLEN 2; BSIZE (u16) follows
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def mulmod(a: int, b: int) -> int:
    """a * b modulo P"""
    p = 0
    for i in range(32):
        if a & (ONE >> i):          # the term x^i of a
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)      # b * x
    return p


def xpow8(n: int) -> int:
    """x^(8 n) modulo P, by squaring along the bits of n"""
    sq, p = ONE >> 8, ONE
    while n:
        if n & 1:
            p = mulmod(p, sq)
        sq = mulmod(sq, sq)
        n >>= 1
    return p


def reg(data: bytes, c: int = 0) -> int:
    """the register after `data`, bit by bit, from the register c; no final xor"""
    for byte in data:
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
    return c


def crc_from_reg(r: int, n: int) -> int:
    return r ^ mulmod(0xFFFFFFFF, xpow8(n)) ^ 0xFFFFFFFF


def combine(crcs, lens) -> int:
    """CRC-32 of the concatenation from the parts' CRCs and lengths: XOR_k crc[k] * x^(8 * bytes behind k)"""
    out, behind = 0, 0
    for c, n in zip(reversed(list(crcs)), reversed(list(lens))):
        out ^= mulmod(c & 0xFFFFFFFF, xpow8(behind))
        behind += n
    return out


def geometry(n: int, smax: int = 128):
    """the CRC kernel's layout of a range of n > 0 bytes: -> (tiles, S = strip bytes per lane and tile, SS = strip bytes per lane)"""
    tile = 64 * smax
    tiles = -(-n // tile)
    s = (-(-n // (64 * tiles)) + 15) & ~15
    return tiles, s, tiles * s


def strip_tree(data: bytes, strip: int | None = None) -> int:
    """CRC-32 the way the kernel computes it: the range right-aligned into 64 strips of `strip` bytes (default: the kernel's), zeros in
    front, one register per strip from 0, six levels of c = c_left * x^(8 * strip * 2^level) ^ c_right, the init folded in at the end."""
    n = len(data)
    if n == 0:
        return 0
    ss = geometry(n)[2] if strip is None else strip
    assert 64 * ss >= n
    padded = bytes(64 * ss - n) + data
    c = [reg(padded[l * ss: (l + 1) * ss]) for l in range(64)]
    m = xpow8(ss)
    while len(c) > 1:
        c = [mulmod(c[i], m) ^ c[i + 1] for i in range(0, len(c), 2)]
        m = mulmod(m, m)
    return crc_from_reg(c[0], n)


def member(stream: bytes, raw: bytes, bgzf: bool = False) -> bytes:
    """one gzip / BGZF member around a raw DEFLATE stream of `raw`"""
    trailer = zlib.crc32(raw).to_bytes(4, "little") + (len(raw) & 0xFFFFFFFF).to_bytes(4, "little")
    if not bgzf:
        return GZIP_HEADER + stream + trailer
    size = 18 + len(stream) + 8
    return BGZF_HEADER + (size - 1).to_bytes(2, "little") + stream + trailer


def parse_members(blob: bytes):
    """split a multi-member file made of members with the headers above -> [(offset, size)], using zlib to find every member's end"""
    out, pos = [], 0
    while pos < len(blob):
        d = zlib.decompressobj(wbits=31)
        d.decompress(blob[pos:])
        assert d.eof
        size = len(blob) - pos - len(d.unused_data)
        out.append((pos, size))
        pos += size
    return out
