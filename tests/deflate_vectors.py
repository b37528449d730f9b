"""Hand-built DEFLATE streams that zlib's encoder never writes (tests/test_deflate_vectors_host.py, tests/test_gpu_deflate_vectors.py,
tools/gunzip_emu.py, tools/inflate_emu.py).  The definition of every decoder here is stock zlib: accepted if and only if
zlib.decompressobj(-15[, zdict]) reaches eof with no unused_data, same bytes.

  BitWriter            LSB-first bits (RFC 1951 §3.1.1); Huffman codes go in MSB first
  canon(lens)          canonical codes from code lengths -> {symbol: (code, length)}
  stored / fixed / dynamic
                       one block each; the caller chooses the code-length operations [(symbol 0..18, extra)] and the token list:
                         int                  a literal/length symbol through the block's code (0..255 literal, 256 end of block, 257.. alone)
                         ("M", len, dist)     a match, the usual way (258 as symbol 285)
                         ("LS", sym, extra)   a length symbol with chosen extra bits;  ("DS", sym, extra) a distance symbol likewise
                         ("R", value, k)      k raw bits;  ("C", code, k) a raw k-bit code, MSB first (codes that a set leaves undefined)
  rle(lens) / plain(lens)
                       code-length operations for lens: greedy runs over the WHOLE array, so a run crosses from the literal/length into
                       the distance lengths wherever they are equal (libdeflate and zopfli do; zlib's two send_tree calls never do) / one
                       single code per length
  header_bits(s, at)   bit length of the dynamic header that starts at bit `at` (parsed from the stream itself)
  verdict(s, zdict)    zlib's answer: the raw bytes, or None
  catalogue()          [(name, stream, zdict | None, "accept" | "reject")]
  flip_family()        [(name, stream)]: every single-bit flip over a seed's header and 64 bits behind it, every truncation to a byte
                       boundary inside those bits; the verdict of a mutant comes from zlib at run time
  records(v, raws, claimed) / pack(recs)
                       the vectors as records of one hmse_l1_inflate call (a dictionary is the stored base record of a DELTA record); with
                       `claimed` every refused stream once more per claimed raw length (CLAIMED, or WOULD_DECODE by entry)
  wrapped(...) / emu_case()
                       the streams as gzip members (tests/gunzip_ref.py::member); the catalogue as one case of tools/gunzip_emu.py
  SLOW                 the entries the thread-per-lane emulators leave out
"""
import functools
import random
import zlib

import gunzip_ref as ref

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
EOB = 256
LONG_HEADER_MIN_BITS = 2240
SLOW = ("stored-65535", "300-one-literal-blocks")


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value, k):
        self.acc |= (value & ((1 << k) - 1)) << self.n
        self.n += k

    def code(self, code, k):
        self.bits(int(format(code & ((1 << k) - 1), f"0{k}b")[::-1], 2) if k else 0, k)

    def align(self):
        self.n = (self.n + 7) & ~7

    def raw(self, data):
        assert self.n % 8 == 0
        self.acc |= int.from_bytes(data, "little") << self.n
        self.n += 8 * len(data)

    def done(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canon(lens):
    """RFC 1951 §3.2.2, whatever the set (an over-subscribed one gives codes that do not fit: nothing is coded with those)"""
    out, code = {}, 0
    for k in range(1, 16):
        for s, l in enumerate(lens):
            if l == k:
                out[s] = (code, k)
                code += 1
        code <<= 1
    return out


def _tokens(w, tokens, lit, dist):
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "M":
            _, length, d = t
            ls = max(i for i, b in enumerate(LEN_BASE) if b <= length)
            ds = max(i for i, b in enumerate(DIST_BASE) if b <= d)
            assert length <= 258 and d <= 32768, "not a DEFLATE match"
            w.code(*lit[257 + ls]); w.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
            w.code(*dist[ds]); w.bits(d - DIST_BASE[ds], DIST_EXTRA[ds])
        elif t[0] == "LS":
            w.code(*lit[t[1]]); w.bits(t[2], LEN_EXTRA[t[1] - 257])
        elif t[0] == "DS":
            w.code(*dist[t[1]]); w.bits(t[2], DIST_EXTRA[t[1]] if t[1] < 30 else 0)
        elif t[0] == "R":
            w.bits(t[1], t[2])
        elif t[0] == "C":
            w.code(t[1], t[2])
        else:
            raise ValueError(t)


def stored(w, data, final=True, length=None, nlen=None):
    w.bits(1 if final else 0, 1); w.bits(0, 2); w.align()
    length = len(data) if length is None else length
    w.bits(length, 16); w.bits(~length & 0xFFFF if nlen is None else nlen, 16)
    w.raw(data)


def fixed(w, tokens, final=True):
    w.bits(1 if final else 0, 1); w.bits(1, 2)
    _tokens(w, tokens, canon(FIXED_LIT), canon(FIXED_DIST))


def expand(ops):
    lens = []
    for s, x in ops:
        if s < 16:
            lens.append(s)
        else:
            lens += [(lens[-1] if lens else 0) if s == 16 else 0] * ((3 if s < 18 else 11) + x)
    return lens


def plain(lens):
    return [(l, 0) for l in lens]


def rle(lens):
    ops, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        run, v = j - i, lens[i]
        if v == 0:
            while run >= 11:
                k = min(run, 138); ops.append((18, k - 11)); run -= k
            if run >= 3:
                ops.append((17, run - 3)); run = 0
        else:
            ops.append((v, 0)); run -= 1
            while run >= 3:
                k = min(run, 6); ops.append((16, k - 3)); run -= k
        ops += [(v, 0)] * run
        i = j
    return ops


def balanced(used):
    """a complete code over the symbols in use (two at least: an incomplete code-length code is refused), lengths differing by one at most"""
    used = sorted(used)
    if len(used) < 2:
        used = sorted(set(used) | {1 if used == [0] else 0})
    k = len(used); m = k.bit_length() - 1; short = (1 << (m + 1)) - k
    lens = [0] * 19
    for i, s in enumerate(used):
        lens[s] = m if i < short else m + 1
    return lens


def dynamic(w, nlit, ndist, ops, tokens, final=True, clens=None, ncl=None, hlit=None, hdist=None):
    """-> the header's bit length (the three block bits to the last code-length operation)"""
    start = w.n
    w.bits(1 if final else 0, 1); w.bits(2, 2)
    w.bits(nlit - 257 if hlit is None else hlit, 5); w.bits(ndist - 1 if hdist is None else hdist, 5)
    clens = balanced({s for s, _ in ops}) if clens is None else clens
    if ncl is None:
        ncl = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if clens[s]])
    w.bits(ncl - 4, 4)
    for s in CL_ORDER[:ncl]:
        w.bits(clens[s], 3)
    cl = canon(clens)
    for s, x in ops:
        w.code(*cl[s]); w.bits(x, CL_EXTRA.get(s, 0))
    hbits = w.n - start
    lens = expand(ops)
    lens += [0] * (nlit + ndist - len(lens))
    _tokens(w, tokens, canon(lens[:nlit]), canon(lens[nlit: nlit + ndist]))
    return hbits


def dyn(w, lit, dist, tokens, final=True, nlit=None, ndist=None, ops=None, coder=rle, **kw):
    """a dynamic block from {symbol: length} of the two alphabets"""
    nlit = nlit or max(257, max(lit) + 1)
    ndist = ndist or max(dist, default=0) + 1
    lens = [lit.get(s, 0) for s in range(nlit)] + [dist.get(s, 0) for s in range(ndist)]
    return dynamic(w, nlit, ndist, coder(lens) if ops is None else ops, tokens, final, **kw)


def header_bits(stream, at=0):
    v = int.from_bytes(stream, "little") >> at
    assert (v >> 1) & 3 == 2, "no dynamic block there"
    nlit, ndist, ncl = ((v >> 3) & 31) + 257, ((v >> 8) & 31) + 1, ((v >> 13) & 15) + 4
    n, clens = 17, [0] * 19
    for s in CL_ORDER[:ncl]:
        clens[s] = (v >> n) & 7; n += 3
    dec = {cl: s for s, cl in canon(clens).items()}
    have = 0
    while have < nlit + ndist:
        c = 0
        for l in range(1, 8):
            c = (c << 1) | ((v >> n) & 1); n += 1
            if (c, l) in dec:
                break
        s = dec[(c, l)]
        have += 1 if s < 16 else (3 if s < 18 else 11) + ((v >> n) & ((1 << CL_EXTRA[s]) - 1))
        n += CL_EXTRA.get(s, 0)
    return n


def verdict(stream, zdict=None):
    d = zlib.decompressobj(-15, zdict) if zdict else zlib.decompressobj(-15)
    try:
        raw = d.decompress(stream)
    except zlib.error:
        return None
    return raw if d.eof and not d.unused_data else None


# ---- pieces the catalogue is made of ---------------------------------------------------------------------------------------------------------
LIT3 = {97: 1, 256: 2, 257: 2}                  # 'a', end of block, length 3
NINE = 200                                      # a literal with a 9-bit fixed code


def shift(w, k):
    """a non-final fixed block of 9-bit literals behind which the next block begins at bit k of its byte"""
    fixed(w, [NINE] * ((k - 2 - w.n) % 8) + [EOB], final=False)
    assert w.n % 8 == k


def _one(build):
    w = BitWriter()
    build(w)
    return w.done()


def long_header(k, short=False, seven=False):
    """-> (stream, header bits, the bit the header starts at; short: three tokens behind it, the stream ends within 288 bytes of it): all
    316 lengths one by one, 7 bits for each of the 286 literal/length lengths, 6 for the 30 distance lengths: 2256 bits.  seven: 7 bits
    for those as well, 2286 bits, the longest header there is.  The lane kernel reads a header from 288 staged bytes, 5 more of them
    whenever fewer than 24 bits are left, and goes back to global memory once fewer than 8 staged bytes lie ahead: at 2256 bits only if
    its reads fall on staged byte 281 or 282 (they do not, at any of the eight offsets), at 2286 bits always."""
    w = BitWriter()
    shift(w, k)
    at = w.n
    lens = [8] * 226 + [9] * 60 + [4] * 2 + [5] * 28
    clens = [0] * 19
    for s, l in ({0: 1, 18: 2, 17: 3, 16: 4, 1: 5, 4: 7, 5: 7, 8: 7, 9: 7} if seven else {0: 1, 18: 2, 17: 3, 16: 4, 1: 6, 4: 6, 5: 6, 8: 7, 9: 7}).items():
        clens[s] = l
    tokens = [104, 105, EOB] if short else [104, 101, 97, 100, 101, 114, ("M", 5, 6), 250, ("M", 258, 1), ("M", 4, 12), EOB]
    hbits = dynamic(w, 286, 30, plain(lens), tokens, clens=clens, ncl=19)
    return w.done(), hbits, at


def crossing(nlit, coder):
    """eight 3-bit literal/length codes, the last three of them the alphabet's last symbols, and eight 3-bit distance codes: the run of
    threes goes on from one alphabet into the other"""
    w = BitWriter()
    lit = {s: 3 for s in (97, 98, 99, 100, 256, nlit - 3, nlit - 2, nlit - 1)}
    dyn(w, lit, {d: 3 for d in range(8)}, [97, 98, 99, 100, ("LS", nlit - 1, 0), ("DS", 0, 0), ("LS", nlit - 2, 0), ("DS", 3, 0), EOB], nlit=nlit, coder=coder)
    return w.done()


def crossing_257():
    """nlit = 257: 254, 255 and the end-of-block code are the last three, so the run crosses 255/256 and then the alphabet boundary"""
    w = BitWriter()
    lit = {s: 3 for s in (97, 98, 99, 100, 101, 254, 255, 256)}
    lens = [lit.get(s, 0) for s in range(257)]
    ops = rle(lens[:254]) + [(3, 0), (16, 3), (16, 1)]          # 254; 255, 256, d0..d3; d4..d7
    dynamic(w, 257, 8, ops, [97, 98, 254, 255, 101, 256])
    return w.done()


def fifteen():
    """both sets with lengths 1..15, 15 (complete), the end-of-block code and the only length symbol at 15 bits; code length 15 is the last
    entry of the code-length order, so HCLEN = 19"""
    w = BitWriter()
    stored(w, bytes(range(256)) + bytes(44), final=False)
    lit = {97 + i: i + 1 for i in range(14)} | {256: 15, 257: 15}
    dist = {i: i + 1 for i in range(14)} | {14: 15, 15: 15}
    tok = list(range(97, 111)) + [("M", 3, 1), ("LS", 257, 0), ("DS", 15, 0), ("LS", 257, 0), ("DS", 14, 63), ("LS", 257, 0), ("DS", 13, 5), EOB]
    dyn(w, lit, dist, tok)
    return w.done()


CLAIMED = tuple(range(1, 13))
WOULD_DECODE = {}              # refused catalogue entry -> the lengths its tokens would give were the refused construct let through (catalogue())

DICTS = {1: b"Q", 100: bytes((37 * i + 11) & 0xFF for i in range(100)), 32768: random.Random(5).randbytes(32768)}


@functools.lru_cache(maxsize=None)
def catalogue():
    out = []
    A = lambda name, s, zd=None: out.append((name, s, zd, "accept"))
    R = lambda name, s, zd=None, would=0: (out.append((name, s, zd, "reject")), WOULD_DECODE.update({name: would if isinstance(would, tuple) else (would,)} if would else {}))
    # ---- accepted ----
    A("run16-crossing-nlit257-and-255/256", crossing_257())
    for nlit in (260, 264, 269, 286):                                              # 264: a multiple of 8; the others are not
        A(f"run16-crossing-nlit{nlit}", crossing(nlit, rle))
    A("single-codes-crossing-nlit260", crossing(260, plain))
    A("single-codes-crossing-nlit269", crossing(269, lambda lens: rle(lens[:266]) + plain(lens[266:])))
    A("run16-crossing-255/256", _one(lambda w: dyn(w, {254: 2, 255: 2, 256: 2, 257: 2}, {0: 1, 1: 1}, [254, 255, ("M", 3, 2), 254, EOB])))
    A("one-distance-code-used", _one(lambda w: dyn(w, LIT3, {0: 1}, [97, ("M", 3, 1), 97, ("M", 3, 1), EOB])))
    A("hdist1-length0-literal-only", _one(lambda w: dyn(w, {97: 1, 256: 1}, {}, [97, 97, 97, EOB])))
    A("eob-only-final", _one(lambda w: dyn(w, {256: 1}, {}, [EOB])))
    A("eob-only-nonfinal-then-data", _one(lambda w: (dyn(w, {256: 1}, {}, [EOB], final=False), fixed(w, [100, 97, 116, 97, EOB]))))
    A("lengths-3-10-11-257-258-and-284+31", _one(lambda w: fixed(w, [97, ("M", 3, 1), 98, ("M", 10, 2), ("M", 11, 1), 99, ("M", 257, 3), ("M", 258, 1),
                                                                       100, ("LS", 284, 31), ("DS", 0, 0), ("LS", 284, 30), ("DS", 1, 0), EOB])))
    far = random.Random(6).randbytes(32768)
    A("distances-1-4-5-24577-32768", _one(lambda w: (stored(w, far, final=False), fixed(w, [("M", 3, 32768), ("M", 3, 1), ("M", 4, 4), ("LS", 257, 0), ("DS", 4, 0),
                                                                                                ("LS", 257, 0), ("DS", 4, 1), ("M", 5, 24577), ("M", 258, 32768), ("LS", 257, 0), ("DS", 29, 8191), EOB]))))
    A("15-bit-codes-hclen19", fifteen())
    cl7 = [0] * 19
    for s, l in {18: 1, 0: 2, 1: 3, 2: 4, 3: 5, 17: 6, 4: 7, 5: 7}.items():
        cl7[s] = l
    A("code-length-code-lengths-1-to-7", _one(lambda w: dyn(w, {97: 1, 98: 2, 99: 3, 100: 4, 256: 5, 257: 5}, {0: 1, 1: 1}, [97, 98, 99, 100, ("M", 3, 2), EOB], clens=cl7)))
    for k in range(8):
        A(f"final-block-ends-at-bit-{(10 + k) % 8}", _one(lambda w: fixed(w, [NINE] * k + [EOB])))
    A("empty-stored-final", _one(lambda w: stored(w, b"")))
    A("empty-fixed-final", _one(lambda w: fixed(w, [EOB])))
    A("empty-blocks-between-data", _one(lambda w: (stored(w, b"", final=False), fixed(w, [115, 121, 110, 99, EOB], final=False), fixed(w, [EOB], final=False),
                                                    stored(w, b"", final=False), dyn(w, LIT3, {0: 1, 1: 1}, [97, ("M", 3, 1), EOB], final=False),
                                                    dyn(w, {97: 1, 256: 1}, {}, [EOB], final=False), stored(w, b"flush", final=False), stored(w, b""))))
    A("stored-65535", _one(lambda w: stored(w, random.Random(7).randbytes(65535))))
    A("300-one-literal-blocks", _one(lambda w: [fixed(w, [33 + i % 90, EOB], final=i == 299) for i in range(300)]))
    for k in range(8):
        A(f"second-dynamic-header@{k}", _one(lambda w: (shift(w, k), dyn(w, {97: 2, 98: 2, 256: 2, 258: 2}, {0: 1, 2: 1}, [97, 98, ("M", 4, 1), ("M", 4, 3), EOB]))))
    for k in range(8):
        s, hbits, _ = long_header(k)
        A(f"longest-header@{k} ({hbits} header bits)", s)
        A(f"longest-header-short@{k} ({hbits} header bits)", long_header(k, short=True)[0])
        s, hbits, _ = long_header(k, seven=True)
        A(f"longest-header-all-7-bit@{k} ({hbits} header bits)", s)
    for dl, zd in DICTS.items():
        for pos in (0, 5) if dl < 32768 else (0,):                                     # (no distance above 32768 can be written)
            A(f"dict{dl}-dist=pos+Dl@pos{pos}", _one(lambda w: fixed(w, [120] * pos + [("M", 3, pos + dl), EOB])), zd)
        for k in (1, 3, 15, 16, 17):
            for pos in (0, 2):
                if k <= dl:
                    A(f"dict{dl}-258-from-last-{k}-bytes@pos{pos}", _one(lambda w: fixed(w, [121] * pos + [("M", 258, pos + k), 122, EOB])), zd)
    # ---- rejected ----
    junk = ("R", 0x5A5A5A5A, 32)
    R("block-type-3", _one(lambda w: (w.bits(1, 1), w.bits(3, 2), w.bits(0, 29))))
    R("stored-len-not-nlen", _one(lambda w: stored(w, b"hello", nlen=0xFFFB)), would=5)
    R("stored-longer-than-stream", _one(lambda w: stored(w, b"hello", length=10)), would=10)
    # A decoder is told the raw length, and refuses whatever decodes to another: behind a header that zlib refuses stands nothing but
    # the end-of-block code the header would define, so that a decoder which lets the header pass ACCEPTS (0 bytes, as told).
    R("hlit-above-286", _one(lambda w: dyn(w, LIT3, {0: 1, 1: 1}, [EOB], hlit=30)))
    R("hdist-above-30", _one(lambda w: dyn(w, LIT3, {0: 1, 1: 1}, [EOB], hdist=30)))
    eob_only = plain([0] * 256 + [1, 0])                                           # the allowed one-code set, coded with single codes
    for name, cl in (("incomplete", {0: 2, 1: 2}), ("over-subscribed", {0: 1, 1: 1, 2: 1})):
        R(f"code-length-code-{name}", _one(lambda w: dynamic(w, 257, 1, eob_only, [EOB], clens=[cl.get(s, 0) for s in range(19)])))
    R("code-length-code-all-zero", _one(lambda w: dynamic(w, 257, 1, [], [junk] * 12, clens=[0] * 19)))
    R("repeat16-first", _one(lambda w: dynamic(w, 257, 1, [(16, 0)] + rle([0] * 253) + [(1, 0), (0, 0)], [EOB])))       # read as zeros it would be complete
    R("run-past-the-end-by-1", _one(lambda w: dynamic(w, 258, 2, rle([0] * 256) + [(1, 0), (16, 1)], [EOB])))
    R("no-end-of-block-code", _one(lambda w: dyn(w, {97: 1, 98: 1}, {0: 1, 1: 1}, [97, 98, junk])))
    R("litlen-incomplete-longest-2", _one(lambda w: dyn(w, {97: 2, 256: 2}, {0: 1, 1: 1}, [EOB])))
    R("litlen-over-subscribed", _one(lambda w: dyn(w, {97: 1, 98: 1, 256: 1}, {0: 1, 1: 1}, [EOB])))
    R("dist-incomplete-two-of-length-2", _one(lambda w: dyn(w, LIT3, {0: 2, 1: 2}, [EOB])))
    R("dist-over-subscribed", _one(lambda w: dyn(w, LIT3, {0: 1, 1: 1, 2: 1}, [EOB])))
    R("unused-code-of-one-distance-code", _one(lambda w: dyn(w, LIT3, {0: 1}, [97, 257, ("C", 1, 1), 97, EOB])), would=(4, 5))
    R("unused-code-of-eob-only-set", _one(lambda w: dyn(w, {256: 1}, {}, [("C", 1, 1), EOB])))
    R("length-symbol-without-distance-code", _one(lambda w: dyn(w, LIT3, {}, [97, 257, ("R", 0, 1), EOB])), would=4)
    for s in (286, 287):
        R(f"fixed-symbol-{s}", _one(lambda w: fixed(w, [97, s, ("R", 0, 5), EOB])), would=1)
    for d in (30, 31):
        R(f"fixed-distance-symbol-{d}", _one(lambda w: fixed(w, [97, 257, ("DS", d, 0), EOB])), would=4)
    R("dist=pos+1-no-dictionary", _one(lambda w: fixed(w, [97, 98, ("M", 3, 3), EOB])), would=5)
    for dl, zd in DICTS.items():
        if dl == 32768:
            continue                  # pos + Dl + 1 > 32768 = the largest distance DEFLATE can write: with a full window there is no such stream
        for pos in (0, 5):
            R(f"dict{dl}-dist=pos+Dl+1@pos{pos}", _one(lambda w: fixed(w, [120] * pos + [("M", 3, pos + dl + 1), EOB])), zd, would=pos + 3)
    R("one-byte-behind-the-final-block", _one(lambda w: fixed(w, [97, EOB])) + b"\0", would=1)
    R("one-bit-short-of-the-final-block", _one(lambda w: fixed(w, [NINE] * 7 + [EOB]))[:-1], would=7)          # 17 bits, 16 of them there
    assert len({e[0] for e in out}) == len(out) and {n for v in WOULD_DECODE.values() for n in v} <= set(CLAIMED)
    return tuple(out)


def two_blocks():
    """-> (stream, bit at which the second dynamic header starts: not a multiple of 8)"""
    w = BitWriter()
    dyn(w, {97: 2, 98: 2, 256: 2, 258: 2}, {0: 1, 2: 1}, [97, 98, ("M", 4, 1), ("M", 4, 3), 97, 98, EOB], final=False)
    at = w.n
    assert at % 8
    dyn(w, {s: 3 for s in (97, 98, 99, 100, 256, 257, 258, 259)}, {d: 3 for d in range(8)}, [99, 100, ("M", 5, 2), ("M", 3, 9), 98] + [97, 99, 100] * 8 + [EOB])
    return w.done(), at


def _deflate(raw, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(raw) + c.flush()


def seeds():
    """[(name, stream, [(first bit, bits) to mutate])]"""
    cat = {e[0]: e[1] for e in catalogue()}
    span = lambda s, at=0: (at, header_bits(s, at) + 64)
    out = []
    for name, s in (("zlib-level9", _deflate(ref.text(21, 2048), 9, zlib.Z_DEFAULT_STRATEGY)), ("zlib-huffman-only", _deflate(ref.text(22, 768).hex().encode(), 9, zlib.Z_HUFFMAN_ONLY)),
                    ("longest-header", long_header(0)[0]), ("crossing-run", cat["run16-crossing-nlit269"]), ("15-bit", cat["15-bit-codes-hclen19"])):
        at = 8 * (5 + 300) if name == "15-bit" else long_header(0)[2] if name == "longest-header" else 0    # behind the stored / the shifting block
        out.append((name, s, [span(s, at)]))
    s, at = two_blocks()
    out.append(("two-blocks", s, [span(s), span(s, at)]))
    # The six seeds above are nearly all header, and hardly any flip inside a header leaves a complete code: zlib accepts 5 % of their
    # mutants (the Z_HUFFMAN_ONLY one is 1.5 KiB of hex digits: a dense header over ref.text adds 900 more that zlib refuses).  Eight more, a short header at each bit offset with nothing but 3-bit literals behind it (seven of the eight codes are
    # literals, so most payload flips decode), bring the accepted share above the floor.
    for k in range(8):
        w = BitWriter()
        shift(w, k)
        at = w.n
        dyn(w, {s: 3 for s in (97, 98, 99, 100, 101, 102, 103, 256)}, {}, [97, 98, 99, 100, 101, 102, 103] * 4 + [EOB])
        out.append((f"literals@{k}", w.done(), [span(w.done(), at)]))
    return out


@functools.lru_cache(maxsize=None)
def flip_family():
    out = []
    for name, s, spans in seeds():
        flips = sorted({b for at, bits in spans for b in range(at, min(at + bits, 8 * len(s)))})
        cuts = sorted({c for at, bits in spans for c in range((at + 7) // 8, min((at + bits) // 8, len(s)) + 1)})
        for b in flips:
            m = bytearray(s); m[b >> 3] ^= 1 << (b & 7)
            out.append((f"{name}:flip{b}", bytes(m)))
        out += [(f"{name}:cut{c}", s[:c]) for c in cuts]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def catalogue_raws():
    """zlib's answer for every catalogue entry, computed once"""
    return tuple(verdict(s, zd) for _, s, zd, _ in catalogue())


@functools.lru_cache(maxsize=None)
def family_raws():
    return tuple(verdict(s) for _, s in flip_family())


def wrapped(entries_and_raws):
    """gzip members around (stream, raw | None) pairs: a rejected stream is wrapped with raw = b"" """
    return [ref.member(raw or b"", stream=s) for s, raw in entries_and_raws]


def emu_case():
    """the catalogue as one case of tools/gunzip_emu.py::cases(): (the wrapped entries one behind the other, where each begins).  Left out
    as too slow for one std::thread per lane: the 65 535-byte stored block and the 300-block stream (SLOW)."""
    members = wrapped((e[1], r) for e, r in zip(catalogue(), catalogue_raws()) if e[0] not in SLOW)
    offs = [0]
    for m in members[:-1]:
        offs.append(offs[-1] + len(m))
    return b"".join(members), offs


def records(vectors, raws, claimed=()):
    """[(name, stream, zdict | None, ...)] and zlib's answers -> ([(stream, raw_len, base record or -1)], index of the first vector's record):
    a vector with a dictionary is a DELTA record whose base is a stored record of that dictionary, in front of all the others; the raw
    length handed to the decoder is the length zlib produced (0 where it refuses).
    A decoder that is told 0 refuses at the first byte it decodes, whatever stands behind it — so with `claimed`, every stream zlib refuses
    follows once more per claimed raw length, behind all the vectors: refused at every one of them.  claimed = the lengths, for every
    refused vector (CLAIMED: 1..12), or {name: length} (WOULD_DECODE: a record more for each of those)."""
    base_of, recs = {}, []
    for zd in DICTS.values():
        base_of[zd] = len(recs)
        recs.append((_one(lambda w: stored(w, zd)), len(zd), -1))
    first = len(recs)
    for v, raw in zip(vectors, raws):
        recs.append((v[1], len(raw or b""), base_of[v[2]] if len(v) > 2 and v[2] else -1))
    for n in sorted({n for v in claimed.values() for n in v}) if isinstance(claimed, dict) else claimed:
        recs += [(v[1], n, base_of[v[2]] if len(v) > 2 and v[2] else -1) for v, raw in zip(vectors, raws)
                 if raw is None and (not isinstance(claimed, dict) or n in claimed.get(v[0], ()))]
    return recs, first


def pack(recs):
    """-> streams, stream_off, kind, base, raw_len: the dense arrays of hmse_l1_inflate / orc.inflate_chunks"""
    import numpy as np
    streams = np.frombuffer(b"".join(r[0] for r in recs) + b"\0", np.uint8)[:-1].copy()
    off = np.concatenate([[0], np.cumsum([len(r[0]) for r in recs])]).astype(np.int64)
    base = np.array([r[2] for r in recs], np.int64)
    return streams, off, np.where(base >= 0, 2, 0).astype(np.uint8), base, np.array([r[1] for r in recs], np.int64)
