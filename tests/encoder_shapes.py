"""Inputs that reach the branches of the DEFLATE encoder's Huffman stage that text, random bytes and small alphabets never take
(l1_encode_kernel with huff_lengths_wave, huff_codes_wave and rle_tree_wave in hmse_amd/csrc/l1_deflate.hip): the Kraft repair of all
three trees, every remainder class of the closed-form code-length RLE, the dummy symbols of a distance tree with fewer than two used
codes, the ends of nlit / ndist / ncl, ties between the three block types in bits, and tokens wider than a dword.

Pure numpy and oracle/pyref.py, seeded, no device, no fixtures.  cases() returns named (chunk, dictionary or None) pairs; witness()
computes FROM THE REFERENCE ONLY (never hmse_amd) what a pair reaches, and tests/test_encoder_shapes_host.py asserts the class every
pair was built for, so that a builder which stops reaching its branch fails there.  tests/test_gpu_encoder_shapes.py and
tests/enc_spill_check.py run the same pairs through the kernels.  All witnesses are for the default configuration (level 9).

Which encode launch a case takes: hmse_l1_deflate runs l1_encode_kernel<0, 12288> on the records of chunks of at most 12 288 bytes and
l1_encode_kernel<12288, 32768> on the longer ones.  A literal/length or distance tree deeper than 15 needs Fibonacci counts over
seventeen symbols, about 4 180 matches: such a chunk is longer than 12 288 bytes, so W1, W2 and W9 exist in the second list only; the
code-length tree's repair (W3) and everything else is present in both.

What cannot be reached: a zero run of 276 or more (two full 18s).  The end-of-block code is always used, so the longest zero run of the
literal/length lengths is 0 .. 255 of a job without a literal (256: one full 18 and an 18 for 118), and the distance tree has 30 codes.
Index 257 (length 3) is never used by an encoder whose shortest match is 4, so no non-zero run crosses 256 / 257.  The smallest ncl is
12: a complete tree over at most 30 distance codes has a length of 4 or less, and of 1 .. 4 the header's order lists 4 first, twelfth."""
from __future__ import annotations

import functools

import numpy as np

from oracle import pyref

FIB17 = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


# ---- the witness ------------------------------------------------------------------------------------------------------------------
def _depths(freq, limit):
    """-> (unclamped maximum depth, how often rule 5's repair loop runs) of the tree over `freq`"""
    raw = [d for d in pyref.huffman_lengths(freq, 40) if d]
    total = sum(1 << (limit - min(d, limit)) for d in raw)
    return max(raw), max(0, total - (1 << limit))


def _runs(lens, tree):
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        out.append((tree, i, lens[i], j - i))
        i = j
    return out


def _rle_at(lens, tree):
    """rule 6's tokens of one tree, each with the index in `lens` at which it starts: (tree, index, symbol, extra bits, extra value)"""
    out, i = [], 0
    for s, eb, ev in pyref.rle_code_lengths(lens):
        out.append((tree, i, s, eb, ev))
        i += {16: 3 + ev, 17: 3 + ev, 18: 11 + ev}.get(s, 1)
    assert i == len(lens)
    return out


def witness(chunk: bytes, dictionary: bytes | None = None) -> dict:
    """What the default encoder reaches on this job, restated from oracle/pyref.py's parts (costs recomputed as in pyref.deflate)."""
    mlen, mdist = pyref.lz_matches(chunk, dictionary or b"", 32)
    toks = pyref.lz_parse(chunk, mlen, mdist)
    lf, df, extra = [0] * 286, [0] * 30, 0
    for a, d in toks:
        if d:
            c, eb, _ = pyref._len_code(a)
            lf[c] += 1
            extra += eb
            c, eb, _ = pyref._dist_code(d)
            df[c] += 1
            extra += eb
        else:
            lf[a] += 1
    lf[256] += 1
    ll, dl = pyref.huffman_lengths(lf, 15), pyref.huffman_lengths(df, 15)
    nlit = max(257, max(s + 1 for s in range(286) if ll[s]))
    ndist = max(1, max((s + 1 for s in range(30) if dl[s]), default=1))
    rle = _rle_at(ll[:nlit], 0) + _rle_at(dl[:ndist], 1)
    cf = [0] * 19
    for _, _, s, _, _ in rle:
        cf[s] += 1
    cl = pyref.huffman_lengths(cf, 7)
    ncl = max(4, max(i + 1 for i in range(19) if cl[pyref._CL_ORDER[i]]))
    hdr_bits = 3 + 14 + 3 * ncl + sum(cl[s] + eb for _, _, s, eb, _ in rle)
    dyn_bits = hdr_bits + extra + sum(f * ll[s] for s, f in enumerate(lf)) + sum(f * dl[s] for s, f in enumerate(df))
    fixed_bits = 3 + extra + sum(f * FIXED_LL[s] for s, f in enumerate(lf)) + 5 * sum(df)
    stored_bits = 8 * (5 + len(chunk))
    if stored_bits <= fixed_bits and stored_bits <= dyn_bits:
        block, bits = 0, stored_bits
    elif fixed_bits <= dyn_bits:
        block, bits = 1, fixed_bits
    else:
        block, bits = 2, dyn_bits
    # token widths of the chosen code, and the puts that touch three dwords of the image: (bit offset mod 32) + bits > 64
    widest, three, off = 0, 0, hdr_bits if block == 2 else 3
    if block:
        wl, wd = (ll, dl) if block == 2 else (FIXED_LL, [5] * 30)
        for a, d in toks:
            if d:
                c, eb, _ = pyref._len_code(a)
                c2, eb2, _ = pyref._dist_code(d)
                b = wl[c] + eb + wd[c2] + eb2
            else:
                b = wl[a]
            widest = max(widest, b)
            three += (off & 31) + b > 64
            off += b
    dmax = [_depths(lf, 15), _depths(df, 15), _depths(cf, 7)]
    return dict(tokens=len(toks), matches=sum(1 for _, d in toks if d), lf=lf, df=df, cf=cf, ll=ll, dl=dl, cl=cl,
                depth=tuple(d for d, _ in dmax), repairs=tuple(r for _, r in dmax), nlit=nlit, ndist=ndist, ncl=ncl,
                rle=rle, runs=_runs(ll[:nlit], 0) + _runs(dl[:ndist], 1), dist_token_base=sum(1 for r in rle if r[0] == 0),
                stored_bits=stored_bits, fixed_bits=fixed_bits, dyn_bits=dyn_bits, block=block, stream_len=(bits + 7) // 8,
                widest_token=widest, three_dword_puts=three)


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def random_dictionary(seed: int) -> np.ndarray:
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, 32768, dtype=np.uint8)


def deletion_job(seed: int, lengths, counts):
    """W1.  The chunk is a random 32 768-byte dictionary with one byte deleted behind every copy: counts[i] copies of lengths[i] bytes,
    in shuffled order.  The deleted byte is first made to differ from its successor, so no match extends and no literal appears: the
    literal/length histogram is exactly `counts` plus the end-of-block code.  Every distance is 32 768 minus the deletions so far."""
    rng = np.random.Generator(np.random.PCG64(seed))
    D = random_dictionary(seed + 1)
    order = rng.permutation(np.repeat(np.asarray(lengths), np.asarray(counts)))
    assert int(order.sum()) + order.size <= D.size
    parts, q = [], 0
    for n in order.tolist():
        if q + n + 1 < D.size and D[q + n] == D[q + n + 1]:
            D[q + n] ^= 0x55
        parts.append(D[q: q + n])
        q += n + 1
    return np.concatenate(parts).tobytes(), D.tobytes()


def distance_job(seed: int, counts: dict, lengths=None, prefix: bytes = b"", suffix: bytes = b""):
    """W2.  counts[code] copies with a distance of that code, smallest code first (a code can only be used while the chunk offset is
    below its largest distance), every copy from a dictionary source of its own.  Sources of the copies of one code form one pool, laid
    out pairwise swapped (the pool holds copy 1, copy 0, copy 3, copy 2, ...): consecutive copies never come from consecutive sources,
    so they do not fuse into one match, no source byte is wasted on gaps, and the distance stays within a copy length of one value.
    With one distance D0 per code (every copy of the code lies within a copy length of it) the pool of a code is its stretch of the
    chunk moved back by D0, so pools are disjoint, the larger code the lower, when D0 grows from one code to the next by the sizes of
    both pools; each code takes the smallest D0 that its range, the dictionary's end and its predecessor allow.
    `lengths` (default: all 4) gives every copy's length in chunk order; `prefix` and `suffix` are literal material in front of and
    behind the copies."""
    codes = sorted(counts)
    n = sum(counts.values())
    lengths = [4] * n if lengths is None else list(lengths)
    assert len(lengths) == n
    D = random_dictionary(seed)
    dl = D.size
    plan, c, i = [], len(prefix), 0            # per code: (code, chunk offset of its first copy, lengths of its copies)
    for code in codes:
        mine = lengths[i: i + counts[code]]
        plan.append((code, c, mine))
        c += sum(mine); i += len(mine)
    src, d0, before = {}, 0, 0
    for code, c0, mine in plan:
        lo = pyref._DIST_BASE[code]
        hi = pyref._DIST_BASE[code + 1] - 1 if code < 29 else 32768
        slack, size = max(mine), sum(mine)
        d0 = max(lo + slack, c0 + size, d0 + before + size)   # distances stay within [d0 - slack, d0 + slack]
        assert d0 + slack <= hi, ("no room for distance code", code)
        P, before = dl + c0 - d0, size
        at, q = [], P
        for j in range(0, len(mine), 2):
            pair = mine[j: j + 2]
            if len(pair) == 2:
                at += [q + pair[1], q]                   # the pool holds the second copy of a pair first
            else:
                at.append(q)
            q += sum(pair)
        src[code] = at
    copies = [(q, n) for code, c0, mine in plan for q, n in zip(src[code], mine)]
    for turn in range(16):                               # no copy may extend into the next one: the byte behind its source differs
        clash = [b[0] for a, b in zip(copies, copies[1:]) if a[0] + a[1] < dl and D[a[0] + a[1]] == D[b[0]]]
        if not clash:
            break
        for q in clash:
            D[q] = (int(D[q]) + 1 + 2 * turn) & 255
    assert not clash
    parts = [np.frombuffer(prefix, np.uint8)] + [D[q: q + n] for q, n in copies] + [np.frombuffer(suffix, np.uint8)]
    return np.concatenate(parts).tobytes(), D.tobytes()


def alphabet_chunk(seed: int, lens: dict, k: int, tail: bytes = b"") -> bytes:
    """A chunk of literals whose literal/length tree gets exactly the code lengths `lens` {byte value: length}: the lengths, with the
    end-of-block code at the longest of them, must fill the Kraft sum; a byte of length l occurs k << (longest - l) times, which the
    two-queue Huffman turns back into l (the end-of-block code, counted once, stands in for a symbol counted k times: it lowers one
    node of every level below the level's weight and changes no depth).  Arranged by no_repeated_4gram; `tail` follows as it is."""
    top = max(lens.values())
    assert sum(1 << (top - l) for l in lens.values()) + 1 == 1 << top, "lengths and the end-of-block code must fill the Kraft sum"
    body = np.concatenate([np.full(k << (top - l), b, np.uint8) for b, l in sorted(lens.items())])
    return no_repeated_4gram(seed, body) + tail


def layout(*runs) -> dict:
    """(first byte value, count, length) ... -> {byte value: length}"""
    out = {}
    for first, count, length in runs:
        for b in range(first, first + count):
            assert b not in out and b < 256
            out[b] = length
    return out


def no_repeated_4gram(seed: int, body: np.ndarray) -> bytes:
    """`body` shuffled, then mended from the front (a byte that would complete a 4-gram seen before swaps with a later one): no 4-gram
    occurs twice, so the matcher finds nothing and the parse is all literals, whatever the length."""
    rng = np.random.Generator(np.random.PCG64(seed))
    b = rng.permutation(body).tolist()
    seen, n = set(), len(b)
    for i in range(3, n):
        for _ in range(64):
            g = (b[i - 3], b[i - 2], b[i - 1], b[i])
            if g not in seen or i + 1 >= n:
                break
            j = int(rng.integers(i + 1, n))
            b[i], b[j] = b[j], b[i]
        seen.add(g)
    return bytes(b)


def spread_layout(n: dict, long_runs, gaps) -> dict:
    """{byte value: length} for the code-length tree cases: n[length] symbols of each length (the end-of-block code counts among the
    longest), `long_runs` [(length, run)] first, then the rest interleaved so that no other run of equal lengths is longer than 3 (each
    symbol of such a run is one code-length token of its own), the zero runs `gaps` spread between them, zeros up to index 255."""
    left = dict(n)
    left[max(left)] -= 1
    seq = []
    for length, run in long_runs:
        seq += [length] * run
        left[length] -= run
    while any(left.values()):
        prev = seq[-1] if seq else 0
        pick = max((l for l in left if left[l] and l != prev), key=lambda l: (left[l], l), default=prev)
        seq.append(pick)
        left[pick] -= 1
    first = sum(r for _, r in long_runs) + 2
    where = {first + k * ((len(seq) - first - 2) // len(gaps)): g for k, g in enumerate(gaps)}
    out, at = {}, 0
    for i, length in enumerate(seq):
        at += where.get(i, 0)
        out[at] = length
        at += 1
    assert at <= 256 - 11
    return out


def repeated_tail(seed: int, hi: int, length: int, tail: int) -> bytes:
    """random bytes below `hi` whose last `tail` bytes repeat the first ones: the sizes around the break-even of the block types"""
    c = np.random.Generator(np.random.PCG64(seed)).integers(0, hi, length, dtype=np.uint8)
    if tail:
        c[length - tail:] = c[:tail]
    return c.tobytes()


def gap_layout(start: int, run: int) -> dict:
    """every byte value except [start, start + run): one long zero run in the literal/length lengths.  Lengths 6 (the lowest values)
    and 7 (the rest: the last of them and the end-of-block code form a non-zero run across 255 / 256)."""
    used = [b for b in range(256) if not start <= b < start + run]
    short = 128 - (len(used) + 1)
    return {b: 6 if i < short else 7 for i, b in enumerate(used)}


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
W1_LENGTHS = (4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35)          # sixteen distinct length codes
FIB_DIST = dict(zip(range(13, 30), FIB17))                                         # distance codes 13 .. 29

# literal alphabets for the code-length RLE: (first value, count, length) runs of equal lengths, zero runs between them
RLE_A = layout((0, 1, 7), (2, 2, 7), (6, 3, 7), (12, 4, 7), (26, 6, 7), (43, 7, 7), (50, 8, 8), (58, 9, 7), (67, 10, 8), (80, 60, 7), (140, 53, 8))
RLE_B = layout((0, 63, 7), (63, 1, 8), (64, 5, 7), (73, 12, 8), (94, 13, 7), (119, 14, 8), (138, 15, 7), (160, 36, 8))
GAPS = {138: 63, 139: 64, 140: 60, 141: 62, 148: 50, 149: 55}                      # zero run -> where it starts
# code-length histograms 1 1 2 3 5 8 13 21 34 [55] over symbols 17, 16 | 18, 1 (both distance lengths), 18 | 16, 0 and four | five lengths
CL_DEPTH_8 = ({5: 14, 6: 21, 7: 13, 8: 34}, [(5, 7)], [1, 2, 2, 5, 30, 40])
CL_DEPTH_9 = ({5: 12, 6: 13, 7: 21, 8: 37, 9: 58}, [(5, 5), (9, 4), (8, 4)], [1, 2, 2, 7])
# found by search over (seed, alphabet, length, tail) with witness(): equal costs in bits, not merely in bytes
TIES = {"w8-stored-eq-fixed": (1, 256, 392, 18), "w8-stored-eq-dynamic": (4, 256, 1125, 54), "w8-fixed-eq-dynamic": (1, 256, 1100, 96)}


def _wide(rare, swap):
    """W9: distance codes 29 .. 19 with counts 1 1 2 3 ... 89, so the codes with 13 extra bits are the rare, long ones; the copies of
    the rare distance codes are also the rare, long lengths (5, 4 and 2 or 3 extra bits)."""
    counts = dict(zip(range(29, 18, -1), FIB17[:11]))
    a, b, c = rare
    lengths = [4] * 89 + [5] * 55 + [6] * 34 + [7] * 21 + [8] * 13 + [9] * 8 + [10] * 5 + [c] * 3 + [b, b] + ([4, a] if swap else [a, 4])
    return distance_job(4, counts, lengths)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name -> (chunk, dictionary or None), in a fixed order"""
    out = {}
    out["w1-litlen-depth-16"] = deletion_job(1, W1_LENGTHS, FIB17[::-1][:16])
    out["w2-dist-depth-16"] = distance_job(2, FIB_DIST)
    per = [l for l, n in zip((11, 19, 13, 15, 17, 10, 9, 8, 7, 6, 5), FIB17[1:]) for _ in range(n)]
    out["w9-both-trees-deep"] = distance_job(3, FIB_DIST, per + [4] * (sum(FIB17) - len(per)))
    out["w9-wide-38"] = _wide((163, 131, 23), False)
    out["w9-wide-36-twice"] = _wide((43, 131, 23), True)
    out["w3-cl-depth-8"] = (alphabet_chunk(1, spread_layout(*CL_DEPTH_8), 8), None)
    out["w3-cl-depth-8-long"] = (alphabet_chunk(1, spread_layout(*CL_DEPTH_8), 50), None)
    out["w3-cl-depth-9"] = (alphabet_chunk(1, spread_layout(*CL_DEPTH_9), 4), None)
    out["w3-cl-depth-9-long"] = (alphabet_chunk(1, spread_layout(*CL_DEPTH_9), 25), None)
    out["w7-rle-a"] = (alphabet_chunk(0, RLE_A, 12), None)
    out["w7-rle-b"] = (alphabet_chunk(0, RLE_B, 12), None)
    for run, start in GAPS.items():
        out[f"w7-zero-run-{run}"] = (alphabet_chunk(run, gap_layout(start, run), 16), None)
    out["w5-only-distance-code-0"] = (alphabet_chunk(0, RLE_B, 12, bytes([200]) * 300), None)        # also nlit = 286
    out["w5-one-distance-code-5"] = (alphabet_chunk(0, RLE_B, 12, bytes(range(160, 167)) * 9), None)
    out["w6-ncl-12"] = distance_job(7, {c: 4 for c in range(14, 30)}, suffix=alphabet_chunk(0, RLE_A, 4))
    for name, args in TIES.items():
        out[name] = (repeated_tail(*args), None)
    assert all(len(c) <= 32768 for c, _ in out.values())
    return out


@functools.lru_cache(maxsize=None)
def witnesses() -> dict:
    return {name: witness(c, d) for name, (c, d) in cases().items()}


# parity-only twins: a literal-alphabet case with another case's chunk as its dictionary (the last pair shares its body: anchors and hints)
TWINS = (("w7-rle-a", "w7-rle-b"), ("w3-cl-depth-9", "w3-cl-depth-8"), ("w7-zero-run-138", "w7-zero-run-149"),
         ("w3-cl-depth-8-long", "w7-rle-a"), ("w5-one-distance-code-5", "w5-only-distance-code-0"))


@functools.lru_cache(maxsize=None)
def batch():
    """All cases as one hmse_l1_deflate selection -> (data uint8[n], cuts uint64[k + 1], base int64[k], names): the cases in order, each
    dictionary once as a chunk of its own (base = its index), then the twins."""
    parts, base, names, index = [], [], [], {}

    def add(name, chunk, b=-1):
        index[name] = len(parts)
        parts.append(np.frombuffer(chunk, np.uint8)); base.append(b); names.append(name)

    todo = []
    for name, (chunk, zdict) in cases().items():
        if zdict is None:
            add(name, chunk)
        else:
            todo.append((name, chunk, zdict))
    held = {}
    for name, chunk, zdict in todo:
        if zdict not in held:
            held[zdict] = len(parts)
            add("dictionary-of-" + name, zdict)
        add(name, chunk, held[zdict])
    for name, other in TWINS:
        add(name + "+" + other, cases()[name][0], index[other])
    cuts = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return np.concatenate(parts), cuts, np.asarray(base, np.int64), tuple(names)
