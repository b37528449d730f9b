"""Inputs of tests/test_anchor_inputs_host.py, tests/test_gpu_dict_anchors.py and tests/dict_anchor_check.py: DICTIONARY DEFLATE jobs built to
reach every branch of the anchor phase (phase 4b of the match kernel): the bucket search of an anchor, the choice of the
nearest dictionary member that agrees on 32 bytes among the bucket's 64 nearest, and the runs along its diagonal.  Jobs have the form
test_gpu_edges.run_jobs takes (dict_handout_inputs.make_job's).

Every job carries what its content is built to make of ONE anchor, in job["expect"][j] = (block a, dictionary members of the anchor's
bucket or None = not said, distance or 0 = no anchor, forward run or None, backward extent or None); `witness` computes the same from
oracle/pyref.py::lz_anchors and a plain bucket count, and tests/test_anchor_inputs_host.py holds the two against each other.

A MARKER is a 4-gram of bytes no filler holds; the dictionary repeats it once per wanted bucket member, the anchor position carries it.  A
member AGREES when the anchor's 32 bytes follow its marker as well: agreeing members are followed by the whole chunk, so the delta is small
and the chosen distance shows in the stream."""
from __future__ import annotations

import numpy as np

import dict_handout_inputs as H
from oracle import pyref

CAPS = H.CAPS
MARKER = bytes([0xF1, 0xF2, 0xF3, 0xF4])
STRIDE = 40                                       # bytes per member that does not agree: marker, one byte that differs, filler
MUL, M32 = 0x9E3779B1, 0xFFFFFFFF

_TEXT = H.words_text(140_000, seed=29)


def hash4(b: bytes) -> int:
    return ((int.from_bytes(b[:4], "little") * MUL) & M32) >> 20


def _rng(salt: int):
    return np.random.Generator(np.random.PCG64(9100 + salt))


def _fill(rng, n: int) -> bytes:
    """Lower-case letters without structure: no 32 bytes of it occur twice."""
    return bytes(rng.integers(97, 123, n, dtype=np.uint8))


def gram_of_bucket(h: int) -> bytes:
    """The first 4-gram of upper-case letters and digits (none in any filler) whose hash is h."""
    abc = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    for a in abc:
        for b in abc:
            for c in abc:
                for d in abc:
                    g = bytes([a, b, c, d])
                    if hash4(g) == h:
                        return g
    raise ValueError(h)


def job_of(pairs, expect) -> dict:
    """pairs: (chunk bytes, dictionary bytes) per job -> the dict of dict_handout_inputs.make_job, plus expect."""
    parts, ids, base, Ts = [], [], [], []
    for c, d in pairs:
        assert len(c) >= 1 and len(d) >= 1
        parts.append(np.frombuffer(bytes(d), np.uint8).copy()); base.append(len(parts) - 1)
        parts.append(np.frombuffer(bytes(c), np.uint8).copy()); ids.append(len(parts) - 1)
        Ts.append(len(c) + min(len(d), 32768))
    lens = np.array([p.size for p in parts], dtype=np.uint64)
    return {"data": np.concatenate(parts), "cuts": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), "ids": np.array(ids, np.uint64),
            "base": np.array(base, np.int64), "T": np.array(Ts), "parts": parts, "promise": [None] * len(ids), "expect": list(expect)}


def _clean(buf: bytearray, mutable: np.ndarray, h: int, keep: set, rng, tail: bytes = b"") -> bytes:
    """Redraw filler bytes until no position of buf (read on into `tail`) but those in `keep` has a 4-gram of bucket h: the bucket holds what
    the builder put there and nothing the hash happened to add."""
    for _ in range(10000):
        w = bytes(buf) + tail
        stray = [q for q in range(len(w) - 3) if q < len(buf) and q not in keep and hash4(w[q:q + 4]) == h]
        if not stray:
            return bytes(buf)
        for q in stray:
            at = [x for x in range(q, min(q + 4, len(buf))) if mutable[x]]
            assert at, "a stray bucket member inside bytes the builder may not change"
            buf[at[-1]] = int(rng.integers(97, 123))
    raise AssertionError("no clean filler found")


def members_dict(chunk: bytes, n: int, agree=(), near31=(), salt=0, marker=MARKER, head=64) -> bytes:
    """A dictionary whose bucket of `marker` holds n members, numbered from the NEAREST (0) to the farthest (n - 1): members in `agree` are
    followed by the whole chunk (whose first four bytes are the marker), members in `near31` by its first 31 bytes and another 32nd, all
    others differ at once behind the marker.  `head` bytes of filler in front.  Exactly n: filler that fell into the bucket is redrawn."""
    assert chunk[:4] == marker and len(chunk) >= 36
    rng = _rng(1000 + salt)
    out, mut, keep, at = [_fill(rng, head)], [np.ones(head, bool)], set(), head
    for i in range(n - 1, -1, -1):
        if i in agree:
            rec, m = chunk, np.zeros(len(chunk), bool)
        elif i in near31:
            rec, m = chunk[:31] + bytes([chunk[31] ^ 0x01]) + _fill(rng, 8), np.concatenate([np.zeros(32, bool), np.ones(8, bool)])
        else:
            rec, m = marker + bytes([chunk[4] ^ 0x80]) + _fill(rng, STRIDE - 5), np.concatenate([np.zeros(5, bool), np.ones(STRIDE - 5, bool)])
        keep.add(at); at += len(rec)
        out.append(rec); mut.append(m)
    return _clean(bytearray(b"".join(out)), np.concatenate(mut), hash4(marker), keep, rng, chunk[:3])


def marker_chunk(L: int, salt: int, marker=MARKER) -> bytes:
    """The marker and L - 4 bytes of filler none of whose 4-grams shares the marker's bucket."""
    rng = _rng(salt)
    return _clean(bytearray(marker + _fill(rng, L - 4)), np.concatenate([np.zeros(4, bool), np.ones(L - 4, bool)]), hash4(marker), {0}, rng)


def _dist(dct: bytes, chunk: bytes, member_from_nearest: int, n: int, agree, near31) -> int:
    """Distance from the chunk's first byte to member i's marker in members_dict's layout."""
    d = 0
    for i in range(0, member_from_nearest + 1):
        d += len(chunk) if i in agree else (40 if i in near31 else STRIDE)
    return d


def g_candidates() -> dict:
    L = 96
    pairs, expect = [], []

    def add(n, agree=(), near31=(), winner=None, salt=0):
        c = marker_chunk(L, 100 + salt)
        d = members_dict(c, n, agree, near31, salt)
        pairs.append((c, d))
        dist = _dist(d, c, winner, n, agree, near31) if winner is not None else 0
        expect.append((0, n, dist, (L if winner is not None else None), None))
    for i, n in enumerate((0, 1, 63, 64, 65, 200)):          # nobody agrees: no anchor, whatever the bucket holds
        add(n, salt=i)
    for i, n in enumerate((1, 63, 64, 65, 200)):             # the agreeing member is the nearest
        add(n, agree=(0,), winner=0, salt=10 + i)
    add(64, agree=(63,), winner=63, salt=20)                 # the farthest of the 64 (bucket slot l - 64)
    add(65, agree=(63,), winner=63, salt=21)
    add(200, agree=(63,), winner=63, salt=22)
    add(65, agree=(64,), salt=23)                            # just outside them (slot l - 65): no anchor
    add(200, agree=(64, 150), salt=24)
    add(40, agree=(3, 17), winner=3, salt=25)                # two members agree: the nearer
    add(200, agree=(15, 16), winner=15, salt=26)             # (on either side of a group of 16)
    add(200, agree=(16, 63), winner=16, salt=27)
    add(200, agree=(31, 32), winner=31, salt=28)
    add(200, agree=(47, 48, 64), winner=47, salt=29)
    add(5, near31=(0,), salt=30)                             # 31 bytes agree and the 32nd differs: no anchor
    add(70, near31=(0, 5), agree=(9,), winner=9, salt=31)    # ... and a farther member that agrees on all 32 wins
    return job_of(pairs, expect)


def g_buckets() -> dict:
    L = 96
    pairs, expect = [], []
    for salt, marker in ((40, bytes(4)), (41, gram_of_bucket(4095)), (42, gram_of_bucket(1))):
        for n, agree, winner in ((3, (1,), 1), (2, (), None)):
            c = marker_chunk(L, salt, marker)
            d = members_dict(c, n, agree, (), salt, marker)
            pairs.append((c, d))
            expect.append((0, n, _dist(d, c, winner, n, agree, ()) if winner is not None else 0, L if winner is not None else None, None))
    return job_of(pairs, expect)


COUNT_LENGTHS = (1, 3, 4, 63, 64, 65, 67, 127, 128, 129, 130, 131, 256, 257)
COUNT_ANCHORS = (15, 16, 17, 63, 64, 65)
COUNT_DICTS = (3, 1024, 2048)


def g_counts() -> dict:
    """Chunks that repeat their dictionary's first bytes (one-byte edits 50 .. 300 bytes apart), so nearly every anchor exists: the chunk
    length decides how many there are and whether the last one has four bytes left.  No single anchor is promised."""
    specs = [("neardup", L, 300, 200 + i) for i, L in enumerate(COUNT_LENGTHS)]
    specs += [("neardup", 64 * n - 9, 64 * n + 40, 230 + i) for i, n in enumerate(COUNT_ANCHORS)]
    specs += [("neardup", 64 * n - 9 + 64 * (n % 2), D, 240 + i) for i, (n, D) in enumerate((n, D) for n in (3, 16) for D in COUNT_DICTS)]
    j = H.make_job(specs)
    j["expect"] = [None] * len(j["ids"])
    return j


def g_worst() -> dict:
    """Dictionary and chunk are copies of one 64-byte period: every anchor's bucket holds 64 members or more and all of them agree.  One job
    per LDS class, the window exactly on the class's cap."""
    period = _fill(_rng(300), 64)
    pairs, expect = [], []
    for cap in CAPS:
        Dl = 4096
        L = cap - Dl
        pairs.append(((period * (L // 64 + 1))[:L], period * (Dl // 64)))
        expect.append((1, Dl // 64, 128, min(512, L - 64), 64))         # block 1: the nearest DICTIONARY member lies two periods back
    return job_of(pairs, expect)


def g_distance() -> dict:
    """Class B (window above 32768): the only agreeing member at distance 32768 (an anchor) and at 32769 (one byte too far: none); the same
    record and chunk behind a dictionary cut to a window of 32768 (class SG3, which has no distance test) are the control."""
    L = 200
    pairs, expect = [], []
    for k, far in enumerate((0, 1)):
        rng = _rng(400 + k)
        body = _fill(rng, 100)
        chunk = _fill(rng, 64) + MARKER + body + _fill(rng, L - 64 - 104)
        at = 64 - far                                                     # the member's place in a dictionary of 32768 bytes
        dct = _fill(rng, at) + MARKER + body + _fill(rng, 32768 - at - 104)
        assert len(chunk) == L and len(dct) == 32768
        pairs.append((chunk, dct)); expect.append((1, None, 0 if far else 32768, None, None))
        cut = dct[:32768 - L]
        pairs.append((chunk, cut)); expect.append((1, None, 32768 - L + far, None, None))
    return job_of(pairs, expect)


def g_padding() -> dict:
    """An anchor 8 bytes in front of the window's end whose dictionary candidate is followed by zero bytes: all 32 bytes agree through the
    window's zero padding, and the run is what the window has left."""
    rng = _rng(500)
    tail = MARKER + _fill(rng, 4)
    chunk = _fill(rng, 128) + tail
    dct = _fill(rng, 50) + tail + bytes(40) + _fill(rng, 30)
    d = len(chunk) - 8 + len(dct) - 50
    return job_of([(chunk, dct)], [(2, None, d, 8, None)])


RUN_EDITS = (511, 512, 600, 39, 40, 41)
BACK_EXTENTS = (0, 7, 8, 127, 128, 150)


def g_runs() -> dict:
    """A chunk that copies its dictionary but for ONE byte.  Forward: the byte lies `e` bytes behind anchor 0 (run e, 512 at most).  Backward:
    it lies in front of anchor 3 (block 3 starts at 192), `back` equal bytes between them.  Then the two ends of the backward stretch: the
    chunk's first position (anchor 1 of an unedited copy: 64) and the window's first byte (a diagonal that meets the dictionary 20 bytes
    behind its start: 16, whole 8-byte pieces only)."""
    pairs, expect = [], []
    for i, e in enumerate(RUN_EDITS):
        src = _fill(_rng(600 + i), 800)
        c = bytearray(src[:700]); c[e] ^= 0x02
        pairs.append((bytes(c), src)); expect.append((0, None, 800, min(e, 512), 0))
    for i, b in enumerate(BACK_EXTENTS):
        src = _fill(_rng(620 + i), 500)
        c = bytearray(src[:400]); c[191 - b] ^= 0x02
        pairs.append((bytes(c), src)); expect.append((3, None, 500, 208, min(b, 128)))
    src = _fill(_rng(640), 500)
    pairs.append((src[:400], src)); expect.append((1, None, 500, 336, 64))
    src = _fill(_rng(641), 500)
    pairs.append((_fill(_rng(642), 44) + src[:300], src)); expect.append((1, None, 544, 280, 16))
    return job_of(pairs, expect)


def groups() -> dict:
    return {"candidates": g_candidates(), "buckets": g_buckets(), "counts": g_counts(), "worst": g_worst(), "distance": g_distance(),
            "padding": g_padding(), "runs": g_runs()}


# ---- the witness --------------------------------------------------------------------------------------------------------------------
def witness_one(chunk: np.ndarray, dct: np.ndarray) -> dict:
    """block a -> (dictionary members of the anchor's bucket, distance, forward run, backward extent) with distance 0 = no anchor; blocks whose
    anchor position has no four bytes left are absent.  Members by a plain count over the window's hashes, distance and run by
    pyref.lz_anchors, the backward extent from its definition (equal bytes in front of the anchor along the diagonal, compared in pieces of
    8 that lie inside the window, at most 128, never in front of the chunk)."""
    dct = dct[-32768:]
    w = bytes(dct) + bytes(chunk)
    t, dl = len(w), len(dct)
    if t < 4:
        return {}
    wp = np.frombuffer(w + bytes(4), np.uint8)
    nh = t - 3
    v = wp[:nh].astype(np.uint64) | (wp[1:nh + 1].astype(np.uint64) << 8) | (wp[2:nh + 2].astype(np.uint64) << 16) | (wp[3:nh + 3].astype(np.uint64) << 24)
    h = (((v * np.uint64(MUL)) & np.uint64(M32)) >> np.uint64(20)).astype(np.int64)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    cut = np.flatnonzero(np.diff(hs)) + 1
    buckets = {int(hs[s]): [int(q) for q in order[s:e]] for s, e in zip(np.concatenate([[0], cut]), np.concatenate([cut, [nh]]))}
    anchors = pyref.lz_anchors(w, dl, buckets)
    out = {}
    for a in range((len(chunk) + 63) // 64):
        pa = dl + 64 * a
        if pa + 4 > t:
            continue
        members = sum(1 for q in buckets[int(h[pa])] if q < dl)
        d, run = anchors.get(a, (0, 0))
        back = 0
        if d:
            for j in range(16):
                if pa - d < 8 * j + 8:
                    break
                n = 0
                while n < 8 and w[pa - 8 * j - 1 - n] == w[pa - d - 8 * j - 1 - n]:
                    n += 1
                back += n
                if n < 8:
                    break
            back = min(back, 64 * a)
        out[a] = (members, d, run, back)
    return out


def witness(job: dict) -> list:
    return [witness_one(job["parts"][int(i)], job["parts"][int(b)]) for i, b in zip(job["ids"], job["base"])]
