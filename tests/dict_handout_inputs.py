"""Inputs of tests/test_dict_handout_host.py, tests/test_gpu_dict_handout.py and tests/dict_handout_check.py: DICTIONARY DEFLATE jobs of the
LDS classes, whose hand-out list is built by one pass over the chunk positions from the ranks the ordered sort left behind (DESIGN.md
§11.35).  Jobs have the form test_gpu_edges.run_jobs takes (`base` = the dictionary's chunk id).

Every job carries the promise its content makes about the list, in job["promise"]; `witness` — rule 2b / 2c of the oracle written again from
the definition alone, in numpy — counts a job's unhinted hashed chunk positions, and tests/test_dict_handout_host.py holds the two against
each other on the CPU:

  "all"    every position that CAN be hinted is: a chunk equal to its dictionary.  The last 15 positions of a window have fewer than 16
           bytes left, so no run hints them; 12 of them are hashed (4 bytes fit behind them).  Those 12 are the whole list.
  "none"   nothing is hinted, the list has L - 3 candidates for entries (the worst case for the list's size): a dictionary that shares
           no 32 bytes with the chunk
  "mixed"  5 % .. 60 % unhinted: a near-duplicate with one-byte edits 50 .. 300 bytes apart (the 16 bytes in front of an edit and the rest
           of its 64-byte block lose their hint)
  None     no promise: one repeated byte against a dictionary of the same byte hints the anchors alone (the nearest member lies one
           byte in front of the anchor, so the diagonal leaves the dictionary at once) — with the unrelated dictionary it fills one
           bucket and all four classes; lengths too short for a percentage
"""
from __future__ import annotations

import numpy as np

from conftest import words_text

CAPS = (10048, 13952, 17408, 22976, 32768)     # windows of the five LDS classes (ops.DEFLATE_CLASS_CAPS; the host test checks that)
LENGTHS = (1, 3, 4, 7,                         # no hashed position; one; four
           1023, 1024, 1025, 2049)             # on and around one step of the position pass (1024 positions), and two
DICT_LENGTHS = (3, 2048, 2500)                 # Dl = 3; a multiple of the sort's step (the store and the position pass map threads alike); not one
DEPTH_LENGTHS = (1025, 9000)

_TEXT = words_text(140_000, seed=23)


def _rng(salt: int):
    return np.random.Generator(np.random.PCG64(7000 + salt))


def neardup(L: int, D: int, salt: int):
    """The dictionary's own bytes with one-byte edits 50 .. 300 bytes apart.  (Past the dictionary's length the chunk goes on with
    the text: nothing there lies on a diagonal into the dictionary.  Of a dictionary above 32768 bytes, which counts its last 32768
    only, the chunk repeats the end.)"""
    o = 500 + 41 * salt
    src = _TEXT[o: o + max(L, D)]
    c = (src[D - L: D] if D > 32768 else src[:L]).copy()
    rng = _rng(salt)
    e = int(rng.integers(50, 301))
    while e < L:
        c[e] ^= 0x01 + int(rng.integers(0, 7))
        e += int(rng.integers(50, 301))
    return c, src[:D].copy()


def content(kind: str, L: int, D: int, salt: int):
    """-> (chunk[L], dictionary[D], promise)"""
    o = 500 + 41 * salt
    if kind == "equal":
        assert L == D
        c = _TEXT[o: o + L].copy()
        return c, c.copy(), "all" if L >= 48 else None
    if kind == "text_random":
        return _TEXT[o: o + L].copy(), _rng(salt).integers(0, 256, D, dtype=np.uint8), "none"
    if kind == "neardup":
        c, d = neardup(L, D, salt)
        return c, d, "mixed" if (D >= L >= 1023) else None
    if kind == "byte_unrelated":
        return np.full(L, 0x61, np.uint8), _TEXT[o + 60000: o + 60000 + D].copy(), "none"
    if kind == "byte_same":
        return np.full(L, 0x61, np.uint8), np.full(D, 0x61, np.uint8), None
    if kind in ("period5", "period7"):
        p = int(kind[-1])
        t = np.tile(np.frombuffer(b"qwertyu"[:p], np.uint8), (max(L, D) + 16) // p + 2)
        return t[:L].copy(), t[3: 3 + D].copy(), None
    raise ValueError(kind)


CONTENTS = ("equal", "text_random", "neardup", "byte_unrelated", "byte_same", "period5", "period7")


def make_job(specs) -> dict:
    """specs: (kind, L, D, salt) per job -> dict(data, cuts, ids, base, T, parts, promise)."""
    parts, ids, base, Ts, promise = [], [], [], [], []
    for kind, L, D, salt in specs:
        c, d, pr = content(kind, L, D, salt)
        assert c.size == L and d.size == D and L >= 1 and D >= 1
        parts.append(d); base.append(len(parts) - 1)
        parts.append(c); ids.append(len(parts) - 1)
        Ts.append(L + min(D, 32768)); promise.append(pr)
    lens = np.array([p.size for p in parts], dtype=np.uint64)
    return {"data": np.concatenate(parts), "cuts": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), "ids": np.array(ids, np.uint64),
            "base": np.array(base, np.int64), "T": np.array(Ts), "parts": parts, "promise": promise}


def groups() -> dict:
    """name -> job dict; windows of at most 64 KiB, a few dozen jobs per group."""
    g = {}
    # every content at a length of two steps and a bit, in class S and (the same chunk behind a longer dictionary) in class SG2
    g["contents"] = make_job([(k, 2049, 2049 if k == "equal" else D, i) for i, k in enumerate(CONTENTS) for D in (2500, 18000) if not (k == "equal" and D == 18000)])
    # L on and around the steps of the position pass x Dl: the near-duplicate where the dictionary covers the chunk, text against an unrelated
    # dictionary as well
    g["lengths"] = make_job([(k, L, D, 20 + i) for i, L in enumerate(LENGTHS) for D in DICT_LENGTHS for k in ("neardup", "text_random")])
    # T on each of the five caps and one byte either side (T = 32769: class B, the unchanged control), the dictionary about half the window
    g["caps"] = make_job([("neardup", T // 2, T - T // 2, 40 + i) for i, T in enumerate(t for c in CAPS for t in (c - 1, c, c + 1))])
    # the longest dictionary that stays in SG3 (T = 32768: a dictionary of MORE than 32768 bytes counts 32768 and puts any chunk into class B),
    # one byte more (class B), and a dictionary above 32768 bytes that is clamped (class B): the controls
    g["long_dictionary"] = make_job([("neardup", 3000, 32768 - 3000, 60), ("neardup", 3000, 32768 - 3000 + 1, 61), ("neardup", 3000, 40000, 62),
                                     ("text_random", 3000, 32768 - 3000, 63), ("byte_same", 3000, 32768 - 3000, 64)])
    return g


def depth_job() -> dict:
    return make_job([("neardup", L, L + 700, 80 + i) for i, L in enumerate(DEPTH_LENGTHS)])


# ---- the witness --------------------------------------------------------------------------------------------------------------------
def _first_mismatch(a: np.ndarray, b: np.ndarray) -> int:
    ne = np.flatnonzero(a != b)
    return int(ne[0]) if ne.size else int(a.size)


def witness_one(chunk: np.ndarray, dct: np.ndarray) -> int:
    """Unhinted hashed chunk positions of one dictionary job, from the definition: an anchor every 64 chunk positions; the up-to-64 nearest
    dictionary members of its 12-bit bucket; at least 32 bytes of agreement, longest then nearest; a run of up to 512 along that diagonal;
    a position is hinted iff at least 16 bytes of this block's or the previous block's run are left at it (and the diagonal meets the
    dictionary there)."""
    dct = dct[-32768:]
    w = np.concatenate([dct, chunk]).astype(np.uint8)
    t, dl, L = int(w.size), int(dct.size), int(chunk.size)
    if L < 4:
        return 0
    nh = t - 3
    wp = np.concatenate([w, np.zeros(64, np.uint8)])
    v = wp[:nh].astype(np.uint64) | (wp[1:nh + 1].astype(np.uint64) << 8) | (wp[2:nh + 2].astype(np.uint64) << 16) | (wp[3:nh + 3].astype(np.uint64) << 24)
    h = ((v * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(20)
    nd = min(dl, nh)
    order = np.argsort(h[:nd], kind="stable")
    hs = h[:nd][order]
    known = np.zeros(L, np.int64)                    # best known length per chunk position
    for a in range((L + 63) // 64):
        pa = dl + 64 * a
        if pa + 4 > t:
            continue
        lo, hi = np.searchsorted(hs, h[pa], "left"), np.searchsorted(hs, h[pa], "right")
        near = order[lo:hi][-64:]
        near = near[pa - near <= 32768]
        if near.size == 0:
            continue
        n = np.array([min(32, _first_mismatch(wp[q: q + 32], wp[pa: pa + 32])) for q in near])
        if n.max() < 32:
            continue
        q = int(near[n == n.max()].max())
        d = pa - q
        lim = min(512, t - pa)
        run = _first_mismatch(w[pa: pa + lim], w[pa - d: pa - d + lim])
        p = np.arange(pa, min(pa + 128, t))          # this block and the next
        cap = np.minimum(258, t - p)
        m = cap if run >= 512 else np.clip(pa + run - p, 0, cap)
        m = np.where((d <= p) & (p - d < dl), m, 0)
        known[p - dl] = np.maximum(known[p - dl], m)
    return int((known[: L - 3] < 16).sum())


def witness(job: dict) -> list:
    """Unhinted hashed chunk positions per job."""
    return [witness_one(job["parts"][int(i)], job["parts"][int(b)]) for i, b in zip(job["ids"], job["base"])]
