"""GPU: dictionary DEFLATE jobs whose walks meet a candidate the NEXT blocks' anchors already know (hmse_amd/csrc/l1_deflate.hip, phase 4b's
backward extents and `known_of`).  The matcher then takes that candidate's common length from the anchor instead of comparing bytes, so
every case here is a near-duplicate (chunk, base) pair with edits placed where the known stretch begins, ends or competes with another
candidate — and every comparison is bit for bit against the CPU oracle (streams, offsets, kind), never against another device run.
ops.l1_deflate raises on a non-zero status word (the trip-budget bit 4 included), so a passing case also had status 0.

Chunks are seeded low-entropy text (300 words): hash buckets are shared, positions without a hint are really walked.
"""
from dataclasses import asdict

import numpy as np
import pytest

from conftest import words_text

pytestmark = pytest.mark.gpu

BLOCK = 10            # the 64-byte block (of the chunk) most cases edit
OFFSETS = (0, 1, 15, 16, 17, 47, 48, 62, 63)   # block start, hint threshold (16 bytes of a run left), anchor compare (32 + 16), block end
KINDS = ("sub", "ins1", "ins5", "del3")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def text():
    """One text for every case (read-only): 48 KiB of words."""
    t = words_text(48 * 1024, seed=4242)
    t.setflags(write=False)
    return t


def edit(chunk, pos, kind):
    """One edit at byte `pos`; bytes that no word holds, so the edit never recreates text."""
    c = chunk.tolist()
    if kind == "sub":
        c[pos] = 0x23
    elif kind == "ins1":
        c[pos:pos] = [0x25]
    elif kind == "ins5":
        c[pos:pos] = [0x25, 0x26, 0x25, 0x26, 0x2A]
    elif kind == "del3":
        del c[pos:pos + 3]
    else:
        raise ValueError(kind)
    return np.array(c, dtype=np.uint8)


def edits(chunk, lst):
    """Several edits, positions in the coordinates of the unedited chunk."""
    for pos, kind in sorted(lst, reverse=True):
        chunk = edit(chunk, pos, kind)
    return chunk


@pytest.fixture(scope="module")
def study():
    """The CPU model of the dictionary walk (tools/study/lz_study.c, study_dict_known): which candidates of a pair the next anchors know."""
    import ctypes as C
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import lz_study
    lz_study.build()
    lib = C.CDLL(lz_study.SO)
    lib.study_dict_known.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]

    def known(base, chunk):
        """(candidates whose length anchor a0+1 knows, ... anchor a0+2 only, known lengths that differ from the compared ones)"""
        b, c, o = np.ascontiguousarray(base), np.ascontiguousarray(chunk), np.zeros(16, np.uint64)
        lib.study_dict_known(c.ctypes.data, c.size, b.ctypes.data, b.size, 32, o.ctypes.data)
        return int(o[4]), int(o[6]), int(o[12])
    return known


def assert_reached(study, pairs, tag, none=(), next_but_one=()):
    """On the CPU: every pair must REACH the known-length path (a walked position meets, with 16 bytes agreed, the candidate the next
    anchors speak about) — all but the pairs `none`, built to have no such candidate; the pairs `next_but_one` through anchor a0+2 —
    and the known length must be the compared one.  Without this every case would also pass with the path dead."""
    for j, (b, c) in enumerate(pairs):
        k1, k2, bad = study(b, c)
        assert bad == 0, (tag, j, "a known length differs from the compared one", bad)
        assert (k1 + k2 == 0) if j in none else (k1 + k2 > 0), (tag, j, k1, k2)
        assert j not in next_but_one or k2 > 0, (tag, j, k1, k2)


def check_pairs(orc, dev, study, pairs, tag, none=(), next_but_one=()):
    """pairs = [(base, chunk)]: one call over base0, chunk0, base1, chunk1, ... with chunk i's dictionary = base i."""
    import torch
    from hmse_amd import IngestConfig, ops
    assert_reached(study, pairs, tag, none, next_but_one)
    cfg = IngestConfig()
    parts, base = [], []
    for b, c in pairs:
        base += [-1, len(parts)]
        parts += [b, c]
    data = np.concatenate(parts)
    cuts = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    base = np.array(base, dtype=np.int64)
    w_out, w_off, w_kind = orc.deflate_chunks(data, cuts, orc.default_cfg(**asdict(cfg)), None, base)
    out, off, kind = ops.l1_deflate(torch.from_numpy(data).to(dev), torch.from_numpy(cuts.astype(np.int64)).to(dev), cfg, None,
                                    torch.from_numpy(base).to(dev))
    out, off, kind = out.cpu().numpy(), off.cpu().numpy().astype(np.uint64), kind.cpu().numpy()
    assert np.array_equal(kind, w_kind), (tag, np.flatnonzero(kind != w_kind)[:4].tolist())
    assert np.array_equal(off, w_off), (tag, np.flatnonzero(off != w_off)[:4].tolist())
    for j in range(len(parts)):
        a, e = int(w_off[j]), int(w_off[j + 1])
        assert np.array_equal(out[a:e], w_out[a:e]), (tag, "record", j, "of", len(parts))
    assert out.size == int(w_off[-1])
    assert (w_kind[1::2] == 2).any(), (tag, "no DELTA record: the case runs no dictionary job to the end")
    return w_kind


@pytest.mark.parametrize("kind", KINDS)
def test_one_edit_at_every_block_offset(kind, text, orc, dev, study):
    """One edit per pair at offsets 0, 1, 15, 16, 17, 47, 48, 62, 63 of block 10: the positions from the edit to the block's end have no
    hint, the next anchor's backward stretch ends at the edit (a known mismatch), and 512 + 258 identical bytes follow: a run of 512
    with no mismatch seen, known length = 258."""
    base = text[:2048]
    pairs = [(base, edit(base, 64 * BLOCK + o, kind)) for o in OFFSETS]
    # (a substitution or a one-byte insertion in the block's last byte leaves no walked position in front of the next anchor; a deletion at the
    # block's first byte puts the following text on the anchor itself)
    check_pairs(orc, dev, study, pairs, kind, none={"sub": (8,), "ins1": (8,), "del3": (0,)}.get(kind, ()))


def test_several_edits_close_together(text, orc, dev, study):
    base = text[2048:2048 + 1500 + 37]          # (the last block is shorter than 64)
    L = base.size
    p = 64 * BLOCK
    pairs = [
        (base, edits(base, [(p + 5, "sub"), (p + 40, "sub")])),                     # two in one block
        (base, edits(base, [(p + 5, "ins1"), (p + 40, "del3")])),                   # ... with two changes of the diagonal
        (base, edits(base, [(p + 30, "sub"), (p + 64 + 30, "sub")])),               # consecutive blocks: anchor 11 fails (edit in its first 32 bytes)
        (base, edits(base, [(p + 30, "ins5"), (p + 64 + 20, "ins1")])),
        (base, edits(base, [(p + 50, "sub"), (p + 64 + 40, "sub"), (p + 128 + 35, "sub")])),   # short runs: known lengths of 40..104
        (base, edits(base, [(10, "sub"), (L - 20, "sub")])),                        # first block, and the last, shorter one
        (base, edits(base, [(3, "ins1"), ((L & ~63) + 5, "del3")])),
    ]
    check_pairs(orc, dev, study, pairs, "several")


def hot_base(text, n_blocks, hot_blocks, seed):
    """A base whose blocks `hot_blocks` begin with a 4-gram that more than 64 LATER places of the base share (each continued differently):
    the anchors of those blocks see the 64 nearest dictionary members only, never the one on the chunk's diagonal, and fail although the
    diagonal is clean — so the positions around them get their facts from an anchor one or two blocks further on."""
    rng = np.random.default_rng(seed)
    b = text[:64 * n_blocks].copy()
    for k in hot_blocks:
        b[64 * k: 64 * k + 4] = np.frombuffer(b"QZXJ", np.uint8)
    tail = b"".join(b"QZXJ" + bytes(rng.integers(65, 91, 6, dtype=np.uint8)) + b" " for _ in range(72))
    return np.concatenate([b, np.frombuffer(tail, np.uint8)])


def test_ends_of_the_backward_stretch(text, orc, dev, study):
    plain = text[4096:4096 + 1800]
    pairs = [
        # reaches the chunk's first position AND the dictionary's first byte: an identical chunk whose anchor 0 fails (hot 4-gram)
        (hot_base(text, 16, [0], 1), hot_base(text, 16, [0], 1)),
        # reaches the dictionary's first byte only: three bytes in front of the chunk (anchor 0 fails, chunk position 3 <-> dictionary byte 0)
        (plain, edit(plain, 0, "ins5")[2:]),
        # the chunk's first position, the dictionary going on in front of it: the chunk is the base without its first 29 bytes, first block edited
        (plain, edit(plain[29:], 2, "sub")),
        # ends at a known mismatch: any edit
        (plain, edit(plain, 64 * BLOCK + 20, "sub")),
        # ends at the compare's limit of 128 bytes, no mismatch seen: anchors 10 and 11 fail, the edit lies in block 9
        (hot_base(text, 24, [10, 11], 2), edit(hot_base(text, 24, [10, 11], 2), 64 * 9 + 20, "sub")),
        # only the next-but-one anchor serves: anchor 10 fails, the edit lies in block 9
        (hot_base(text, 24, [10], 3), edit(hot_base(text, 24, [10], 3), 64 * 9 + 20, "sub")),
        (hot_base(text, 24, [10], 3), edit(hot_base(text, 24, [10], 3), 64 * 9 + 20, "ins1")),
    ]
    check_pairs(orc, dev, study, pairs, "ends", next_but_one=(4, 5))


def test_run_lengths(text, orc, dev, study):
    big = text[8192:8192 + 3000]
    p = 64 * BLOCK
    pairs = [
        (big, edit(big, 64 * 3 + 20, "sub")),                    # > 512 + 258 identical bytes behind the edit: known length == maxlen == 258
        (big, edit(big, big.size - 150, "sub")),                  # tail: the run ends at the window's end, maxlen < 258
        (big, edit(big, big.size - 150, "del3")),
        (big[:1500], edit(big[:1500], 1500 - 70, "ins1")),
    ]
    # known lengths of 15, 16 and 17 (the EXTEND threshold is 16): only an anchor whose 32-byte compare runs into the zero padding behind
    # the window can have a run below 32, so the chunk ends 14 bytes behind anchor 10 and the base goes on with zeros there; the three
    # positions in front of the anchor then know 15, 16 and 17 bytes (= their maxlen), the edit 10 bytes in front of it leaves them unhinted
    x, y = big[:p], big[p:p + 14]
    zbase = np.concatenate([x, y, np.zeros(24, np.uint8), big[p + 14:p + 400]])
    for back in (10, 4):
        pairs.append((zbase, np.concatenate([edit(x, p - back, "sub"), y])))
    check_pairs(orc, dev, study, pairs, "runs", none=(3,))


def test_lure_candidate_on_another_diagonal(text, orc, dev, study):
    """A candidate inside the chunk, nearer than the known one and agreeing on 16 or more bytes, comes first in the walk: it must be
    compared as always, and win or lose by its length alone."""
    base = text[12288:12288 + 2048]
    p = 64 * BLOCK
    pairs = []
    for lure_len, second in ((16, None), (24, None), (60, None), (60, p + 64 + 40), (40, p + 64 + 50)):
        c = edit(base, p + 20, "sub")
        if second is not None:
            c = edit(c, second, "sub")            # the known length ends here: shorter than the lure where the lure spans it
        lure = c[p + 21: p + 21 + lure_len].copy()
        c[p - 200: p - 200 + lure_len] = lure      # chunk only: the nearest candidate of the positions behind the edit
        pairs.append((base, c))
        b2 = base.copy(); b2[p - 200: p - 200 + lure_len] = lure   # and once in the dictionary too (same diagonal as the known one's neighbours)
        pairs.append((b2, c))
    check_pairs(orc, dev, study, pairs, "lure")


def class_windows():
    from hmse_amd import ops
    return list(zip(("S", "S2", "SG", "SG2", "SG3", "B"), tuple(ops.DEFLATE_CLASS_CAPS) + (65536,)))


@pytest.mark.parametrize("name,cap", class_windows(), ids=[c[0] for c in class_windows()])
def test_every_dictionary_size_class(name, cap, text, orc, dev, study):
    """The same edits in a window just inside each class's cap (class B: a dictionary of the full 32 KiB): both EXTEND variants (32 and
    64 bytes per trip) sit behind the one test; the backward extents have one home, the mark area in LDS, in every class."""
    T = cap - 5
    Dl = min(32768, T // 2 + 8)
    L = T - Dl
    base = src = text[:Dl]                                 # (class B: the dictionary at its limit of 32 KiB, which is also a chunk's)
    p = 64 * BLOCK
    lst = [(p + 20, "sub"), (64 * 20 + 47, "ins1"), (64 * 30 + 1, "del3"), (64 * 40 + 30, "sub"), (64 * 41 + 30, "sub"),
           (L - 700, "ins5"), (L - 100, "sub")]
    c = edits(src, lst)[:L]
    assert c.size == L and Dl + L == T
    check_pairs(orc, dev, study, [(base, c)], name)
