"""GPU: substitute / redact (hmse_amd.find substitute, redact, substitute_regex, redact_regex; hmse_subst_apply) against the plain-Python
reference of tests/subst_ref.py — the kernel on synthetic chunk maps (a corpus of three tiles + 37 bytes under five chunkings, edit lists
built to reach every path: strips in one gap, strips assembled from pieces, edits at strip and tile edges, thousands of edits under one
strip, replacements that span tiles), refused input with out poisoned, poisoned / misaligned / guarded memory (tests/arena.py), and
stores with POINTER and DELTA records, ingested again.  Every result is compared byte for byte.  The shapes are the smallest at which
the kernel can go wrong."""
import os
import re

import numpy as np
import pytest

import arena as A_
import lines_ref
import regex_ref
import subst_ref as ref
from test_sync_host import SEG, corpora

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc", "subst.hip")).read()
_K = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, _SRC).group(1))
STRIP = _K("SUBST_STRIP")
T = _K("SUBST_NT") * STRIP * _K("SUBST_TRIPS")            # output bytes of a workgroup
N = 3 * T + 37
BLOCK = 20                                               # one record placed at three corpus positions
POISON = 0xA5


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    import torch
    a = np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)


def _tables(dev, corpus, cuts, place=None):
    place = place or (lambda x, **kw: _t(x, dev))
    raw, raw_off, slot = lines_ref.tables(corpus, cuts)
    i64 = lambda v: np.asarray(v, np.int64).reshape(-1)
    return place(np.frombuffer(raw, np.uint8).copy(), side="raw"), place(i64(raw_off)), place(i64(cuts)), place(i64(slot))


def _corpus():
    rng = np.random.default_rng(1)
    c = rng.integers(97, 123, N, dtype=np.uint8)
    for at in (70, 150):
        c[at: at + BLOCK] = c[5: 5 + BLOCK]
    return c.tobytes()


def _chunkings():
    rng = np.random.default_rng(2)
    tiny = [0]
    while tiny[-1] < N:
        tiny.append(min(tiny[-1] + int(rng.integers(0, 3)), N))
    edges = sorted({0, N, *(k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)), *(k * STRIP + d for k in (1, 5) for d in (-1, 0, 1))})
    return {"one chunk": [0, N], "a byte per chunk": list(range(N + 1)), "0, 1 and 2 bytes": tiny + [N, N, N], "tile and strip edges": edges,
            "one record at three places": [0, 5, 5 + BLOCK, 70, 70 + BLOCK, 150, 150 + BLOCK, 2 * T + 3, N]}


def _edit_lists(cuts):
    """-> [(name, edits, reps)]: (start, end, sel) lists in order, with the replacements they select"""
    A, B, C3, E = b"Q", b"RS", b"XYZ", b""
    out = [("none", [], [A]),
           ("an insertion at 0 and one at N", [(0, 0, 0), (N, N, 1)], [C3, B]),
           ("the whole corpus deleted", [(0, N, 0)], [E]),
           ("the whole corpus replaced by one byte", [(0, N, 0)], [A]),
           ("touching edits", [(100, 110, 0), (110, 120, 1), (120, 120, 2), (120, 130, 0), (130, 131, 3)], [A, B, C3, E]),
           ("three insertions at one position", [(T + 3, T + 3, 0), (T + 3, T + 3, 1), (T + 3, T + 3, 2)], [A, B, C3]),
           ("2 T one-byte deletions in a row", [(50 + i, 51 + i, 0) for i in range(2 * T)], [E]),
           ("2 T one-byte deletions in a row, then an insertion", [(50 + i, 51 + i, 0) for i in range(2 * T)] + [(50 + 2 * T, 50 + 2 * T, 1)], [E, C3]),
           ("every other byte deleted", [(i, i + 1, 0) for i in range(0, N, 2)], [E]),
           ("every third byte doubled", [(i, i, 0) for i in range(0, N, 3)], [A]),
           ("a replacement of 2 T + 5 bytes", [(77, 80, 0)], [bytes(65 + i % 26 for i in range(2 * T + 5))])]
    for edge in (3 * STRIP, T, 2 * T):
        for d in (-1, 0, 1):
            out.append((f"a corpus end and an output end at {edge}{d:+d}", [(edge + d - 3, edge + d, 0)], [C3]))
            out.append((f"an output end at {edge}{d:+d}", [(10, 12, 0)], [bytes(48 + i % 10 for i in range(edge + d - 10))]))
            out.append((f"a corpus end at {edge}{d:+d}, the output 7 on", [(2, 2, 1), (edge + d - 2, edge + d, 0)], [E, b"1234567"]))
    if len(cuts) - 1 >= 8:                                 # edits that start in one chunk and end three chunks later
        ks = [k for k in (1, (len(cuts) - 1) // 2, len(cuts) - 6) if cuts[k + 3] < N]
        eds = []
        for k in ks:
            s, e = cuts[k], min(cuts[k + 3] + 1, N)
            if not eds or s >= eds[-1][1]:
                eds.append((s, e, len(eds) % 2))
        out.append(("edits across three chunk boundaries", eds, [B, E]))
    return out


def _random_list(rng):
    kind = int(rng.integers(0, 4))                          # 0: sparse, 1: dense, 2: clustered at a tile edge, 3: long replacements
    reps = [bytes(rng.integers(65, 91, int(rng.choice([0, 1, 2, 7, 16, 33]))).astype(np.uint8)) for _ in range(int(rng.integers(1, 5)))]
    if kind == 3:
        reps.append(bytes(rng.integers(65, 91, int(rng.integers(T - 40, T + 40))).astype(np.uint8)))
    at = int(rng.integers(0, 40)) if kind != 2 else int(rng.integers(1, 3)) * T - int(rng.integers(0, 60))
    eds = []
    for _ in range(int(rng.integers(1, 8)) if kind in (0, 3) else int(rng.integers(20, 400))):
        s = at + int(rng.choice([0, 0, 1, 5, 17, 300])) if kind else at + int(rng.integers(0, N // 3))
        if s > N:
            break
        e = min(N, s + int(rng.choice([0, 1, 1, 2, 9, 40]) if kind else rng.integers(0, 3000)))
        eds.append((s, e, int(rng.integers(0, len(reps)))))
        at = e
    return eds, reps


def _apply(dev, tabs, edits, reps, fill, place=None):
    from hmse_amd import ops
    place = place or (lambda x, **kw: _t(x, dev))
    if fill:
        reps = [bytes([42 + j]) for j in range(len(reps))]
    i64 = lambda v: place(np.asarray(v, np.int64).reshape(-1))
    rep_off = [0]
    for r in reps:
        rep_off.append(rep_off[-1] + len(r))
    out_off = ref.out_offsets(int(tabs[2][-1]) if tabs[3].numel() else 0, edits, reps, fill)
    got = ops.subst_apply(*tabs, i64([e[0] for e in edits]), i64([e[1] for e in edits]), i64([e[2] for e in edits]),
                          place(np.frombuffer(b"".join(reps), np.uint8).copy(), side="rep"), i64(rep_off), i64(out_off), out_off[-1], fill)
    return got.cpu().numpy().tobytes(), reps, out_off


# ---- 1. identity and constructed edits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(_chunkings()))
def test_constructed_and_random_edit_lists_under_five_chunkings(dev, name):
    corpus, cuts = _corpus(), _chunkings()[name]
    tabs = _tables(dev, corpus, cuts)
    assert int(tabs[2][-1]) == N == len(corpus)
    if name == "one record at three places":
        assert tabs[3].tolist()[1] == tabs[3].tolist()[3] == tabs[3].tolist()[5]
    rng = np.random.default_rng(17 + list(_chunkings()).index(name))     # other random lists under every chunking: 300 in all
    lists = _edit_lists(cuts) + [("random %d" % i, *_random_list(rng)) for i in range(60)]
    assert name in ("one chunk",) or any(nm.startswith("edits across") for nm, _, _ in lists)
    for fill in (False, True):
        for nm, edits, reps in lists:
            got, used, out_off = _apply(dev, tabs, edits, reps, fill)
            want, want_off = ref.splice(corpus, edits, used, fill)
            assert out_off == want_off and len(got) == len(want), (nm, fill)
            if got != want:
                bad = next(i for i in range(len(want)) if got[i] != want[i])
                raise AssertionError(f"{nm} (fill {fill}): output byte {bad} of {len(want)} is {got[bad]}, the splice has {want[bad]}")
            if fill:
                assert len(got) == N
    got, _, _ = _apply(dev, tabs, [], [b"x"], False)
    assert got == corpus                                   # no edits: the corpus itself


def test_insertions_into_an_empty_corpus_on_a_store_of_zero_chunks(dev):
    import torch
    z = lambda n, dt=torch.int64: torch.zeros(n, dtype=dt, device=dev)
    tabs = (z(0, torch.uint8), z(1), z(1), z(0))
    edits, reps = [(0, 0, 1), (0, 0, 0), (0, 0, 1)], [b"abc", bytes(range(1, 40))]
    got, _, out_off = _apply(dev, tabs, edits, reps, False)
    assert got == reps[1] + reps[0] + reps[1] == ref.splice(b"", edits, reps)[0] and out_off == [0, 39, 42, 81]
    assert _apply(dev, tabs, edits, reps, True)[0] == b"" == _apply(dev, tabs, [], reps, False)[0]


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------------------
def _raw_apply(dev, raw, raw_off, cuts, slot, edits, reps, out_off, fill=False, out_cap=None, rep_off=None, rep_bytes=None):
    """hmse_subst_apply through ctypes on an out and a status word that start poisoned -> (return code, status, out with 64 bytes behind out_cap)"""
    import torch
    from hmse_amd import _lib
    i64 = lambda v: _t(np.asarray(v, np.int64).reshape(-1), dev)
    rep = b"".join(reps)
    if rep_off is None:
        rep_off = [0]
        for r in reps:
            rep_off.append(rep_off[-1] + len(r))
    out_cap = out_off[-1] if out_cap is None else out_cap
    raw_d, ro, cu, sl, ro2, oo = _t(raw, dev), i64(raw_off), i64(cuts), i64(slot), i64(rep_off), i64(out_off)
    s, e, r = (i64([ed[j] for ed in edits]) for j in range(3))
    rep_d = _t(rep + b"#", dev)
    out = torch.full((out_cap + 64,), POISON, dtype=torch.uint8, device=dev)
    st = torch.full((1,), -1, dtype=torch.int32, device=dev)
    rc = _lib.hip_lib().hmse_subst_apply(raw_d.data_ptr(), raw_d.numel(), ro.data_ptr(), len(raw_off) - 1, cu.data_ptr(), sl.data_ptr() if len(slot) else None,
                                         len(slot), s.data_ptr() if edits else None, e.data_ptr() if edits else None, r.data_ptr() if edits else None, len(edits),
                                         rep_d.data_ptr(), len(rep) if rep_bytes is None else rep_bytes, ro2.data_ptr(), len(rep_off) - 1, 1 if fill else 0,
                                         oo.data_ptr(), out.data_ptr(), out_cap, st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, int(st[0].item()) & 0xFFFFFFFF, out.cpu().numpy().tobytes()


def test_refused_calls_set_their_status_bit_and_write_not_one_byte(dev):
    from hmse_amd import ops
    rng = np.random.default_rng(6)
    n = T + 300
    corpus = rng.integers(97, 123, n, dtype=np.uint8).tobytes()
    cuts = [0, 100, 100, 250, T + 1, n]
    raw, raw_off, slot = lines_ref.tables(corpus, cuts)
    edits, reps = [(5, 9, 0), (9, 9, 1), (240, 260, 2), (T - 2, T + 40, 1), (n - 1, n, 0)], [b"", b"<redacted>", b"Z"]
    want, off = ref.splice(corpus, edits, reps)
    untouched = lambda got, cap: got[2] == bytes([POISON]) * (cap + 64)
    rc, st, out = _raw_apply(dev, raw, raw_off, cuts, slot, edits, reps, off)
    assert (rc, st) == (0, 0) and out == want + bytes([POISON]) * 64
    one = [b"*", b"#", b"@"]
    rc, st, out = _raw_apply(dev, raw, raw_off, cuts, slot, edits, one, ref.out_offsets(n, edits, one, True), fill=True)
    assert (rc, st) == (0, 0) and out == ref.splice(corpus, edits, one, True)[0] + bytes([POISON]) * 64

    def moved(i, by):
        o = list(off)
        o[i] += by
        return o
    swap = lambda i, ed: edits[:i] + [ed] + edits[i + 1:]
    cases = {"overlap": dict(edits=swap(2, (8, 260, 2))), "an edit that descends": dict(edits=swap(2, (260, 240, 2))),
             "end > N": dict(edits=swap(4, (n - 1, n + 1, 0))), "end = 2^62": dict(edits=swap(4, (n - 1, 1 << 62, 0))),
             "start = 2^64 - 1": dict(edits=swap(0, (-1, -1, 0))), "an insertion inside the edit in front": dict(edits=swap(1, (8, 8, 1))),
             "sel = n_rep": dict(edits=swap(3, (T - 2, T + 40, 3))), "sel = -1": dict(edits=swap(3, (T - 2, T + 40, -1))),
             "a rep_off that descends": dict(rep_off=[0, 11, 10, 11]), "a rep_off that does not start at 0": dict(rep_off=[1, 1, 11, 11]),
             "a rep_off that ends past rep_bytes": dict(rep_off=[0, 0, 10, 12]), "rep_bytes one short": dict(rep_bytes=10),
             "out_off wrong at 0": dict(out_off=moved(0, 1)), "out_off wrong in the middle": dict(out_off=moved(2, -1)),
             "out_off wrong at n": dict(out_off=moved(5, 1)), "out_off wrong at n, downwards": dict(out_off=moved(5, -1))}
    for nm, kw in cases.items():
        a = dict(edits=edits, out_off=off, rep_off=None, rep_bytes=None)
        a.update(kw)
        cap = a["out_off"][-1] + 1
        got = _raw_apply(dev, raw, raw_off, cuts, slot, a["edits"], reps, a["out_off"], out_cap=cap, rep_off=a["rep_off"], rep_bytes=a["rep_bytes"])
        assert got[:2] == (0, 2) and untouched(got, cap), nm
    # fill with a 2-byte replacement (one nobody selects), and with an empty one
    for bad in ([b"*", b"#", b"@@"], [b"*", b"", b"@"]):
        got = _raw_apply(dev, raw, raw_off, cuts, slot, [(5, 9, 0)], bad, [5, n], fill=True)
        assert got[:2] == (0, 2) and untouched(got, n), bad
    for bad_cuts, bad_slot, bad_off in (([0, 100, 90, 250, T + 1, n], slot, raw_off),               # cuts descend
                                        (cuts, [0, 1, len(raw_off) - 1, 3, 4], raw_off),            # a slot outside the index
                                        ([0, 100, 100, 250, T + 1, n + 1], slot, raw_off),          # a chunk longer than its record
                                        ([1, 100, 100, 250, T + 1, n], slot, raw_off),              # the corpus does not start at 0
                                        (cuts, slot, raw_off[:-1] + [raw_off[-1] + 50])):           # records beyond raw
        got = _raw_apply(dev, raw, bad_off, bad_cuts, bad_slot, edits, reps, off)
        assert got[:2] == (0, 2) and untouched(got, off[-1]), (bad_cuts, bad_slot)
        i64 = lambda v: _t(np.asarray(v, np.int64), dev)
        with pytest.raises(ops.HmseError, match="inconsistent tables"):
            ops.subst_apply(_t(raw, dev), i64(bad_off), i64(bad_cuts), i64(bad_slot), i64([]), i64([]), i64([]), _t(b"x", dev), i64([0, 1]), i64([n]), n)
    # out_cap one short: bit 0 alone, and still nothing is written; the wrapper says which
    got = _raw_apply(dev, raw, raw_off, cuts, slot, edits, reps, off, out_cap=off[-1] - 1)
    assert got[:2] == (0, 1) and untouched(got, off[-1] - 1)
    got = _raw_apply(dev, raw, raw_off, cuts, slot, [], reps, [n], out_cap=n - 1)
    assert got[:2] == (0, 1) and untouched(got, n - 1)
    got = _raw_apply(dev, raw, raw_off, cuts, slot, [], reps, [n - 1], out_cap=n)                  # no edits: out_off[0] is N, nothing else
    assert got[:2] == (0, 2) and untouched(got, n)
    tabs = _tables(dev, corpus, cuts)
    i64 = lambda v: _t(np.asarray(v, np.int64), dev)
    with pytest.raises(ops.HmseError, match="out_off\\[-1\\] exceeds the output"):
        ops.subst_apply(*tabs, i64([]), i64([]), i64([]), _t(b"x", dev), i64([0, 1]), i64([n]), n - 1)
    with pytest.raises(ops.HmseError, match="edits that overlap"):
        ops.subst_apply(*tabs, i64([5, 4]), i64([6, 7]), i64([0, 0]), _t(b"x", dev), i64([0, 1]), i64([5, 5, n - 2]), n - 2)
    rc, st, out = _raw_apply(dev, raw, raw_off, cuts, slot, edits, reps, off)                      # and the run is still clean
    assert (rc, st) == (0, 0) and out == want + bytes([POISON]) * 64


# ---- 3. arguments only -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["random", "ones", "zero"])
def test_on_poisoned_misaligned_guarded_memory(dev, monkeypatch, pattern):
    """Inputs off their alignment between guard bands (the last record ends at raw's guarded end, the last replacement at rep's), out and
    the status word from poisoned memory at three bytes off: the output is fully determined and no guard band is touched."""
    ar = A_.Arena(dev, pattern, seed=13).install(monkeypatch, distrust_zeros=True, byte_misalign=3)
    put = lambda x, side: ar.place(x, misalign={"raw": 5, "rep": 9}.get(side, 0))
    place = lambda x, side=None: put(x, side) if len(x) else put(np.zeros(1, x.dtype), side)[:0]      # (nothing to place: an empty view of a guarded byte)
    rng = np.random.default_rng(7)
    n = T + 5 * STRIP + 9
    corpus = rng.integers(97, 123, n, dtype=np.uint8).tobytes()
    tiny = [0]
    while tiny[-1] < n:
        tiny.append(min(tiny[-1] + int(rng.integers(0, 3)), n))
    lists = [([], [b"x"]), ([(0, 0, 0), (n, n, 1)], [b"head", b"tail!"]), ([(n - 40, n, 0)], [b""]), ([(3, 5, 0), (T - 1, T + 1, 1), (n - 1, n, 0)], [b"AB", b"C" * 33]),
             ([(i, i + 1, 0) for i in range(7, n - 7, 2)], [b""]), ([(0, n, 0)], [bytes(range(64, 64 + 47))])]
    for cuts in (tiny, sorted({0, n, *rng.integers(1, n, 12).tolist()}), [0, n]):
        tabs = _tables(dev, corpus, cuts, place)
        for edits, reps in lists:
            for fill in (False, True):
                got, used, _ = _apply(dev, tabs, edits, reps, fill, place)
                assert got == ref.splice(corpus, edits, used, fill)[0], (len(cuts), edits[:3], fill)
    ar.check()


@pytest.mark.parametrize("misalign", [1, 9, 15])
def test_outputs_that_end_around_a_tile_edge_on_a_misaligned_out(dev, monkeypatch, misalign):
    """The tiles count from out's address rounded down to 16, so with out `misalign` bytes off an output of T - 1, T or T + 1 bytes (and
    of 2 T - 1) reaches into a tile that an aligned out would not need: its last bytes are written all the same, and nothing behind
    them.  out comes from poisoned, guarded memory at that misalignment; the corpus is shorter, as long and longer than the output."""
    ar = A_.Arena(dev, "random", seed=19).install(monkeypatch, distrust_zeros=True, byte_misalign=misalign)
    place = lambda x, side=None: ar.place(x) if len(x) else ar.place(np.zeros(1, x.dtype))[:0]
    rng = np.random.default_rng(23)
    for total in (T - 1, T, T + 1, 2 * T - 1, 2 * T - misalign, 2 * T - misalign + 1):
        for grow in (0, 7, -5):                              # no edit; an insertion of 7 bytes; 5 bytes deleted
            n = total - grow
            corpus = rng.integers(97, 123, n, dtype=np.uint8).tobytes()
            tabs = _tables(dev, corpus, sorted({0, n, *rng.integers(1, n, 5).tolist()}), place)
            edits, reps = ([], [b"x"]) if grow == 0 else ([(n - 3, n - 3, 0)], [b"1234567"]) if grow > 0 else ([(n - 9, n - 4, 0)], [b""])
            got, used, out_off = _apply(dev, tabs, edits, reps, False, place)
            want = ref.splice(corpus, edits, used)[0]
            assert out_off[-1] == total == len(want) and got == want, (total, grow, next((i for i in range(total) if got[i] != want[i]), None))
    ar.check()


# ---- 4. stores -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stores(dev):
    import torch
    from hmse_amd import IngestConfig, find, ingest, manifest, read
    cfg = IngestConfig(seg_size=SEG)
    out = {}
    for k, d in corpora().items():
        if k == "B2":
            continue
        m = manifest.Manifest.from_bytes(manifest.build_manifest(ingest.ingest_shard(torch.from_numpy(d).to(dev), cfg)).to_bytes())
        corpus = read.read_manifest(m, dev).cpu().numpy().tobytes()
        assert corpus == d.tobytes()
        out[k] = (m, find.StoreFinder(m, dev), corpus)
    return cfg, out


# a capitalised word and up to six lower-case words behind it: long enough to lie across chunk boundaries (a content-defined cut
# rarely falls inside a single word), few enough starts for the reference; '*' and '#' can take no part in it
NAME, NUM, LOWER = rb"[A-Z][a-z]+( [a-z]+){0,6}", rb"[0-9]+", rb"[a-z]+"
_MATCHES = {}


def _matches(key, corpus, pattern, rx):
    """the reference's edits of one regex: regex_ref's occurrences (every start with its longest match), then the leftmost-longest chain"""
    if (key, pattern) not in _MATCHES:
        _MATCHES[key, pattern] = ref.leftmost_longest(regex_ref.find(corpus, pattern, rx.reach))
    return _MATCHES[key, pattern]


def _reingested(dev, cfg, data):
    from hmse_amd import ingest, manifest, read
    m = manifest.Manifest.from_bytes(manifest.build_manifest(ingest.ingest_shard(data, cfg)).to_bytes())
    return m, read.read_store(manifest.Store.from_bytes(manifest.Store([m]).to_bytes()), dev).cpu().numpy().tobytes()


@pytest.mark.parametrize("name", ["A", "B"])
def test_substitute_regex_and_redact_regex_on_stores_ingested_again(dev, stores, name):
    import torch
    from hmse_amd import KIND_DELTA, KIND_POINTER, find
    from hmse_amd.regex import Regex
    cfg, out = stores
    m, fd, corpus = out[name]
    assert (m.chunk_map["kind"] == KIND_DELTA).any() and (m.chunk_map["kind"] == KIND_POINTER).any()
    rxs = [Regex(NAME, device=dev), Regex(NUM, device=dev)]
    kept = [_matches(name, corpus, p, r) for p, r in zip((NAME, NUM), rxs)]
    edits = [(s, s + ln, 0) for s, ln in kept[0]]
    cuts, slot, mult = fd.cuts.cpu().numpy(), fd.slot.cpu().numpy(), fd.mult.cpu().numpy()
    s_, e_ = np.array([x[0] for x in edits]), np.array([x[1] for x in edits])
    k = np.searchsorted(cuts, s_, side="right") - 1
    assert len(edits) >= 100 and (e_ > cuts[k + 1]).any() and ((e_ <= cuts[k + 1]) & (mult[slot[k]] > 1)).any()
    # substitute_regex: longer, shorter and empty replacements
    for repl in (b"<a name>", b"X", b""):
        sub = fd.substitute_regex(rxs[0], repl)
        want, off = ref.splice(corpus, edits, [repl])
        assert sub.data.cpu().numpy().tobytes() == want and sub.out_off.tolist() == off and sub.data.dtype == torch.uint8 and sub.data.is_cuda
        assert (sub.n_edits, sub.n_bytes_in, sub.n_bytes_out) == (len(edits), len(corpus), len(want))
        assert sub.start.tolist() == [x[0] for x in edits] and sub.end.tolist() == [x[1] for x in edits]
    sub = fd.substitute_regex(rxs[0], b"<a name>")
    want = ref.splice(corpus, edits, [b"<a name>"])[0]
    m2, again = _reingested(dev, cfg, sub.data)
    assert again == want
    found = fd.nonoverlapping(fd.find_regex(rxs[0]))
    at = sub.translate(found.offsets).tolist()
    assert all(want[a: a + 8] == b"<a name>" for a in at) and len(at) == len(edits)
    # redact_regex: lengths and offsets stay, and the expression is gone from the store ingested again
    red = fd.redact_regex(rxs[0], b"*")
    want = ref.splice(corpus, edits, [b"*"], True)[0]
    assert red.data.cpu().numpy().tobytes() == want and red.n_bytes_out == red.n_bytes_in == len(corpus) and red.out_off.tolist() == [x[0] for x in edits] + [len(corpus)]
    m3, again = _reingested(dev, cfg, red.data)
    assert again == want
    fd3 = find.StoreFinder(m3, dev)
    assert fd3.count_regex(rxs[0]).tolist() == [0] and fd.count_regex(rxs[0]).tolist()[0] >= len(edits)
    assert torch.equal(red.translate(found.offsets), found.offsets)
    # two regexes, a replacement each; the one-off forms
    both = sorted([(s, s + ln, 0) for s, ln in kept[0]] + [(s, s + ln, 1) for s, ln in kept[1]])
    assert len(kept[1]) > 10
    sub = fd.substitute_regex(rxs, [b"", b"<N>"])
    assert sub.data.cpu().numpy().tobytes() == ref.splice(corpus, both, [b"", b"<N>"])[0] and sub.sel.tolist() == [x[2] for x in both]
    red = fd.redact_regex(rxs, [b"#", b"0"])
    assert red.data.cpu().numpy().tobytes() == ref.splice(corpus, both, [b"#", b"0"], True)[0]
    one = find.substitute_regex(m, rxs[1], b"<N>", dev)
    assert one.data.cpu().numpy().tobytes() == ref.splice(corpus, [(s, s + ln, 0) for s, ln in kept[1]], [b"<N>"])[0]
    one = find.redact_regex(m, rxs[1], dev, b"9")
    assert one.data.cpu().numpy().tobytes() == ref.splice(corpus, [(s, s + ln, 0) for s, ln in kept[1]], [b"9"], True)[0]
    # groups that overlap, a plain Found, lines
    with pytest.raises(ValueError, match="ranges overlap"):
        fd.substitute_regex([rxs[0], Regex(LOWER, device=dev)], [b"a", b"b"])
    with pytest.raises(ValueError, match="has offsets but no lengths"):
        fd.substitute(fd.find([b"the"]), b"THE")
    ln = fd.grep([b"== "])
    lines = sorted(zip(ln.start.tolist(), ln.end.tolist()))
    assert len(lines) > 3 and all(a[1] <= b[0] for a, b in zip(lines, lines[1:]))
    assert fd.substitute(ln, b"").data.cpu().numpy().tobytes() == ref.splice(corpus, [(s, e, 0) for s, e in lines], [b""])[0]


def test_the_two_shard_merged_store_and_the_empty_one(dev, stores):
    import torch
    from hmse_amd import find, ingest, manifest
    from hmse_amd.regex import Regex
    cfg, out = stores
    m, fd1, corpus = out["A"]
    d = np.frombuffer(corpus, np.uint8)
    half = 3 * SEG
    rs = ingest.ingest_shards_local([torch.from_numpy(d[:half].copy()).to(dev), torch.from_numpy(d[half:].copy()).to(dev)], cfg)
    st = manifest.Store.from_bytes(manifest.merge_manifests([manifest.build_manifest(r, i, 2) for i, r in enumerate(rs)]).to_bytes())
    assert len(st.shards) == 2
    fd2 = find.StoreFinder(st, dev)
    rx = Regex(NAME, device=dev)
    a, b = fd1.substitute_regex(rx, b"<a name>"), fd2.substitute_regex(rx, b"<a name>")
    assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("data", "start", "end", "sel", "out_off")) and a.n_edits == b.n_edits >= 100
    assert torch.equal(fd1.redact_regex(rx).data, fd2.redact_regex(rx).data)
    across = (torch.tensor([0, half - 3], dtype=torch.int64, device=dev), torch.tensor([6, half + 3], dtype=torch.int64, device=dev))
    assert fd2.substitute(across, b"[cut]").data.cpu().numpy().tobytes() == ref.splice(corpus, [(0, 6, 0), (half - 3, half + 3, 0)], [b"[cut]"])[0]
    empty = find.StoreFinder(manifest.Store([]), dev)
    for z in (empty.substitute_regex(rx, b"x"), empty.redact_regex([rx, rx], [b"*", b"#"]), empty.substitute(empty.grep([b"a", b"bc"]), [b"1", b"2"])):
        assert (z.n_edits, z.n_bytes_in, z.n_bytes_out) == (0, 0, 0) and z.data.numel() == 0 and z.data.dtype == torch.uint8 and z.data.device.type == "cuda"
        assert z.out_off.tolist() == [0] and all(getattr(z, f).numel() == 0 and getattr(z, f).dtype == torch.int64 for f in ("start", "end", "sel"))
    zero = torch.zeros(2, dtype=torch.int64, device=dev)
    z = empty.substitute((zero, zero), b"only this")                             # two insertions into an empty corpus
    assert z.data.cpu().numpy().tobytes() == b"only thisonly this" and z.out_off.tolist() == [0, 9, 18]
