"""GPU: every stage depends on its declared arguments only — not on what its workspace or its outputs held before the call, not on where
its byte pointers point, not on what lies behind the declared end of a buffer — and writes nothing outside its outputs.

The memory a call sees comes from tests/arena.py (checked on the CPU by tests/test_arena_host.py): inputs are placed between guard bands,
outputs, status words and workspaces of hmse_amd.ops are allocated in the arena and arrive filled with its pattern.  Every comparison is
byte-exact against the references the suite already has (the CPU oracle, hashlib, zlib, the numpy writers, the host restatements under
tests/); each test asserts the reference first and arena.check() second.

Axes (CASES): the patterns zero / ones / random with aligned byte pointers; random with the byte-typed arguments (data, streams, blob,
digests as inputs; out, raw_out, digests, kind, ok as outputs) 1, 2, 3, 4, 8 and 13 bytes off a 256-byte boundary — typed arrays and
workspaces stay aligned; random with even the buffers the wrapper asks to be zero poisoned (distrust: include/hmse.h tells no caller to
clear anything).  Inside a test: the declared size ends inside the placed buffer, once with the guard pattern behind it and once with valid
bytes of the same kind; a second call with another input of another size gets the first call's workspace as it was left.
"""
import os
import random
import sys
import zlib
from dataclasses import asdict

import numpy as np
import pytest

import arena as A
import edge_inputs as E
from conftest import words_text

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

MIB = 1 << 20
# (pattern, misalignment of the byte-typed arguments, distrust the wrapper's zeros)
CASES = [("zero", 0, False), ("ones", 0, False), ("random", 0, False)] + [("random", m, False) for m in (1, 2, 3, 4, 8, 13)] + [("random", 0, True)]
# l4_lsh / l4_lsh_update take no byte-typed argument: the misalignment only moves nothing there, so three of its values are enough
CASES_TYPED = [c for c in CASES if c[1] in (0, 3, 13)]
case_id = lambda c: f"{c[0]}-m{c[1]}" + ("-distrust" if c[2] else "")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    return E.kernel_constants()


def ocfg(orc, cfg):
    return orc.default_cfg(**asdict(cfg))


def make_arena(dev, monkeypatch, case, seed, reuse_ws=False):
    pattern, mis, distrust = case
    return A.Arena(dev, pattern, seed=seed).install(monkeypatch, distrust_zeros=distrust, reuse_ws=reuse_ws, byte_misalign=mis), mis


def fresh_arena(dev, monkeypatch, case, seed):
    """A second arena for the same test, without workspace reuse: the call that follows is the FIRST on its workspace (with reuse_ws only a
    test's first call finds the pattern there, every later one what the first left behind)."""
    return make_arena(dev, monkeypatch, case, seed + 1000)


def u64(t):
    return t.cpu().numpy().astype(np.uint64)


def tails(ar, data, mis, valid_tail):
    """The same bytes twice: with the arena's guard band right behind the declared end, and with `valid_tail` (bytes of the same kind) there."""
    yield "guard", ar.place(data, mis)
    yield "valid", ar.place_with_tail(data, valid_tail, mis)[0]


# ---- L2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def l2_ref(orc):
    from hmse_amd import IngestConfig
    cfg = IngestConfig(seg_size=1 << 19)
    text = words_text(2 * (1 << 19) + 300_001 + 70_000, seed=61)
    n = 2 * (1 << 19) + 300_001                              # three segments, the last one partial and ending on an odd byte
    data, behind = text[:n], text[n:]
    given = np.array([0, 300_001, 700_000, n], dtype=np.uint64)
    small = words_text(150_001, seed=62)
    return dict(cfg=cfg, data=data, behind=behind, given=given, small=small, want=orc.cdc(data, ocfg(orc, cfg)),
                want_given=orc.cdc(data, ocfg(orc, cfg), given), want_small=orc.cdc(small, ocfg(orc, cfg)))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_l2_cdc(case, l2_ref, dev, monkeypatch):
    from hmse_amd import ops
    r = l2_ref
    ar, mis = make_arena(dev, monkeypatch, case, seed=1, reuse_ws=True)
    for tag, d in tails(ar, r["data"], mis, r["behind"]):
        assert d.numel() == r["data"].size and d.numel() % 2 == 1
        assert np.array_equal(u64(ops.l2_cdc(d, r["cfg"])), r["want"]), tag
        assert np.array_equal(u64(ops.l2_cdc(d, r["cfg"], ar.place(r["given"].astype(np.int64)))), r["want_given"]), tag
    # another input of another size on the workspace the calls above left behind
    assert np.array_equal(u64(ops.l2_cdc(ar.place(r["small"], mis), r["cfg"])), r["want_small"])
    assert [k for k, _ in ar.requests].count("ws-reused") >= 4
    ar.check()
    ar, mis = fresh_arena(dev, monkeypatch, case, 1)
    assert np.array_equal(u64(ops.l2_cdc(ar.place(r["small"], mis), r["cfg"])), r["want_small"])
    ar.check()


# ---- L3 SHA-256 ------------------------------------------------------------------------------------------------------------------------
SHA_LENS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 3000, 0, 4097, 5000, 64]


def sha_inputs(last: int, seed: int, many: bool = False):
    lens = ([i % 131 for i in range(4200)] if many else SHA_LENS) + [last]
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = words_text(int(cuts[-1]) + 4096, seed=seed)
    return data[: int(cuts[-1])], data[int(cuts[-1]):], cuts


def sha_want(orc, data, cuts):
    import hashlib
    return np.stack([np.frombuffer(hashlib.sha256(data[int(a): int(b)].tobytes()).digest(), np.uint8) for a, b in zip(cuts[:-1], cuts[1:])])


@pytest.fixture(scope="module")
def sha_ref(orc):
    """Last chunk ending at n with n - start < 64 (the bounded tail branch), with n - start >= 128 (the prefetch's bound), and more than 4096
    chunks (the longest-first hand-out order, built in the workspace)."""
    out = []
    for last, seed, many in ((40, 71, False), (200, 72, False), (33, 73, True)):
        data, behind, cuts = sha_inputs(last, seed, many)
        out.append((data, behind, cuts, sha_want(None, data, cuts)))
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_l3_sha256(case, sha_ref, dev, monkeypatch):
    from hmse_amd import ops
    ar, mis = make_arena(dev, monkeypatch, case, seed=2, reuse_ws=True)
    for data, behind, cuts, want in sha_ref[::-1]:          # the large selection first: the small ones reuse its workspace
        cu = ar.place(cuts.astype(np.int64))
        for tag, d in tails(ar, data, mis, behind):
            got = ops.l3_sha256(d, cu)
            assert got.data_ptr() % 16 == mis
            assert np.array_equal(got.cpu().numpy(), want), (tag, len(cuts), np.flatnonzero((got.cpu().numpy() != want).any(axis=1))[:5])
    ar.check()
    # the small selections (no hand-out order: only the counter is cleared), each the first call on a workspace full of the pattern
    ar, mis = fresh_arena(dev, monkeypatch, case, 2)
    for data, behind, cuts, want in sha_ref[:2]:
        got = ops.l3_sha256(ar.place_with_tail(data, behind, mis)[0], ar.place(cuts.astype(np.int64)))
        assert np.array_equal(got.cpu().numpy(), want), len(cuts)
    assert [k for k, _ in ar.requests].count("ws") == 2
    ar.check()


# ---- L3 dedupe / index ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dedup_ref(orc):
    dg, _ = E.planted_digests(1500)
    dg = np.ascontiguousarray(dg[:5000])
    small = np.ascontiguousarray(dg[1000:2777][::-1])
    fo, rc = orc.dedup(dg)
    assert (fo != np.arange(len(fo))).sum() > 500            # repeats
    return dg, fo, rc, small, orc.dedup(small)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_l3_dedup_and_index_update(case, dedup_ref, dev, monkeypatch):
    import torch
    from hmse_amd import ops
    dg, fo_w, rc_w, small, (fo_s, rc_s) = dedup_ref
    ar, mis = make_arena(dev, monkeypatch, case, seed=3, reuse_ws=True)
    d = ar.place(dg, mis)                                    # digest rows off their alignment
    assert d.shape == (5000, 32) and d.data_ptr() % 16 == mis
    fo, rc = ops.l3_dedup(d)
    assert np.array_equal(u64(fo), fo_w) and np.array_equal(rc.cpu().numpy().astype(np.uint32), rc_w)
    fo, rc = ops.l3_dedup(ar.place(small, mis))              # reused table
    assert np.array_equal(u64(fo), fo_s) and np.array_equal(rc.cpu().numpy().astype(np.uint32), rc_s)
    n = dg.shape[0]
    for splits in ([n], [1700, 1701, n]):                    # old / new
        table = ar.empty(ops.l3_index_slots(n), torch.int32)
        fo, rc = ar.empty(n, torch.int64), ar.empty(n, torch.int32)
        a = 0
        for e in splits:
            ops.l3_index_update(d, a, e - a, fo, rc, table)
            a = e
        assert np.array_equal(u64(fo), fo_w) and np.array_equal(rc.cpu().numpy().astype(np.uint32), rc_w), splits
    ar.check()
    ar, mis = fresh_arena(dev, monkeypatch, case, 3)
    fo, rc = ops.l3_dedup(ar.place(small, mis))
    assert np.array_equal(u64(fo), fo_s) and np.array_equal(rc.cpu().numpy().astype(np.uint32), rc_s)
    ar.check()


# ---- L4 MinHash -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def minhash_ref(orc, K):
    """The pass-boundary chunks of tests/edge_inputs.py in front of chunks shorter than four bytes and text chunks; the last chunk is text and
    ends at n.  Signatures once, from the oracle."""
    from hmse_amd import IngestConfig
    cfg = IngestConfig()
    data, cuts, facts = E.minhash_boundary_chunks(K["MH_SUB"])
    rows = facts["rows"]
    keep = rows["distinct"][:3] + rows["abcd"][2:4] + rows["text"][:4] + rows["sentinel"][:4] + rows["plain"]    # one chunk on each side of the boundary, per content
    text = words_text(40_000, seed=81)
    parts = [data[int(cuts[i]): int(cuts[i + 1])] for i in keep]
    parts += [text[:0], text[:1], text[1:3], text[3:6], text[100:104], text[200:5200], text[6000:6003], text[7000:19001]]
    ln = np.array([p.size for p in parts], np.uint64)
    cu = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
    d = np.concatenate(parts)
    want = orc.minhash_chunks(d, cu, ocfg(orc, cfg))
    assert (want[len(keep)] == 0xFFFFFFFF).all() and not (want[-1] == 0xFFFFFFFF).any()
    ids = np.arange(len(parts), dtype=np.int64)[::-1][::2].copy()
    return dict(cfg=cfg, data=d, cuts=cu, want=want, behind=text[19001: 19001 + 5000], ids=ids)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_l4_minhash(case, minhash_ref, dev, monkeypatch):
    """With misalignment 1, 2, 3 and 13 the base pointer is off a dword: the byte-wise branch of the insert loop (base_aligned == false)
    hashes every chunk; with 0, 4 and 8 the aligned branch does, and the shifted cuts below give it chunk starts on start % 4 = 0 .. 3."""
    from hmse_amd import ops
    r = minhash_ref
    cfg, want = r["cfg"], r["want"]
    ar, mis = make_arena(dev, monkeypatch, case, seed=4, reuse_ws=True)
    cu = ar.place(r["cuts"].astype(np.int64))
    bad = lambda got: np.flatnonzero((got.cpu().numpy().view(np.uint32) != want).any(axis=1)).tolist()
    for tag, d in tails(ar, r["data"], mis, r["behind"]):
        for memo in (True, False):
            assert not bad(ops.l4_minhash(d, cu, cfg, memo=memo)), (tag, memo)
    got = ops.l4_minhash(d, cu, cfg, ar.place(r["ids"])).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want[r["ids"]])
    for s in (1, 2, 3):                                      # every chunk start moves by s: chunk 0 is the s bytes in front, not selected
        ds = ar.place(np.concatenate([np.full(s, 0x2E, np.uint8), r["data"]]), mis)
        cs = ar.place(np.concatenate([[0], r["cuts"].astype(np.int64) + s]))
        ids = ar.place(np.arange(1, len(r["cuts"]), dtype=np.int64))
        assert not bad(ops.l4_minhash(ds, cs, cfg, ids)), s
    ar.check()
    ar, mis = fresh_arena(dev, monkeypatch, case, 4)        # a selection as the first call on its memo table
    got = ops.l4_minhash(ar.place(r["data"], mis), ar.place(r["cuts"].astype(np.int64)), cfg, ar.place(r["ids"])).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want[r["ids"]])
    ar.check()


# ---- L4 LSH ---------------------------------------------------------------------------------------------------------------------------------
BANDINGS = [(4, 32), (8, 16), (16, 8)]


@pytest.fixture(scope="module")
def lsh_ref(orc):
    from hmse_amd import IngestConfig
    out = {}
    for bands, rows in BANDINGS:
        cfg = IngestConfig(bands=bands, rows=rows)
        sig = E.lsh_population(4000, bands, rows, planted=900)
        keys, base = orc.lsh(sig, ocfg(orc, cfg))
        small = np.ascontiguousarray(sig[500:2100])
        assert (base >= 0).sum() > 300
        out[bands] = (cfg, sig, keys, base, small, orc.lsh(small, ocfg(orc, cfg)))
    return out


@pytest.mark.parametrize("bands,rows", BANDINGS)
@pytest.mark.parametrize("case", CASES_TYPED, ids=case_id)
def test_l4_lsh_and_update(case, bands, rows, lsh_ref, dev, monkeypatch):
    """Signatures are a typed (u32) argument: 4-byte alignment is all they need.  The view that starts one element into its buffer is 4 bytes
    off a 16-byte boundary, so the band rows are read by the word-wise branch of murmur3_words instead of the 16-byte one."""
    import torch
    from hmse_amd import ops
    cfg, sig, keys_w, base_w, small, (keys_s, base_s) = lsh_ref[bands]
    ar, _ = make_arena(dev, monkeypatch, case, seed=5, reuse_ws=True)
    n = sig.shape[0]
    aligned = ar.place(sig.view(np.int32))
    flat = ar.place(np.concatenate([np.array([0x5A5A5A5A], np.uint32), sig.reshape(-1)]).view(np.int32))
    shifted = flat[1:].view(n, 128)
    rows3 = ar.place(np.concatenate([sig[:3], sig]).view(np.int32))[3:]      # a view that starts at a row offset
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous() and rows3.is_contiguous()
    for tag, s in (("aligned", aligned), ("one element in", shifted), ("three rows in", rows3)):
        keys, base = ops.l4_lsh(s, cfg)
        assert np.array_equal(keys.cpu().numpy().view(np.uint32), keys_w), tag
        assert np.array_equal(base.cpu().numpy(), base_w), tag
    keys, base = ops.l4_lsh(ar.place(small.view(np.int32)), cfg)             # reused tables
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), keys_s) and np.array_equal(base.cpu().numpy(), base_s)
    slots = ops.l4_lsh_slots(n)
    for s in (aligned, shifted):
        tables = ar.empty((bands, slots), torch.int32)
        keys, base = ar.empty((n, bands), torch.int32), ar.empty(n, torch.int64)
        a = 0
        for e in (1300, 1301, n):
            ops.l4_lsh_update(s, a, e - a, cfg, keys, base, tables)
            a = e
        assert np.array_equal(keys.cpu().numpy().view(np.uint32), keys_w) and np.array_equal(base.cpu().numpy(), base_w)
    ar.check()
    ar, _ = fresh_arena(dev, monkeypatch, case, 5)
    keys, base = ops.l4_lsh(ar.place(small.view(np.int32)), cfg)
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), keys_s) and np.array_equal(base.cpu().numpy(), base_s)
    ar.check()


# ---- L1 DEFLATE ------------------------------------------------------------------------------------------------------------------------------
def run_jobs(ar, mis, job, cfg, want, ws_limit=None, valid_tail=False):
    """test_gpu_edges.run_jobs with the inputs placed by the arena and the oracle's records computed once per module.  The last chunk ends
    at n; behind it lies the guard band or, with valid_tail, the text the data begins with."""
    from hmse_amd import ops
    w_out, w_off, w_kind = want
    rows = job["ids"].astype(np.int64)
    has_base = bool((job["base"] >= 0).any())
    data = ar.place_with_tail(job["data"], job["data"][:5000], mis)[0] if valid_tail else ar.place(job["data"], mis)
    assert data.numel() == int(job["cuts"][-1])
    out, off, kind = ops.l1_deflate(data, ar.place(job["cuts"].astype(np.int64)), cfg, ar.place(rows),
                                    ar.place(job["base"]) if has_base else None, base_is_chunk_id=True, ws_limit=ws_limit)
    assert out.data_ptr() % 16 == mis
    out, off, kind = out.cpu().numpy(), off.cpu().numpy().astype(np.int64), kind.cpu().numpy()
    parts = job["parts"]
    assert off[0] == 0
    for j, r in enumerate(rows):
        w = w_out[int(w_off[r]): int(w_off[r + 1])]
        got = out[off[j]: off[j + 1]]
        info = (j, parts[r].size, int(job["base"][j]))
        assert kind[j] == w_kind[r], info
        assert got.size == w.size and np.array_equal(got, w), info
        if j % 16 == 0 or len(rows) < 64:                    # stock zlib reads the record
            zd = parts[int(job["base"][j])].tobytes() if kind[j] == 2 else None
            d = zlib.decompressobj(-15, zdict=zd) if zd else zlib.decompressobj(-15)
            assert d.decompress(got.tobytes()) == parts[r].tobytes(), info


def oracle_records(orc, job, cfg):
    odata, ocuts, obase, _ = E.oracle_view(job)
    return orc.deflate_chunks(odata, ocuts, ocfg(orc, cfg), None, obase)


@pytest.fixture(scope="module")
def deflate_ref(orc):
    """Per class cap and job kind, the first jobs of the class on a fresh workspace: windows on the cap and one byte either side, text and
    near-duplicate content.  And one selection with more jobs of classes S and SG than the match kernels have workgroups (512): the first
    512 find the arena's pattern in their scratch, the others what an earlier job left there."""
    from hmse_amd import IngestConfig, ops
    cfg = IngestConfig()
    caps = tuple(ops.DEFLATE_CLASS_CAPS) + (65536,)
    jobs = {}
    for dict_jobs in (False, True):
        for c in caps:
            if c == 65536 and not dict_jobs:
                continue                                     # no plain job has a window above 32768 bytes: class B takes dictionary jobs only
            job = E.deflate_boundary_jobs(caps, dict_jobs, only_cap=c, contents=("text", "neardup"))
            assert len(job["ids"]) >= 4 and {E.window_class(int(t), caps) for t in job["T"]} >= {c}
            jobs[(c, dict_jobs)] = (job, oracle_records(orc, job, cfg))
    assert len(jobs) == 11
    text = words_text(560 * 4096 + 530 * 15000 + 64, seed=91)
    lens = [4096] * 560 + [15000] * 530
    parts, o = [], 0
    for ln in lens:
        parts.append(text[o: o + ln]); o += ln
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    many = {"data": text[:o], "cuts": cuts, "ids": np.arange(len(lens), dtype=np.uint64), "base": np.full(len(lens), -1, np.int64), "parts": parts}
    return cfg, jobs, many, oracle_records(orc, many, cfg)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_l1_deflate_first_jobs_of_every_class(case, deflate_ref, dev, monkeypatch):
    cfg, jobs, _, _ = deflate_ref
    ar, mis = make_arena(dev, monkeypatch, case, seed=6)
    for (c, dict_jobs), (job, want) in jobs.items():
        run_jobs(ar, mis, job, cfg, want, valid_tail=dict_jobs)   # every call: a fresh workspace full of the pattern
    ar.check()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_l1_deflate_more_jobs_than_workgroups_pieces_and_reuse(case, deflate_ref, dev, monkeypatch):
    import torch
    from hmse_amd import ops
    cfg, jobs, many, want_many = deflate_ref
    ar, mis = make_arena(dev, monkeypatch, case, seed=7, reuse_ws=True)
    run_jobs(ar, mis, many, cfg, want_many)
    need = int(ops.record_bytes(torch.from_numpy(np.diff(many["cuts"].astype(np.int64)))).sum().item())
    n_req = len(ar.requests)
    run_jobs(ar, mis, many, cfg, want_many, ws_limit=need * 6 // 10)          # two pieces, in the workspace the call above left behind
    kinds = [k for k, _ in ar.requests[n_req:]]
    assert kinds.count("ws-reused") == 1 and kinds.count("ws") == 0 and kinds.count("buf") == 4 + 2      # one workspace for both pieces, an out_off per piece
    job, want = jobs[(17408, True)]                          # and a dictionary selection of another size on the same workspace
    run_jobs(ar, mis, job, cfg, want)
    ar.check()


# ---- L1 INFLATE ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inflate_ref(orc):
    from test_gpu_read import pack, zlib_records
    from test_oracle import mutate
    recs = zlib_records()
    assert len(recs) == 257
    rnd = random.Random(7)
    mutated = [recs[0]]
    for s, n, b in recs[1:]:
        for _ in range(2):
            mutated.append((mutate(s, rnd), n + (rnd.random() < 0.05), b))
    out = {}
    for name, rs in (("clean", recs), ("mutated", mutated)):
        p = pack(rs)
        out[name] = (p, orc.inflate_chunks(*p))
    assert out["clean"][1][2].all() and 30 < out["mutated"][1][2].sum() < len(mutated) - 150
    return out, np.frombuffer(recs[5][0] + recs[200][0], np.uint8)           # (bytes of valid streams, to lie behind streams_bytes)


@pytest.mark.parametrize("mode", [1, 2, 0], ids=["wave-per-stream", "lane-per-stream", "automatic"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_l1_inflate(case, mode, inflate_ref, dev, monkeypatch):
    """streams_bytes ends at the last record's last byte; records addressed densely and through stream_len; the accept / reject decisions
    of the mutated set equal the oracle's."""
    from hmse_amd import ops
    sets, valid = inflate_ref
    ar, mis = make_arena(dev, monkeypatch, case, seed=8, reuse_ws=True)
    ops.l1_inflate_mode(mode)
    try:
        for name in ("mutated", "clean"):
            (streams, off, kind, base, raw_len), (w_raw, w_off, w_ok) = sets[name]
            k, b, rl = ar.place(kind, mis), ar.place(base), ar.place(raw_len)      # (kind: a byte-typed input)
            for tag, s in tails(ar, streams, mis, valid):
                assert s.numel() == off[-1]
                for dense in (True, False):
                    if dense:
                        raw, raw_off, ok = ops.l1_inflate(s, ar.place(off), k, b, rl, check=False)
                    else:
                        raw, raw_off, ok = ops.l1_inflate(s, ar.place(off[:-1].copy()), k, b, rl, stream_len=ar.place(np.diff(off).astype(np.int32)), check=False)
                    assert raw.data_ptr() % 16 == mis
                    raw, ok = raw.cpu().numpy(), ok.cpu().numpy().astype(bool)
                    assert np.array_equal(u64(raw_off), w_off), (name, tag, dense)
                    assert np.array_equal(ok, w_ok), (name, tag, dense, np.flatnonzero(ok != w_ok)[:10])
                    for i in np.flatnonzero(w_ok):
                        a, e = int(w_off[i]), int(w_off[i + 1])
                        assert np.array_equal(raw[a:e], w_raw[a:e]), (name, tag, dense, i)
        ar.check()
        ar, mis = fresh_arena(dev, monkeypatch, case, 8)    # the clean set as the first call on its workspace
        (streams, off, kind, base, raw_len), (w_raw, w_off, w_ok) = sets["clean"]
        raw, raw_off, ok = ops.l1_inflate(ar.place(streams, mis), ar.place(off), ar.place(kind, mis), ar.place(base), ar.place(raw_len))
        assert bool(ok.all()) and np.array_equal(u64(raw_off), w_off) and np.array_equal(raw.cpu().numpy(), w_raw)
    finally:
        ops.l1_inflate_mode(0)
    ar.check()


# ---- a workspace off its alignment --------------------------------------------------------------------------------------------------------
def test_a_misaligned_workspace_is_refused_and_nothing_is_written(sha_ref, minhash_ref, dev, monkeypatch):
    """include/hmse.h: a workspace is 256-byte aligned; HMSE_EINVAL otherwise, before anything is cleared or launched — the outputs still
    hold the arena's pattern.  (Every entry point, without a GPU: tests/test_arena_host.py.)"""
    import torch
    from hmse_amd import ops
    ar = A.Arena(dev, "random", seed=9).install(monkeypatch)
    good_ws = ops._ws
    outs = []
    real_buf = ops._buf

    def buf(*a, **k):
        t = real_buf(*a, **k)
        outs.append((t, t.clone()))
        return t
    monkeypatch.setattr(ops, "_buf", buf)
    data, _, cuts, want = sha_ref[0]
    d, cu = ar.place(data), ar.place(cuts.astype(np.int64))
    mh = minhash_ref
    calls = {"l3_sha256": lambda: ops.l3_sha256(d, cu),
             "l4_minhash": lambda: ops.l4_minhash(ar.place(mh["data"]), ar.place(mh["cuts"].astype(np.int64)), mh["cfg"]),
             "l2_cdc": lambda: ops.l2_cdc(d, mh["cfg"]),
             "l1_deflate": lambda: ops.l1_deflate(d, cu, mh["cfg"]),
             "l3_dedup": lambda: ops.l3_dedup(ar.place(want)),
             "l4_lsh": lambda: ops.l4_lsh(ar.place(np.arange(256, dtype=np.int32).reshape(2, 128)), mh["cfg"])}
    for shift in (16, 128):
        monkeypatch.setattr(ops, "_ws", lambda nbytes, device, s=shift: good_ws(int(nbytes) + 256, device)[s: s + max(int(nbytes), 256)])
        for name, fn in calls.items():
            del outs[:]
            with pytest.raises(ops.HmseError) as ei:
                fn()
            assert ei.value.code == -1, (name, shift, ei.value)
            torch.cuda.synchronize()
            assert outs and all(torch.equal(t, was) for t, was in outs), (name, shift)
    monkeypatch.setattr(ops, "_ws", good_ws)
    assert np.array_equal(ops.l3_sha256(d, cu).cpu().numpy(), want)           # the aligned call goes through
    ar.check()


# ---- stages over a store ----------------------------------------------------------------------------------------------------------------------
def dataset():
    """3 MiB + 54321 bytes: five near-duplicates and an exact copy of a 200 KB piece of wiki-synth (DELTA and POINTER records), the text they
    were cut from, other text."""
    from make_golden import variants_dataset
    from hmse_amd import corpus
    a = corpus.wiki_synth(MIB, seed=42)
    v = variants_dataset(a)
    return np.concatenate([v, a, corpus.wiki_synth(3 * MIB + 54321 - v.size - a.size, seed=7)])


@pytest.fixture(scope="module")
def ingested(orc, dev):
    """One small ingest with the ordinary allocator, and everything the store-level tests compare with."""
    import torch
    import manifest_ref
    from test_gpu_ingest import _to_host, oracle_pipeline
    from hmse_amd import IngestConfig, bandtable, ingest, manifest
    cfg = IngestConfig(seg_size=MIB)
    data = dataset()
    res = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    assert res.stats["pointer"] > 5 and res.stats["delta"] > 10
    m_bytes = manifest_ref.build(_to_host(res)).to_bytes()
    side = bandtable.write_band_tables(res.band_keys.cpu().numpy(), cfg.band_bits, signatures=res.sig.cpu().numpy())
    _, (o,) = oracle_pipeline(orc, data, cfg)
    return dict(cfg=cfg, data=data, res=res, m_bytes=m_bytes, side=side, oracle=o, m=manifest.Manifest.from_bytes(m_bytes))


def place_uploads(ar, mis, monkeypatch):
    """The store-level modules bring host arrays to the device through read.to_device: byte arrays (blobs, digests, kinds) land in the arena
    `mis` bytes off their alignment, typed arrays aligned."""
    import torch
    from hmse_amd import read, scrub
    real = read.to_device

    def to_device(a, dt, device):
        t = real(a, dt, "cpu")
        return ar.place(t, mis if dt == torch.uint8 else 0)
    monkeypatch.setattr(read, "to_device", to_device)
    monkeypatch.setattr(scrub, "_t", to_device)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_manifest_pack_and_read_path(case, ingested, dev, monkeypatch):
    """hmse_manifest_pack into arena buffers (blob, index, chunk map, pointers: byte-typed, misaligned) == the host reference writer;
    hmse_l1_inflate + hmse_read_assemble over the misaligned blob of that manifest return the input."""
    import torch
    from hmse_amd import manifest, ops, read
    g = ingested
    res, data = g["res"], g["data"]
    ar, mis = make_arena(dev, monkeypatch, case, seed=10)      # (no reuse: every call of every stage finds the pattern)
    # pack_manifest_device with its four outputs allocated here
    m = g["m"]
    n, u = len(m.chunk_map), len(m.index)
    rec_len = (res.stream_off[1:] - res.stream_off[:-1]) + 8 * (res.kind == 2).to(torch.int64)
    is_ptr = res.first_occ != torch.arange(n, dtype=torch.int64, device=dev)
    ptr_index = ar.place(torch.cumsum(is_ptr.to(torch.int64), 0) - is_ptr.to(torch.int64))
    rec_off = ar.place(torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(rec_len, 0)]))
    assert m.lba_unit == 1 and int(rec_off[-1].item()) == m.blob.size
    blob, index = ar.empty(m.blob.size, torch.uint8, misalign=mis), ar.empty((u, 40), torch.uint8, misalign=mis)
    cmap, ptrs = ar.empty((n, 8), torch.uint8, misalign=mis), ar.empty((len(m.pointers), 8), torch.uint8, misalign=mis)
    ops.manifest_pack(res, 0, 1, None, rec_off, 1, ptr_index, blob, index, cmap, ptrs)
    assert blob.cpu().numpy().tobytes() == m.blob.tobytes()
    assert index.cpu().numpy().tobytes() == m.index.tobytes() and cmap.cpu().numpy().tobytes() == m.chunk_map.tobytes()
    assert ptrs.cpu().numpy().tobytes() == m.pointers.tobytes()
    assert manifest.build_manifest(res).to_bytes() == g["m_bytes"]             # and through the module (status word and workspace from the arena)
    # the read path
    place_uploads(ar, mis, monkeypatch)
    back = read.read_manifest(m, dev, verify=True)
    assert back.cpu().numpy().tobytes() == data.tobytes()
    part = read.read_ranges(m, [(MIB - 5, 70001), (0, 1)], dev)
    assert part[0].cpu().numpy().tobytes() == data[MIB - 5: MIB - 5 + 70001].tobytes() and part[1].cpu().numpy().tobytes() == data[:1].tobytes()
    ar.check()


@pytest.fixture(scope="module")
def gc_want(ingested, dev):
    """What a fresh ingest of the store's remainder writes, per drop (test_gpu_gc's contract)."""
    from test_gpu_gc import _fixed, _remainder, _store
    g = ingested
    so = _fixed(g["data"].size, MIB)
    out = {}
    for drop in ((0,), (1, 3)):
        r, r_so = _remainder(g["data"], so, list(drop))
        m, side = _store(r, g["cfg"], dev, seg_off=r_so)
        out[drop] = (m.to_bytes(), side, r)
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gc_plan_and_record_gather(case, ingested, gc_want, dev, monkeypatch):
    from hmse_amd import gc, read
    g = ingested
    ar, mis = make_arena(dev, monkeypatch, case, seed=11)      # (no reuse: every call of every stage finds the pattern)
    place_uploads(ar, mis, monkeypatch)
    for drop, (want, want_side, r) in gc_want.items():
        for side in (g["side"], None):                       # with the sidecar records are gathered; without it everything is decoded
            out, out_side, st = gc.drop_segments(g["m"], list(drop), g["cfg"], dev, band_tables=side)
            assert out.to_bytes() == want and out_side == want_side, (drop, side is None)
            assert st["records_reused"] > 0
    assert read.read_manifest(out, dev).cpu().numpy().tobytes() == r.tobytes()
    ar.check()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_band_tables_index_build_and_query(case, ingested, dev, monkeypatch):
    import similarity_ref as ref
    from hmse_amd import bandtable, ops, similarity
    g = ingested
    res, cfg = g["res"], g["cfg"]
    ar, mis = make_arena(dev, monkeypatch, case, seed=12)      # (no reuse: every call of every stage finds the pattern)
    keys_h, sig_h = res.band_keys.cpu().numpy(), res.sig.cpu().numpy()
    keys, sig = ar.place(keys_h), ar.place(sig_h)
    out = ops.band_tables_write(keys, sig, cfg.band_bits)
    assert out.data_ptr() % 16 == mis
    assert out.cpu().numpy().tobytes() == g["side"]
    assert ops.band_tables_write(keys, None, 12).cpu().numpy().tobytes() == bandtable.write_band_tables(keys_h, 12)
    sk, si = ops.l4_index_build(keys)
    ku = keys_h.view(np.uint32)
    for b in range(cfg.bands):
        o = np.argsort(ku[:, b], kind="stable")
        assert np.array_equal(si[b].cpu().numpy(), o) and np.array_equal(sk[b].cpu().numpy().view(np.uint32), ku[o, b]), b
    S = sig_h.view(np.uint32)
    for bands in (4, 16):
        ix = similarity.SimilarityIndex(sig, cfg, bands=bands)
        for top_k, min_score in ((8, 0), (3, 100)):
            h = ix.near_duplicates(top_k=top_k, min_score=min_score)
            w_ids, w_sc, w_nh, w_nc = ref.search(S, S, bands, top_k, min_score, self_join=True)
            assert np.array_equal(h.n_candidates.cpu().numpy(), w_nc) and np.array_equal(h.n_hits.cpu().numpy(), w_nh), (bands, top_k)
            assert np.array_equal(h.ids.cpu().numpy(), w_ids) and np.array_equal(h.scores.cpu().numpy(), w_sc), (bands, top_k)
            assert (w_nh > 0).sum() > 20
    ar.check()


@pytest.fixture(scope="module")
def scrub_stores(ingested):
    """The store, clean and damaged — a flipped payload byte in a FULL record, in a dictionary and in a DELTA record, and a flipped length in
    a DELTA record's header — with the host reference's report for both."""
    import dataclasses
    import scrub_ref
    from hmse_amd import manifest
    from hmse_amd.config import KIND_DELTA, KIND_FULL
    m = ingested["m"]
    cm = m.chunk_map
    lba = m.index["lba"].astype(np.int64) * m.lba_unit
    base = ingested["oracle"]["base"]
    full = np.unique(cm["slot"][cm["kind"] == KIND_FULL])
    delta = np.unique(cm["slot"][cm["kind"] == KIND_DELTA])
    dicts = np.unique(base[base >= 0])
    assert len(delta) > 10 and len(dicts) > 2
    blob = m.blob.copy()
    blob[lba[int(full[len(full) // 2])] + 20] ^= 0x10        # a FULL record nobody depends on (or somebody: the reference decides)
    blob[lba[int(dicts[1])] + 20] ^= 0x10                    # a dictionary: its dependants are damaged with it
    blob[lba[int(delta[-1])] + 8 + 20] ^= 0x10               # a DELTA record's stream
    blob[lba[int(delta[2])] + 6] ^= 0x01                     # a DELTA record's header: delta_length
    clean, bad = manifest.Store([m]), manifest.Store([dataclasses.replace(m, blob=blob)])
    refs = {"clean": (clean, scrub_ref.scrub_ref(clean)), "damaged": (bad, scrub_ref.scrub_ref(bad))}
    assert len(refs["damaged"][1]["roots"]) >= 3 and len(refs["damaged"][1]["ranges"]) >= 2 and not refs["clean"][1]["roots"]
    return refs


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_scrub_records_and_attribute(case, ingested, scrub_stores, dev, monkeypatch):
    import scrub_ref
    from hmse_amd import scrub
    ar, mis = make_arena(dev, monkeypatch, case, seed=13)      # (no reuse: every call of every stage finds the pattern)
    place_uploads(ar, mis, monkeypatch)
    for name in ("damaged", "clean"):
        store, ref = scrub_stores[name]
        rep = scrub.scrub(store, dev, cfg=ingested["cfg"], band_tables=[ingested["side"]])
        assert scrub_ref.same(rep, ref) == [], (name, scrub_ref.same(rep, ref))
        assert rep.clean == (name == "clean")
    ar.check()


# ---- the captured chain ------------------------------------------------------------------------------------------------------------------------
CHAIN_ARRAYS = ("_cuts", "_digests", "_first_occ", "_refcount", "_uniq", "_sig", "_band_keys", "_base", "_kind", "_stream_off", "_l3_table",
                "_lsh_tables", "_streams")


def poisoned_stream(ar, mis, cfg, capacity, dev, **kw):
    """StreamIngest(graph=True) with its resident data, index, state and output arrays replaced by arena buffers full of the pattern before
    the first batch (the stream's workspace comes from ops._ws, so it is poisoned before hmse_stream_workspace_init).  Two words keep the
    value the module gave them: cuts[0] and stream_off[0], the starts of the first chunk and the first record, are inputs of the chain."""
    import torch
    from hmse_amd import stream
    s = stream.StreamIngest(cfg, capacity, dev, graph=True, **kw)
    for name in CHAIN_ARRAYS:
        t = getattr(s, name)
        setattr(s, name, ar.empty(tuple(t.shape), t.dtype, name=name, misalign=mis if t.dtype == torch.uint8 else 0))
    s._cuts[:1] = 0
    s._stream_off[:1] = 0
    s.data = ar.empty(s.data.numel(), torch.uint8, name="data", misalign=mis)
    s._state = ar.empty(16, torch.int64, name="state")       # (written whole by the module before the first chain call)
    return s


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_captured_chain(case, ingested, orc, dev, monkeypatch):
    """Three batches of one segment and a partial last one through the captured chain == the one-shot ingest == the oracle pipeline."""
    import torch
    from hmse_amd import read
    g = ingested
    data, cfg, whole, o = g["data"], g["cfg"], g["res"], g["oracle"]
    ar, mis = make_arena(dev, monkeypatch, case, seed=14)
    s = poisoned_stream(ar, mis, cfg, data.size, dev)
    for a in range(0, data.size, MIB):
        s.push(torch.from_numpy(data[a: a + MIB].copy()))
    res = s.finish()
    torch.cuda.synchronize()
    assert {k: bool(s._graphs.captured(k)) for k in s._graphs.sizes()} == {MIB: True, data.size % MIB: False}
    for name in ("cuts", "digests", "first_occ", "refcount", "uniq_ids", "sig", "band_keys", "base", "kind", "stream_off", "streams"):
        assert torch.equal(getattr(res, name), getattr(whole, name)), name
    for name, got, want in (("cuts", u64(res.cuts), o["cuts"]), ("digests", res.digests.cpu().numpy(), o["dg"]), ("first_occ", u64(res.first_occ), o["fo"]),
                            ("uniq", u64(res.uniq_ids), o["uniq"]), ("sig", res.sig.cpu().numpy().view(np.uint32), o["sig"]),
                            ("base", res.base.cpu().numpy(), o["base"]), ("kind", res.kind.cpu().numpy(), o["kind"]),
                            ("off", u64(res.stream_off), o["off"]), ("streams", res.streams.cpu().numpy(), o["out"])):
        assert got.shape == want.shape and np.array_equal(got, want), name
    assert torch.equal(read.reconstruct_shard(res, verify=True).cpu(), torch.from_numpy(data))
    ar.check()


@pytest.fixture(scope="module")
def windowed_want(ingested, orc):
    from test_gpu_stream import _oracle_windowed
    g = ingested
    starts = list(range(0, g["data"].size, 2 * MIB))
    return starts, _oracle_windowed(orc, g["data"], g["cfg"], starts)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_captured_chain_with_a_window(case, ingested, windowed_want, dev, monkeypatch):
    import torch
    g = ingested
    data, cfg = g["data"], g["cfg"]
    starts, o = windowed_want
    ar, mis = make_arena(dev, monkeypatch, case, seed=15)
    s = poisoned_stream(ar, mis, cfg, data.size, dev, window_bytes=2 * MIB)
    assert s.data.numel() == 2 * MIB
    for a in range(0, data.size, MIB):
        s.push(torch.from_numpy(data[a: a + MIB].copy()))
    res = s.finish()
    torch.cuda.synchronize()
    assert s.window_starts == starts
    for name, got, want in (("cuts", u64(res.cuts), o["cuts"]), ("digests", res.digests.cpu().numpy(), o["dg"]), ("first_occ", u64(res.first_occ), o["fo"]),
                            ("uniq", u64(res.uniq_ids), o["uniq"]), ("sig", res.sig.cpu().numpy().view(np.uint32), o["sig"]),
                            ("base", res.base.cpu().numpy(), o["base"]), ("kind", res.kind.cpu().numpy(), o["kind"]),
                            ("off", u64(res.stream_off), o["off"]), ("streams", res.streams.cpu().numpy(), o["out"])):
        assert got.shape == want.shape and np.array_equal(got, want), name
    ar.check()
