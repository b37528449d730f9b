"""GPU: the kernels' fallback paths, capacity limits and class boundaries (inputs: tests/edge_inputs.py, each proved to reach its branch
by tests/test_edge_inputs_host.py).  Every comparison is byte-exact against the CPU oracle, or against zlib / numpy where the oracle is
not the definition — never against another run of the device code.

  l2_resolve_kernel's walk from global memory   segments above RS_MAX_CAND candidates or RS_MAX_TILES tiles      oracle cuts
  l2 candidate list overflow                    runs of a byte pair whose every second position is a candidate     oracle cuts
  DEFLATE size classes / encode lists           windows on every cap and one byte either side; 12288 / 32768       oracle records, zlib
  MinHash passes                                shingle counts on MH_SUB and 2 MH_SUB; sentinel chunks             oracle signatures
  L3 / L4 open addressing                       equal home slots, the last slot, equal 32-bit keys                 oracle dedupe / LSH
  band tables, index sort                       n around a tile / 2^16, buckets around one and two pieces          numpy writer / argsort
"""
import ctypes as C
import zlib
from dataclasses import asdict

import numpy as np
import pytest

import edge_inputs as E
from conftest import words_text

pytestmark = pytest.mark.gpu


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


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def l2_cfgs():
    from hmse_amd import IngestConfig
    return [("default", IngestConfig()), ("reference", IngestConfig.reference_preset()), ("norm0", IngestConfig(norm_level=0)),
            ("norm3", IngestConfig(norm_level=3))]


def pair_for(orc, cfg):
    pairs = E.dense_pairs(orc.gear_table(), orc.cdc_masks(ocfg(orc, cfg))[1])
    assert pairs
    return pairs[0]


def check_cuts(orc, dev, data, cfg, seg_off=None, tag=""):
    from hmse_amd import ops
    want = orc.cdc(data, ocfg(orc, cfg), seg_off)
    so = None if seg_off is None else to_dev(np.asarray(seg_off).astype(np.int64), dev)
    got = ops.l2_cdc(to_dev(data, dev), cfg, so).cpu().numpy().astype(np.uint64)
    m = min(len(got), len(want))
    assert got.shape == want.shape and np.array_equal(got, want), (tag, got.shape, want.shape, np.flatnonzero(got[:m] != want[:m])[:3].tolist())
    return want


# ---- L2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg", l2_cfgs(), ids=[c[0] for c in l2_cfgs()])
def test_l2_global_walk_by_candidate_count(name, cfg, orc, dev, K):
    """One segment with more candidates than the resolve kernel stages in LDS (RS_MAX_CAND) and fewer than the provisioned list holds:
    the pair alone, and text with dense stretches at the very start, in the middle and at the very end of the segment."""
    pair = pair_for(orc, cfg)
    data, _ = E.l2_dense_segment(pair)
    want = check_cuts(orc, dev, data, cfg, tag="dense")
    assert np.diff(want.astype(np.int64))[:-1].max() <= cfg.avg_size + 2          # every second byte passes the easy mask: no chunk grows past AVG (+1)
    data, _ = E.l2_mixed_segment(pair, words_text(8 * K["L2_TILE"], seed=3), K["L2_TILE"])
    check_cuts(orc, dev, data, cfg, tag="mixed")
    # the same bytes with a dense stretch in a segment of its own and a segment boundary inside one
    so = np.array([0, K["L2_TILE"] + 5, 2 * K["L2_TILE"], data.size - 5000, data.size], dtype=np.uint64)
    check_cuts(orc, dev, data, cfg, so, tag="mixed, custom segments")


def test_l2_global_walk_by_tile_count(orc, dev, K):
    """Segments above RS_MAX_TILES tiles: 40 MiB of text as one segment, and cut at 33 MiB + 1 (the first segment walks from global
    memory, the second starts off a tile boundary)."""
    from hmse_amd import IngestConfig, corpus
    n = 40 << 20
    data = corpus.wiki_synth(n, seed=42)
    for cfg in (IngestConfig(seg_size=64 << 20), IngestConfig.reference_preset().with_(seg_size=64 << 20)):
        want = check_cuts(orc, dev, data, cfg, tag="one segment")
        assert len(want) > 4000
        check_cuts(orc, dev, data, cfg, np.array([0, (33 << 20) + 1, n], dtype=np.uint64), tag="33 MiB + 1")
        check_cuts(orc, dev, data, cfg, np.array([0, 12345, 12345 + (1 << 20), (34 << 20) + 12345, n], dtype=np.uint64), tag="unaligned")


def test_l2_exactly_max_tiles_and_one_more(orc, dev, K):
    """Few candidates (under RS_MAX_CAND in the whole input), so the tile count alone decides: a segment of exactly RS_MAX_TILES tiles
    (staged), of one more (global), and of RS_MAX_TILES tiles' worth of bytes from an unaligned start (spans one more: global)."""
    from hmse_amd import IngestConfig
    data, segs, _ = E.l2_sparse_tiles(K["L2_TILE"], K["RS_MAX_TILES"])
    for cfg in (IngestConfig(seg_size=64 << 20), IngestConfig.reference_preset().with_(seg_size=64 << 20)):
        for name, so in segs.items():
            check_cuts(orc, dev, data, cfg, so, tag=name)
        check_cuts(orc, dev, data, cfg, tag="one segment")


@pytest.mark.parametrize("name,cfg", l2_cfgs(), ids=[c[0] for c in l2_cfgs()])
def test_l2_candidate_overflow_is_chunked_not_refused(name, cfg, orc, dev, K):
    """More candidates than hmse_workspace_bytes(HMSE_STAGE_L2) provisions for: ops.l2_cdc returns the oracle's cuts (it runs the
    call again with a list of one entry per byte); the C entry point with the DEFAULT workspace reports status bit 0, and with
    4 n more bytes of workspace it does not."""
    import torch
    from hmse_amd import _lib, ops
    pair = pair_for(orc, cfg)
    for n in (400_000, 8 << 20):
        data, _ = E.l2_overflow(pair, n)
        check_cuts(orc, dev, data, cfg, tag=n)
    assert ops.workspace_bytes(ops.STAGE_L2, 8 << 20, cfg) < (8 << 20) // 2 * 4       # the default call did not grow to the worst case
    # the C-ABI, directly
    data, _ = E.l2_overflow(pair, 400_000)
    d = to_dev(data, dev)
    n = d.numel()
    so = ops.segment_offsets(n, cfg.seg_size, dev)
    cap = n // cfg.min_size + so.numel() + 1
    c = cfg.to_c()
    want = orc.cdc(data, ocfg(orc, cfg))
    for extra, overflow in ((0, True), (4 * n + 256, False)):
        cuts = torch.zeros(cap, dtype=torch.int64, device=dev)
        meta = torch.zeros(2, dtype=torch.int64, device=dev)
        ws = torch.empty(ops.workspace_bytes(ops.STAGE_L2, n, cfg) + extra, dtype=torch.uint8, device=dev)
        rc = _lib.hip_lib().hmse_l2_cdc(d.data_ptr(), n, so.data_ptr(), so.numel() - 1, C.byref(c), cuts.data_ptr(), cap, meta.data_ptr(),
                                        meta.data_ptr() + 8, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        n_cuts, status = meta.tolist()
        assert bool(status & 1) == overflow and not (status & ~1), (extra, status)
        if not overflow:
            assert np.array_equal(cuts[: n_cuts + 1].cpu().numpy().astype(np.uint64), want)


def test_l2_dense_stretch_end_to_end(orc, dev):
    """ingest_shard over a corpus with a stretch that overflows the default candidate list: every stage equals the oracle pipeline, and
    read_store returns the bytes."""
    import torch
    from test_gpu_ingest import oracle_pipeline
    from hmse_amd import IngestConfig, corpus, ingest, manifest, read
    cfg = IngestConfig(seg_size=1 << 20)
    data, _ = E.l2_corpus_with_dense_stretch(pair_for(orc, cfg), corpus.wiki_synth(2 << 20, seed=42))
    res = ingest.ingest_shard(to_dev(data, dev), cfg)
    _, (o,) = oracle_pipeline(orc, data, cfg)
    for name, got, want in (("cuts", res.cuts.cpu().numpy().astype(np.uint64), o["cuts"]), ("digests", res.digests.cpu().numpy(), o["dg"]),
                            ("first_occ", res.first_occ.cpu().numpy().astype(np.uint64), o["fo"]), ("uniq", res.uniq_ids.cpu().numpy().astype(np.uint64), o["uniq"]),
                            ("sig", res.sig.cpu().numpy().view(np.uint32), o["sig"]), ("base", res.base.cpu().numpy(), o["base"]),
                            ("kind", res.kind.cpu().numpy(), o["kind"]), ("off", res.stream_off.cpu().numpy().astype(np.uint64), o["off"]),
                            ("streams", res.streams.cpu().numpy(), o["out"])):
        assert got.shape == want.shape and np.array_equal(got, want), name
    assert res.stats["pointer"] > 50 and res.stats["delta"] > 10                # the dense stretch dedupes; the edited text deltas
    store = manifest.merge_manifests([manifest.build_manifest(res, 0, 1)])
    assert torch.equal(read.read_store(store, dev, verify=True), to_dev(data, dev))


def test_l2_overflow_in_the_captured_chain_is_refused_through_the_sticky_status(orc, dev):
    """The device-count chain (one enqueue per batch, no host read) cannot run a batch twice: a batch denser than its fixed candidate list
    sets bit 2 of the sticky status word, publishes no cut, leaves the earlier batches intact and turns every later batch into a no-op;
    finish() raises with the cause.  The host-sized path (graph=False) retries and takes the same bytes."""
    import torch
    from hmse_amd import IngestConfig, corpus, stream
    cfg = IngestConfig(seg_size=1 << 20)
    B = 2 << 20
    text = corpus.wiki_synth(2 * B, seed=42)
    batches = [text[:B], E.pair_run(B, pair_for(orc, cfg)), text[B:]]
    s = stream.StreamIngest(cfg, 3 * B, dev, graph=True)
    for b in batches:
        s.push(torch.from_numpy(b.copy()))
    want1 = orc.cdc(batches[0], ocfg(orc, cfg))
    with pytest.raises(ValueError, match="candidate") as ei:
        s.finish()
    st = s._state.tolist()
    assert st[7] == 4, hex(st[7])                                               # bit 2 and nothing else
    assert st[0] == B and st[1] == len(want1) - 1 and st[8] == st[1]            # counters frozen at the last good batch: no cut published
    assert np.array_equal(s._cuts[: st[1] + 1].cpu().numpy().astype(np.uint64), want1)
    assert f"{B} bytes" in str(ei.value) and f"{st[1]} chunks" in str(ei.value)
    # the host-sized path takes the same three batches
    s2 = stream.StreamIngest(cfg, 3 * B, dev, graph=False)
    for b in batches:
        s2.push(torch.from_numpy(b.copy()))
    r2 = s2.finish()
    assert np.array_equal(r2.cuts.cpu().numpy().astype(np.uint64), orc.cdc(np.concatenate(batches), ocfg(orc, cfg)))


# ---- L1 DEFLATE ------------------------------------------------------------------------------------------------------------------
def dfl_cfgs():
    from hmse_amd import IngestConfig
    return [("default", IngestConfig()), ("level1", IngestConfig(level=1)), ("depth3", IngestConfig(chain_depth=3))]


def profile_counters(lib):
    """Read and reset the token counters of the match kernels (8..13 plain, 18..23 dictionary) and the encode kernels (14, 15, 30, 31)."""
    v = C.c_uint64()
    out = {}
    for s in list(range(8, 16)) + list(range(18, 24)) + [30, 31]:
        assert lib.hmse_profile_counter(s, C.byref(v), 1) == 0
        out[s] = int(v.value)
    return out


def run_jobs(orc, dev, job, cfg, tag):
    """ops.l1_deflate over the job's selection (dictionaries named by chunk id) == orc.deflate_chunks; every record through stock zlib."""
    from hmse_amd import ops
    odata, ocuts, obase, _ = E.oracle_view(job)
    rows = job["ids"].astype(np.int64)
    w_out, w_off, w_kind = orc.deflate_chunks(odata, ocuts, ocfg(orc, cfg), None, obase)
    has_base = bool((job["base"] >= 0).any())
    out, off, kind = ops.l1_deflate(to_dev(job["data"], dev), to_dev(job["cuts"].astype(np.int64), dev), cfg, to_dev(rows, dev),
                                    to_dev(job["base"], dev) if has_base else None, base_is_chunk_id=True)
    out, off, kind = out.cpu().numpy(), off.cpu().numpy().astype(np.int64), kind.cpu().numpy()
    parts = job["parts"]
    for j, r in enumerate(rows):
        want = w_out[int(w_off[r]): int(w_off[r + 1])]
        got = out[off[j]: off[j + 1]]
        info = (tag, j, parts[r].size, int(job["base"][j]))
        assert kind[j] == w_kind[r], info
        assert got.size == want.size and np.array_equal(got, want), info
        zd = parts[int(job["base"][j])].tobytes() if kind[j] == 2 else None
        d = zlib.decompressobj(-15, zdict=zd) if zd else zlib.decompressobj(-15)
        assert d.decompress(got.tobytes()) == parts[r].tobytes(), info
    return w_kind[rows]


@pytest.mark.parametrize("name,cfg", dfl_cfgs(), ids=[c[0] for c in dfl_cfgs()])
@pytest.mark.parametrize("dict_jobs", [False, True], ids=["plain", "dictionary"])
def test_l1_deflate_windows_on_the_class_caps(dict_jobs, name, cfg, orc, dev, K):
    """T = cap - 1, cap, cap + 1 for every size class, five contents, three dictionary splits: records equal the oracle's and inflate
    through zlib; and — class by class, with the profile counters on — the jobs of a class count tokens in that class's slot only."""
    from hmse_amd import _lib, ops
    caps = tuple(ops.DEFLATE_CLASS_CAPS) + (65536,)
    job = E.deflate_boundary_jobs(caps, dict_jobs)
    kinds = run_jobs(orc, dev, job, cfg, name)
    if dict_jobs:
        assert (kinds == 2).sum() >= 40 and (kinds == 0).sum() >= 40          # DELTA, and FULL after a refused delta (second pass)
    # one call per class: the windows (previous cap, cap] and nothing else
    lib = _lib.hip_lib()
    lens = np.diff(job["cuts"].astype(np.int64))
    for c in caps:
        sel = np.flatnonzero([E.window_class(int(t), caps) == c for t in job["T"]])
        if sel.size == 0:
            assert not dict_jobs and c == 65536
            continue
        assert {int(t) for t in job["T"][sel]} >= {c - 1, c}
        sub = dict(job, ids=job["ids"][sel], base=job["base"][sel], T=job["T"][sel], cap=job["cap"][sel])
        lib.hmse_profile_enable(1)
        try:
            profile_counters(lib)                                              # reset
            run_jobs(orc, dev, sub, cfg, (name, "class", c))
            ctr = profile_counters(lib)
        finally:
            lib.hmse_profile_enable(0)
        slot = K["CLASS_SLOT"][c] + (10 if dict_jobs else 0)
        match = {s: v for s, v in ctr.items() if s in range(8, 14) or s in range(18, 24)}
        print(name, "dict" if dict_jobs else "plain", c, {s: v for s, v in ctr.items() if v})
        assert match[slot] > 0, (c, match)
        if not dict_jobs:
            assert all(v == 0 for s, v in match.items() if s != slot), (c, match)
        else:
            # dictionary slots: this class only; plain slots: only the FULL records of refused deltas, in the class of their own length
            assert all(v == 0 for s, v in match.items() if s >= 18 and s != slot), (c, match)
            redo = {K["CLASS_SLOT"][E.window_class(int(lens[int(i)]), caps)] for i in sub["ids"]}
            assert all(v == 0 for s, v in match.items() if s < 18 and s not in redo), (c, match, redo)


@pytest.mark.parametrize("name,cfg", dfl_cfgs(), ids=[c[0] for c in dfl_cfgs()])
@pytest.mark.parametrize("delta", [False, True], ids=["FULL", "DELTA"])
def test_l1_encode_lists_split_at_12288_and_end_at_32768(delta, name, cfg, orc, dev, K):
    """Chunks of 12287 / 12288 and of 12289 / 32767 / 32768 bytes, each list in a call of its own: records exact, and only that
    list's encode kernel (slots 14 / 15 for FULL records, 30 / 31 for DELTA records) read tokens."""
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    job = E.encode_list_jobs(K["ENC_SPLIT"], delta)
    kinds = run_jobs(orc, dev, job, cfg, name)
    assert (kinds == (2 if delta else 0)).all()
    for short in (True, False):
        sel = np.flatnonzero((job["L"] <= K["ENC_SPLIT"]) == short)
        assert sel.size >= 2
        sub = dict(job, ids=job["ids"][sel], base=job["base"][sel])
        lib.hmse_profile_enable(1)
        try:
            profile_counters(lib)
            run_jobs(orc, dev, sub, cfg, (name, "short" if short else "long"))
            ctr = profile_counters(lib)
        finally:
            lib.hmse_profile_enable(0)
        enc = {s: ctr[s] for s in (14, 15, 30, 31)}
        mine = (30 if short else 31) if delta else (14 if short else 15)
        print(name, "DELTA" if delta else "FULL", "short" if short else "long", enc)
        assert enc[mine] > 0 and all(v == 0 for s, v in enc.items() if s != mine), enc


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_l1_deflate_record_offsets_across_the_blocks_of_the_device_scan(n, orc, dev):
    """n chunks of two bytes: the two exclusive scans inside hmse_l1_deflate (record offsets in the workspace, stream offsets in out_off)
    run 1024 elements per workgroup, so n = 1023 / 1024 / 1025 / 2049 is one block short of full, full, two and three blocks.  Offsets,
    kinds and every stream byte equal the oracle's."""
    from hmse_amd import IngestConfig, ops
    cfg = IngestConfig()
    data = words_text(2 * n, seed=n)
    cuts = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
    w_out, w_off, w_kind = orc.deflate_chunks(data, cuts, ocfg(orc, cfg))
    out, off, kind = ops.l1_deflate(to_dev(data, dev), to_dev(cuts.astype(np.int64), dev), cfg)
    assert off.numel() == n + 1 and np.array_equal(off.cpu().numpy().astype(np.uint64), w_off)
    assert np.array_equal(kind.cpu().numpy(), w_kind) and np.array_equal(out.cpu().numpy(), w_out)


def test_l1_deflate_signals_a_chunk_above_32768_bytes(orc, dev):
    """A chunk of 32769 bytes next to normal ones: no crash; status bit 2 (include/hmse.h); the oversized chunk gets an EMPTY record
    (out_off[k + 1] == out_off[k]); every other record is exactly the oracle's.  ops.l1_deflate raises on that status."""
    import torch
    from hmse_amd import IngestConfig, _lib, ops
    from hmse_amd.ops import HmseError
    cfg = IngestConfig()
    text = words_text(200_000, seed=31)
    lens = [5000, 32769, 12000, 32768, 70000, 300, 9000]
    big = [1, 4]
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = text[: int(cuts[-1])].copy()
    data[int(cuts[6]): int(cuts[6]) + 9000] = data[int(cuts[2]): int(cuts[2]) + 9000]
    data[int(cuts[6]) + 77] ^= 1
    base = np.full(len(lens), -1, np.int64)
    base[6] = 2                                                                   # a DELTA record behind the oversized chunks
    ok = [k for k in range(len(lens)) if k not in big]
    obase = np.full(len(ok), -1, np.int64)
    obase[ok.index(6)] = ok.index(2)
    w_out, w_off, w_kind = orc.deflate_chunks(data, cuts, ocfg(orc, cfg), np.array(ok, np.uint64), obase)
    assert w_kind[ok.index(6)] == 2
    d, cu, b = to_dev(data, dev), to_dev(cuts.astype(np.int64), dev), to_dev(base, dev)
    with pytest.raises(HmseError, match="0x4"):
        ops.l1_deflate(d, cu, cfg, None, b)
    # the C entry point: everything else is written
    n = len(lens)
    ln = torch.from_numpy(np.array(lens, np.int64)).to(dev)
    need = int(ops.record_bytes(ln, b >= 0).sum().item())
    c = cfg.to_c()
    ws = torch.empty(ops.workspace_bytes(ops.STAGE_DEFLATE, n, cfg) + need + 4096, dtype=torch.uint8, device=dev)
    cap = int(cuts[-1]) + 64 * n + 4096
    out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    kind = torch.zeros(n, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.hip_lib().hmse_l1_deflate_ex(d.data_ptr(), d.numel(), cu.data_ptr(), None, b.data_ptr(), n, C.byref(c), 0, out.data_ptr(), cap,
                                          off.data_ptr(), kind.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert int(status.item()) == 4
    off, out, kind = off.cpu().numpy(), out.cpu().numpy(), kind.cpu().numpy()
    for k in big:
        assert off[k + 1] == off[k] and kind[k] == 0
    for j, k in enumerate(ok):
        assert kind[k] == w_kind[j], k
        assert np.array_equal(out[off[k]: off[k + 1]], w_out[int(w_off[j]): int(w_off[j + 1])]), k
    assert off[-1] == w_off[-1]


# ---- L4 MinHash ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed_base", [0, 1])
@pytest.mark.parametrize("memo", [True, False], ids=["memo", "no-memo"])
def test_l4_minhash_on_the_pass_boundary(memo, seed_base, orc, dev, K):
    """Chunks whose shingle count sits on one and two passes of MH_SUB through the LDS set (all-distinct: load factor 0.75; 'abcd';
    text), and the sentinel chunks, whose five distinct shingles each hold the minimum of about a fifth of the seeds — one shingle
    dropped or doubled at the pass boundary changes the signature."""
    from hmse_amd import IngestConfig, ops
    cfg = IngestConfig(seed_base=seed_base)
    data, cuts, facts = E.minhash_boundary_chunks(K["MH_SUB"])
    d, cu = to_dev(data, dev), to_dev(cuts.astype(np.int64), dev)
    want = orc.minhash_chunks(data, cuts, ocfg(orc, cfg))
    got = ops.l4_minhash(d, cu, cfg, memo=memo).cpu().numpy().view(np.uint32)
    bad = np.flatnonzero((got != want).any(axis=1)).tolist()
    assert not bad, (bad, [k for k, v in facts["rows"].items() if set(v) & set(bad)])
    rows = facts["rows"]
    ids = np.array(rows["sentinel"][::-1] + rows["distinct"] + rows["plain"] + rows["abcd"][1::2] + rows["text"][::3], dtype=np.uint64)
    got = ops.l4_minhash(d, cu, cfg, to_dev(ids.astype(np.int64), dev), memo=memo).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want[ids.astype(np.int64)])
    assert np.array_equal(got, orc.minhash_chunks(data, cuts, ocfg(orc, cfg), ids))


# ---- L3 / L4 tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16384, 16385, 40000], ids=["mask-32767", "mask-65535", "all"])
def test_l3_dedup_equal_home_slots_and_the_last_slot(n, orc, dev):
    """4096 different digests sharing their first four bytes (one home slot: a probe run of 4096), 4096 whose home slot is the table's
    LAST slot (every probe wraps to slot 0), duplicates of both, among random digests; n on both sides of a power of two of the size
    rule.  The one-call dedupe and the incremental index (several old / new splits) equal the oracle."""
    import torch
    from hmse_amd import ops
    dg, _ = E.planted_digests(20000)
    dg = np.ascontiguousarray(dg[: min(n, dg.shape[0])])
    n = dg.shape[0]
    first4 = np.ascontiguousarray(dg[:, :4]).view("<u4").reshape(-1)
    assert (first4 == 0xFFFFFFFF).sum() > 1000 and (first4 == 0x78563412).sum() > 1000
    fo_w, rc_w = orc.dedup(dg)
    d = to_dev(dg, dev)
    fo, rc = ops.l3_dedup(d)
    assert np.array_equal(fo.cpu().numpy().astype(np.uint64), fo_w)
    assert np.array_equal(rc.cpu().numpy().astype(np.uint32), rc_w)
    slots = ops.l3_index_slots(n)
    assert slots == E.table_slots(n)
    for splits in ([n], [1, n], [n // 3, n // 2, n - 1, n], [4096, 8192, 8193, n]):
        table = torch.empty(slots, dtype=torch.int32, device=dev)
        fo = torch.full((n,), -1, dtype=torch.int64, device=dev)
        rc = torch.full((n,), -1, dtype=torch.int32, device=dev)
        a = 0
        for e in splits:
            ops.l3_index_update(d, a, e - a, fo, rc, table)
            a = e
        assert np.array_equal(fo.cpu().numpy().astype(np.uint64), fo_w), splits
        assert np.array_equal(rc.cpu().numpy().astype(np.uint32), rc_w), splits


@pytest.mark.parametrize("band_bits", [12, 16, 32])
@pytest.mark.parametrize("bands,rows", [(4, 32), (8, 16), (16, 8)])
def test_l4_lsh_equal_keys_over_different_bands(bands, rows, band_bits, orc, dev):
    """300 000 signatures: the oracle's own keys hold pairs of DIFFERENT band rows with EQUAL 32-bit keys (same home slot, told apart by
    content only), plus whole-band copies across the population.  One call and the incremental tables (several old / new splits)
    equal orc.lsh of the whole array."""
    import torch
    from hmse_amd import IngestConfig, ops
    cfg = IngestConfig(bands=bands, rows=rows, band_bits=band_bits)
    n = E.LSH_N
    sig = E.lsh_population(n, bands, rows)
    keys_w, base_w = orc.lsh(sig, ocfg(orc, cfg))
    assert sum(E.equal_key_different_rows(sig, keys_w, rows)) >= 3
    s = to_dev(sig.view(np.int32), dev)
    keys, base = ops.l4_lsh(s, cfg)
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), keys_w)
    assert np.array_equal(base.cpu().numpy(), base_w)
    slots = ops.l4_lsh_slots(n)
    for splits in ([n], [1, 100_000, 100_001, n], [n // 2, n]):
        tables = torch.empty((bands, slots), dtype=torch.int32, device=dev)
        keys = torch.zeros((n, bands), dtype=torch.int32, device=dev)
        base = torch.full((n,), -7, dtype=torch.int64, device=dev)
        a = 0
        for e in splits:
            ops.l4_lsh_update(s, a, e - a, cfg, keys, base, tables)
            a = e
        assert np.array_equal(keys.cpu().numpy().view(np.uint32), keys_w), splits
        assert np.array_equal(base.cpu().numpy(), base_w), splits


# ---- band tables and index sort ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.BT_N)
def test_band_tables_and_index_sort_around_tiles_and_2_16(n, dev):
    from hmse_amd import bandtable, ops
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 32, (n, 3), dtype=np.uint64).astype(np.uint32)
    keys[:, 1] = rng.integers(0, 40, n)                                         # crowded buckets, equal keys: stability decides
    keys[:, 2] = 0x00070007                                                     # ONE bucket and one key for all n ids
    sig = rng.integers(0, 1 << 32, (n, 128), dtype=np.uint64).astype(np.uint32)
    kd = to_dev(keys.view(np.int32), dev)
    for bits in (16, 12):
        assert bandtable.write_band_tables_device(kd, bits) == bandtable.write_band_tables(keys.view(np.int32), bits), bits
    assert bandtable.write_band_tables_device(kd, 16, signatures=to_dev(sig.view(np.int32), dev)) == \
        bandtable.write_band_tables(keys.view(np.int32), 16, signatures=sig.view(np.int32))
    k4 = np.ascontiguousarray(np.concatenate([keys, keys[:, :1] | np.uint32(0xFFFFFF00)], axis=1))    # a fourth band at the top of the u32 range
    sk, si = ops.l4_index_build(to_dev(k4.view(np.int32), dev))
    for b in range(4):
        o = np.argsort(k4[:, b], kind="stable")
        assert np.array_equal(si[b].cpu().numpy(), o), b
        assert np.array_equal(sk[b].cpu().numpy().view(np.uint32), k4[o, b]), b


@pytest.mark.parametrize("spread", [False, True], ids=["contiguous", "spread"])
@pytest.mark.parametrize("hot", E.BT_HOT)
def test_band_tables_and_index_sort_bucket_of_exactly_one_and_two_pieces(hot, spread, dev):
    """One bucket of exactly 65534 / 65535 / 65536 / 131070 / 131071 ids (a continuation header from the 65536th id on), its ids
    contiguous or spread over every tile."""
    from hmse_amd import bandtable, ops
    keys, facts = E.hot_bucket_keys(200_000, hot, spread)
    kd = to_dev(keys.view(np.int32), dev)
    want = bandtable.write_band_tables(keys.view(np.int32), 16)
    assert bandtable.write_band_tables_device(kd, 16) == want
    _, tables = bandtable.read_band_tables(want)
    bh, start, cnt, ids = tables[1]
    k = int(np.flatnonzero(bh == facts["bucket"])[0])
    assert int(cnt[k]) == hot
    # the same population as ONE KEY of the index sort (a run of `hot` equal keys)
    k2 = keys.copy()
    k2[facts["hot_ids"], 1] = 0x80001234
    sk, si = ops.l4_index_build(to_dev(k2.view(np.int32), dev))
    for b in range(2):
        o = np.argsort(k2[:, b], kind="stable")
        assert np.array_equal(si[b].cpu().numpy(), o), b
        assert np.array_equal(sk[b].cpu().numpy().view(np.uint32), k2[o, b]), b
