"""GPU: every capped or persistent grid of tests/grid_caps.py taken through two full trips and a ragged third, bit for bit against a plain
reference: hashlib, the CPU oracle (inflate, MinHash), tests/similarity_ref.py, zlib.crc32, bytes.find at the planted places.  The inputs
and what they promise are proved on the CPU in tests/test_grid_caps_host.py; every comparison here is exact equality."""
import ctypes as C

import numpy as np
import pytest

import find_ref
import grid_caps as G
import similarity_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    return G.kernel_constants()


def _t(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


# ---- SHA-256 ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sha(K, dev):
    data, cuts, facts = G.sha_chunks(K)
    return _t(data, dev), _t(cuts, dev), G.sha_reference(data, cuts), facts


@pytest.mark.parametrize("order", ["longest-first", "index-order"])
def test_sha256_lanes_hash_a_second_and_a_third_chunk(sha, K, dev, order):
    """524 365 chunks on 262 144 lanes: every lane takes a chunk after its first (the refill: state seeded again, a prefetched block of the
    chunk before left behind), with the order table (chunks handed out longest first) and with a workspace too small for it (index order:
    a lane goes from a 32 KiB chunk to an empty one)."""
    import torch
    from hmse_amd import IngestConfig, ops
    data, cuts, want, facts = sha
    if order == "longest-first":
        assert ops.workspace_bytes(ops.STAGE_SHA, facts["count"], IngestConfig()) >= G.sha_order_workspace(K, facts["count"])
        got = ops.l3_sha256(data, cuts)
    else:
        got = torch.full((facts["count"], 32), 0x5A, dtype=torch.uint8, device=dev)
        ws = torch.empty(256, dtype=torch.uint8, device=dev)                          # holds the hand-out counter and nothing else
        ops._call("hmse_l3_sha256", data, data.numel(), cuts, facts["count"], got, ws, ws.numel())
    got = got.cpu().numpy()
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (bad.size, bad[:10], G.trip_of(bad[:10], facts["lanes"]))


# ---- inflate, a stream a lane --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def records(K, orc, dev):
    recs, facts = G.inflate_records(K)
    streams, off, kind, base, raw_len = G.pack_records(recs)
    want = orc.inflate_chunks(streams, off, kind, base, raw_len)
    return tuple(_t(a, dev) for a in (streams, off, kind, base, raw_len)), want, facts


@pytest.mark.parametrize("mode", [2, 0], ids=["forced", "automatic"])
def test_inflate_lanes_pull_a_second_and_a_third_stream(records, K, dev, mode):
    """264 517 records on 131 072 lanes, more FULL records than lanes: a lane takes a FULL record after a FULL record, a DELTA after
    either, and a third record.  Bytes and accept / reject decisions are the oracle's.  (Progress: a DELTA record's base has a smaller
    index, pass 1 hands out every FULL record before pass 2 starts, and pass 2 hands the DELTA records out in index order, so a lane
    only ever waits for a record that another lane holds or has finished.)"""
    from hmse_amd import ops
    (streams, off, kind, base, raw_len), (want_raw, want_off, want_ok), facts = records
    assert facts["count"] >= K["IFL_WIDE_MIN"]
    ops.l1_inflate_mode(mode)
    try:
        raw, raw_off, ok = ops.l1_inflate(streams, off, kind, base, raw_len, check=False)
    finally:
        ops.l1_inflate_mode(0)
    raw, raw_off, ok = raw.cpu().numpy(), raw_off.cpu().numpy().astype(np.uint64), ok.cpu().numpy().astype(bool)
    assert np.array_equal(raw_off, want_off)
    assert np.array_equal(ok, want_ok), np.flatnonzero(ok != want_ok)[:10]
    keep = np.repeat(want_ok, np.diff(want_off.astype(np.int64)))                      # the bytes of the accepted records
    diff = np.flatnonzero((raw[: keep.size] != want_raw)[keep])
    assert diff.size == 0, diff[:10]


# ---- MinHash ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memo", [True, False], ids=["memo", "no-memo"])
def test_minhash_workgroups_sign_a_second_and_a_third_chunk(K, orc, dev, memo):
    from dataclasses import asdict
    from hmse_amd import IngestConfig, ops
    data, cuts, facts = G.minhash_chunks(K)
    cfg = IngestConfig()
    want = orc.minhash_chunks(data, cuts.astype(np.uint64), orc.default_cfg(**asdict(cfg)))
    got = ops.l4_minhash(_t(data, dev), _t(cuts, dev), cfg, memo=memo).cpu().numpy().view(np.uint32)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (bad.size, bad[:10], G.trip_of(bad[:10], K["MH_GRID"]))


# ---- query --------------------------------------------------------------------------------------------------------------------------------
def test_query_workgroups_score_a_second_and_a_third_query(K, dev):
    """16 429 queries on 8 192 workgroups against 3000 stored signatures.  The first 8192 all have 300 candidates (the hit buffer is reduced,
    the threshold raised far above 32): every workgroup that takes a later query comes from one of them, and the later queries have no
    candidate, or one to four of score 32 which a threshold carried over would drop, or 300 again."""
    from hmse_amd import IngestConfig, ops
    S, Q, facts = G.query_signatures(K)
    cfg = ops.search_cfg(IngestConfig(), facts["bands"])
    sig_s, sig_q = _t(S.view(np.int32), dev), _t(Q.view(np.int32), dev)
    sk, si = ops.l4_index_build(ops.l4_lsh(sig_s, cfg)[0])
    keys_q = ops.l4_lsh(sig_q, cfg)[0]
    pairs = similarity_ref.candidate_pairs(S, Q, facts["bands"])
    for top_k, min_score in ((8, 0), (1, 0), (64, 0), (64, 40)):
        ids, sc, nh, nc = ops.l4_query(sig_q, keys_q, sig_s, sk, si, cfg, top_k, min_score)
        w_ids, w_sc, w_nh, w_nc = similarity_ref.select(*pairs, len(Q), top_k, min_score)
        assert np.array_equal(nc.cpu().numpy(), w_nc), (top_k, min_score)
        assert np.array_equal(nh.cpu().numpy(), w_nh), (top_k, min_score)
        assert np.array_equal(ids.cpu().numpy(), w_ids), (top_k, min_score)
        assert np.array_equal(sc.cpu().numpy(), w_sc), (top_k, min_score)


# ---- CRC-32 -------------------------------------------------------------------------------------------------------------------------------
def test_crc32_workgroups_take_a_second_and_a_third_range(K, dev):
    from hmse_amd import ops
    data, cuts, facts = G.crc_ranges(K)
    got = ops.crc32(_t(data, dev), _t(cuts, dev)).cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got != G.crc_reference(data, cuts))
    assert bad.size == 0, (bad.size, bad[:10])


def test_crc32_cuts_are_validated_beyond_the_first_trip(K, dev):
    """2 097 229 ranges, 1 048 576 to a trip of the kernel that checks the cuts: valid cuts give zlib's CRCs; one descending pair in the
    second trip, or in the ragged third, refuses the call and leaves the output as it was."""
    import torch
    from hmse_amd import ops
    data, cuts, facts = G.many_tiny_ranges(K)
    data_d = _t(data, dev)
    got = ops.crc32(data_d, _t(cuts, dev)).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, G.tiny_crc_reference(data, cuts))
    for i in facts["bad_at"]:
        bad = cuts.copy()
        bad[i], bad[i + 1] = cuts[i + 1], cuts[i]
        out = torch.full((facts["count"],), -7, dtype=torch.int32, device=dev)
        with pytest.raises(ops.HmseError, match="descends"):
            ops.crc32(data_d, _t(bad, dev), out=out)
        assert bool((out == -7).all()), i


# ---- the scans ----------------------------------------------------------------------------------------------------------------------------
def _in_every_trip(positions, tile, cap):
    return set(np.unique(G.trip_of(np.asarray(positions) // tile, cap)).tolist()) == {0, 1, 2}


def _pairs(hits, bits):
    h = np.sort(hits.cpu().numpy())
    return list(zip((h >> bits).tolist(), (h & ((1 << bits) - 1)).tolist()))


@pytest.fixture(scope="module")
def find_input(K, dev):
    raw, raw_off, facts = G.scan_input(K["FIND_TILE"], K["FIND_MAX_BLOCKS"], G.FIND_MANY_PATTERNS, seed=71)
    return raw, raw_off, facts, _t(raw, dev), _t(raw_off, dev)


@pytest.mark.parametrize("group,ic", [("few", False), ("many", False), ("few", True), ("many", True)])
def test_find_scan_strides_over_more_tiles_than_the_grid(find_input, K, dev, group, ic):
    """4099 tiles on 2048 workgroups: occurrences in every trip, across the seams of the trips, clipped by a record's end, and ending on
    the last byte; FIND_FEW patterns (the head compare) and more (the bitmap)."""
    from hmse_amd import find, ops
    raw, raw_off, facts, raw_d, ro_d = find_input
    pats = G.FIND_FEW_PATTERNS if group == "few" else G.FIND_MANY_PATTERNS
    assert (len(pats) <= K["FIND_FEW"]) == (group == "few")
    want, want_counts = G.planted_hits(raw, raw_off, facts["places"], pats, ic)
    flat, off = find.pack_patterns(pats)
    hits, n, counts = ops.find_scan(raw_d, ro_d, None, _t(flat, dev), off, ic)
    assert n == len(want) and counts.tolist() == want_counts
    assert _pairs(hits, 8) == want
    assert (raw.size - len(pats[0]), 0) in want and _in_every_trip([o for o, _ in want], K["FIND_TILE"], K["FIND_MAX_BLOCKS"])


@pytest.mark.parametrize("ic", [False, True])
def test_findset_scan_strides_over_more_tiles_than_the_grid(K, dev, ic):
    """1027 tiles on 512 workgroups (each with the set's bitmap in LDS, built once), as the grouped scan's test."""
    from hmse_amd import find, ops
    raw, raw_off, facts = G.scan_input(K["FSET_TILE"], K["FSET_MAX_BLOCKS"], G.FSET_PATTERNS, seed=73)
    ps = find.PatternSet(G.FSET_PATTERNS, ic, dev)
    assert ps.n_unique == len(G.FSET_PATTERNS) and ps.index.tolist() == list(range(ps.n_unique))
    want, want_counts = G.planted_hits(raw, raw_off, facts["places"], G.FSET_PATTERNS, ic)
    hits, n, counts = ops.findset_scan(_t(raw, dev), _t(raw_off, dev), None, ps.set)
    assert n == len(want) and counts.tolist() == want_counts
    assert _pairs(hits, 24) == want
    assert (raw.size - len(G.FSET_PATTERNS[0]), 0) in want and _in_every_trip([o for o, _ in want], K["FSET_TILE"], K["FSET_MAX_BLOCKS"])


def _raw_find_scan(dev, raw_d, ro_d, n_rec, pat, cap):
    """hmse_find_scan called directly, every output prefilled with -7 -> (rc, hits, n_hits, counts, status)."""
    import torch
    from hmse_amd import _lib
    pat_d = _t(np.frombuffer(pat, np.uint8), dev)
    hits = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    nh = torch.full((1,), -7, dtype=torch.int64, device=dev)
    counts = torch.full((1,), -7, dtype=torch.int64, device=dev)
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    rc = _lib.hip_lib().hmse_find_scan(raw_d.data_ptr(), raw_d.numel(), ro_d.data_ptr(), n_rec, None, pat_d.data_ptr(), (C.c_uint32 * 2)(0, len(pat)), 1, 0,
                                       hits.data_ptr(), cap, nh.data_ptr(), counts.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, hits, int(nh.item()), counts.tolist(), int(status.item())


@pytest.mark.parametrize("which", ["find", "findset"])
def test_tables_are_validated_beyond_the_first_trip(K, dev, which):
    """1 048 653 records, 524 288 to a trip of tables_validate_kernel (2 097 229 and 1 048 576 for findset_validate_kernel).  The valid
    table: the scan's hits are the reference's.  One pair of bounds out of order in the second trip, or in the ragged third, and nothing
    else wrong: status bit 1 (value 2), and the scan behind it leaves its outputs alone."""
    from hmse_amd import find, ops
    per = K["FIND_MAX_BLOCKS"] * K["FIND_NT"] if which == "find" else K["FSET_VALIDATE_BLOCKS"] * K["FSET_NT"]
    raw, raw_off, facts = G.many_records(per)
    pat = facts["pattern"]
    want, want_counts = G.planted_hits(raw, raw_off, facts["places"], [pat])
    raw_d = _t(raw, dev)
    if which == "findset":
        ps = find.PatternSet([pat], False, dev)
        hits, n, counts = ops.findset_scan(raw_d, _t(raw_off, dev), None, ps.set)
        assert _pairs(hits, 24) == want and n == len(want) and counts.tolist() == want_counts
        for i in facts["bad_at"]:
            bad = raw_off.copy()
            bad[i], bad[i + 1] = raw_off[i + 1], raw_off[i]
            with pytest.raises(ops.HmseError, match="inconsistent"):
                ops.findset_scan(raw_d, _t(bad, dev), None, ps.set)
        return
    rc, hits, n, counts, status = _raw_find_scan(dev, raw_d, _t(raw_off, dev), facts["count"], pat, len(want) + 64)
    assert rc == 0 and status == 0 and n == len(want) and counts == want_counts
    assert _pairs(hits[:n], 8) == want and bool((hits[n:] == -7).all())
    for i in facts["bad_at"]:
        bad = raw_off.copy()
        bad[i], bad[i + 1] = raw_off[i + 1], raw_off[i]
        rc, hits, n, counts, status = _raw_find_scan(dev, raw_d, _t(bad, dev), facts["count"], pat, len(want) + 64)
        assert rc == 0 and status == 2 and n == 0 and counts == [0] and bool((hits == -7).all()), i


# ---- the seams -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["find", "findset"])
def test_seams_stride_over_more_pairs_than_the_grid(K, dev, which):
    """One thread per (chunk, distance from its end): 255 distances of a 256-byte pattern over enough chunks for two trips and a ragged
    third of find_seams_kernel (2048 x 256 threads) and of findset_seams_kernel (4096 x 512)."""
    from hmse_amd import find, ops
    per = K["FIND_MAX_BLOCKS"] * K["FIND_NT"] if which == "find" else K["FSET_SEAMS_BLOCKS"] * K["FSET_NT"]
    corpus, cuts, pats, facts = G.seam_corpus(per, 255, seed=79 if which == "find" else 83)
    _, want = find_ref.split(corpus, pats, cuts)
    raw_d, cu = _t(np.frombuffer(corpus, np.uint8), dev), _t(np.asarray(cuts, np.int64), dev)
    slot = _t(np.arange(len(cuts) - 1, dtype=np.int64), dev)                          # every chunk is its own record
    if which == "find":
        flat, off = find.pack_patterns(pats)
        hits, n, counts = ops.find_seams(raw_d, cu, cu, slot, _t(flat, dev), off)
        got = _pairs(hits, 8)
    else:
        ps = find.PatternSet(pats, False, dev)
        assert ps.index.tolist() == list(range(len(pats)))
        hits, n, counts = ops.findset_seams(raw_d, cu, cu, slot, ps.set)
        got = _pairs(hits, 24)
    assert got == want and n == len(want) and counts.tolist() == [sum(1 for _, j in want if j == q) for q in range(len(pats))]
    chunk = np.searchsorted(np.asarray(cuts), [o for o, _ in want], side="right") - 1          # seam hits in every trip
    assert set(np.unique(G.trip_of(chunk * 255, per)).tolist()) == {0, 1, 2} and {j for _, j in want} == set(range(len(pats)))


# ---- ranges ---------------------------------------------------------------------------------------------------------------------------------
def test_ranges_are_checked_beyond_the_first_trip(K, dev):
    """1 048 653 ranges, 524 288 to a trip of lines_ranges_kernel and of tally_ranges_kernel: the gathered bytes and the equalities are
    numpy's; one range of the second trip, or of the ragged third, that leaves the corpus, or one rep outside the ranges, refuses the call."""
    from hmse_amd import ops
    per = K["LINES_MAX_BLOCKS"] * K["LINES_NT"]
    corpus, cuts, start, end, rep, facts = G.many_ranges(per)
    want, out_off = G.gathered(corpus, start, end)
    raw_d, cu = _t(corpus, dev), _t(cuts, dev)
    slot = _t(np.arange(len(cuts) - 1, dtype=np.int64), dev)
    st_d, en_d, rep_d = _t(start, dev), _t(end, dev), _t(rep, dev)
    got = ops.lines_gather(raw_d, cu, cu, slot, st_d, en_d, _t(out_off, dev), int(out_off[-1]))
    assert np.array_equal(got.cpu().numpy(), want)
    same = ops.tally_same(raw_d, cu, cu, slot, st_d, en_d, rep_d)
    assert np.array_equal(same.cpu().numpy(), G.same_ranges(corpus, start, end, rep))
    for i in facts["bad_at"]:
        bad_end, bad_rep = end.copy(), rep.copy()
        bad_end[i] = corpus.size + 1                                                   # leaves the corpus (out_off no longer fits either)
        bad_rep[i] = facts["count"]
        with pytest.raises(ops.HmseError, match="leaves the corpus"):
            ops.lines_gather(raw_d, cu, cu, slot, st_d, _t(bad_end, dev), _t(out_off, dev), int(out_off[-1]))
        with pytest.raises(ops.HmseError, match="leaves the corpus"):
            ops.tally_same(raw_d, cu, cu, slot, st_d, _t(bad_end, dev), rep_d)
        with pytest.raises(ops.HmseError, match="rep outside"):
            ops.tally_same(raw_d, cu, cu, slot, st_d, en_d, _t(bad_rep, dev))


# ---- deflate's gather --------------------------------------------------------------------------------------------------------------------------
def test_deflate_gathers_more_records_than_its_grid_has_wavefronts(K, orc, dev):
    """131 109 chunks of 2..40 bytes through hmse_l1_deflate: its gather kernel copies a record per wavefront with 65 536 wavefronts.
    Offsets, kinds and every stream byte are the oracle's."""
    from dataclasses import asdict
    from hmse_amd import IngestConfig, ops
    data, cuts, facts = G.tiny_chunks(K)
    cfg = IngestConfig()
    w_out, w_off, w_kind = orc.deflate_chunks(data, cuts.astype(np.uint64), orc.default_cfg(**asdict(cfg)))
    out, off, kind = ops.l1_deflate(_t(data, dev), _t(cuts, dev), cfg)
    assert np.array_equal(off.cpu().numpy().astype(np.uint64), w_off) and np.array_equal(kind.cpu().numpy(), w_kind)
    assert np.array_equal(out.cpu().numpy(), w_out)
