"""CPU: every builder of tests/edge_inputs.py reaches the branch it is meant for — proved from the reference (the oracle's Gear table,
masks, MinHash, LSH keys and dedupe) and from the constants in the kernel sources, never from the device.  If someone retunes a cap,
these fail before the GPU tests quietly stop covering it."""
from dataclasses import asdict

import numpy as np
import pytest

import edge_inputs as E


def _cfgs():
    from hmse_amd import IngestConfig
    return [IngestConfig(), IngestConfig.reference_preset(), IngestConfig(norm_level=0), IngestConfig(norm_level=3)]


def _masks(orc, cfg):
    return orc.cdc_masks(orc.default_cfg(**asdict(cfg)))


@pytest.fixture(scope="module")
def K():
    return E.kernel_constants()


def test_constants_are_the_kernel_source_s(K):
    from hmse_amd import ops
    assert K["L2_TILE"] == 32768 and K["MH_SUB"] == 12288 and K["RS_MAX_CAND"] < K["CAND_SLACK"]
    caps = tuple(ops.DEFLATE_CLASS_CAPS) + (65536,)
    assert sorted(K["CLASS_SLOT"]) == list(caps) and sorted(K["CLASS_SLOT"].values()) == list(range(8, 14))
    assert K["ENC_SPLIT"] == 12288 and K["BT_PIECE"] == 65535 and K["BT_NT"] == 256


def test_gear_candidates_window_form_equals_the_rolling_hash(orc):
    """The vectorised window form against the plain recurrence h = (h << 1) + G[b] on random bytes."""
    G = orc.gear_table()
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 5000, dtype=np.uint8)
    mask = (0xFFFF << 58) & 0xFFFFFFFFFFFFFFFF        # 6 bits: plenty of hits
    h, want = 0, []
    for b in data:
        h = ((h << 1) + int(G[b])) & 0xFFFFFFFFFFFFFFFF
        want.append((h & mask) == 0)
    assert np.array_equal(E.gear_candidates(data, G, mask, block=1000), np.array(want)) and sum(want) > 30


@pytest.mark.parametrize("i", range(4), ids=["default", "reference", "norm0", "norm3"])
def test_dense_pairs_exist_and_fill_every_second_position(i, orc, K):
    cfg = _cfgs()[i]
    G = orc.gear_table()
    _, ml = _masks(orc, cfg)
    pairs = E.dense_pairs(G, ml)
    assert pairs, "no byte pair whose alternating run passes the easy mask: the dense inputs cannot be built for this configuration"
    # the global walk by candidate count: above RS_MAX_CAND, inside the provisioned list
    data, facts = E.l2_dense_segment(pairs[0])
    c = int(E.gear_candidates(data, G, ml).sum())
    assert abs(c - facts["candidates_about"]) <= 64
    assert K["RS_MAX_CAND"] < c <= E.l2_cand_capacity(data.size, cfg, K)
    assert E.tiles_spanned(0, data.size, K["L2_TILE"]) <= K["RS_MAX_TILES"]
    # the mixed segment: tiles with no candidate, a few, and tile / 2
    text = E.words_text(8 * K["L2_TILE"], seed=3)
    data, facts = E.l2_mixed_segment(pairs[0], text, K["L2_TILE"])
    cand = E.gear_candidates(data, G, ml)
    per_tile = np.add.reduceat(cand, np.arange(0, data.size, K["L2_TILE"]))
    assert K["RS_MAX_CAND"] < int(cand.sum()) <= E.l2_cand_capacity(data.size, cfg, K)
    assert (per_tile == 0).any() and ((per_tile > 0) & (per_tile < 200)).any() and (per_tile == K["L2_TILE"] // 2).any()
    assert per_tile[0] == K["L2_TILE"] // 2 - 31 or per_tile[0] >= K["L2_TILE"] // 2 - 32     # dense from the first window on
    assert cand[-1] or cand[-2]                                                              # and up to the last byte
    # overflow: more candidates than the provisioned list holds, at both sizes
    for n in (400_000, 8 << 20):
        assert n // 2 - 64 > E.l2_cand_capacity(n, cfg, K)
    data, _ = E.l2_overflow(pairs[0], 400_000)
    assert int(E.gear_candidates(data, G, ml).sum()) > E.l2_cand_capacity(data.size, cfg, K)


def test_no_constant_byte_is_dense(orc):
    """Why the existing 'zeros' / 'ones' cases never got there."""
    from hmse_amd import IngestConfig
    G = orc.gear_table()
    _, ml = _masks(orc, IngestConfig())
    for b in range(256):
        assert not E.gear_candidates(np.full(200, b, np.uint8), G, ml)[64:].any()


def test_l2_tile_count_inputs(orc, K):
    """Segments above RS_MAX_TILES tiles (40 MiB in one segment; 33 MiB + 1), and the sparse input whose candidate count stays under
    RS_MAX_CAND so that the tile count alone picks the walk."""
    from hmse_amd import IngestConfig
    tile, mt = K["L2_TILE"], K["RS_MAX_TILES"]
    n = 40 << 20
    assert E.tiles_spanned(0, n, tile) > mt and E.tiles_spanned(0, (33 << 20) + 1, tile) > mt
    assert E.tiles_spanned((33 << 20) + 1, n, tile) <= mt
    data, segs, facts = E.l2_sparse_tiles(tile, mt)
    G = orc.gear_table()
    for cfg in (IngestConfig(), IngestConfig.reference_preset()):
        _, ml = _masks(orc, cfg)
        cand = E.gear_candidates(data, G, ml)
        assert 100 < int(cand.sum()) <= K["RS_MAX_CAND"], "the sparse input must leave the choice of walk to the tile count"
    for name, so in segs.items():
        got = [E.tiles_spanned(int(a), int(b), tile) for a, b in zip(so[:-1], so[1:])]
        want = facts["tiles_spanned"][name]
        assert [g for g, w in zip(got, want) if w is not None] == [w for w in want if w is not None], name
        assert got[-1] <= mt
    assert facts["tiles_spanned"]["exactly"][0] == mt and facts["tiles_spanned"]["one_more"][0] == mt + 1
    so = segs["unaligned"]
    assert int(so[1]) % tile != 0 and int(so[2] - so[1]) == mt * tile          # mt tiles' worth of bytes, one tile more spanned


def test_deflate_windows_sit_on_every_cap(K):
    from hmse_amd import ops
    caps = tuple(ops.DEFLATE_CLASS_CAPS) + (65536,)
    for dict_jobs in (False, True):
        job = E.deflate_boundary_jobs(caps, dict_jobs)
        lens = np.diff(job["cuts"].astype(np.int64))
        L = lens[job["ids"].astype(np.int64)]
        D = np.where(job["base"] >= 0, np.minimum(lens[np.maximum(job["base"], 0)], 32768), 0)
        assert np.array_equal(L + D, job["T"]) and L.max() <= 32768 and L.min() >= 1
        assert (job["base"] >= 0).all() == dict_jobs and (job["base"] >= 0).any() == dict_jobs
        for c in caps:
            want = {c - 1, c, c + 1} if c < 65536 else {c - 1, c}
            if not dict_jobs:
                want = {t for t in want if t <= 32768}
            assert set(job["T"][job["cap"] == c].tolist()) == want, (dict_jobs, c)
            for t in want:                                               # one byte either side is the NEXT class
                assert E.window_class(t, caps) == (c if t <= c else caps[caps.index(c) + 1])
        if dict_jobs:
            d_raw = lens[job["base"]]
            assert (d_raw <= 3).sum() >= 15 * 5 and (np.abs(d_raw - L) <= 1).sum() >= 17 * 5 and (d_raw > 32768).sum() >= 3 * 5
            assert L[d_raw > 32768].max() == 32768 and L[d_raw > 32768].min() == 1
        # every content occurs at every window
        assert len(job["T"]) % len(E.CONTENTS) == 0
        # the oracle's view keeps every job's bytes and window
        data, cuts, base, rows = E.oracle_view(job)
        ol = np.diff(cuts.astype(np.int64))
        assert np.array_equal(ol[rows], L) and ol.max() <= 32768
        assert np.array_equal(ol[rows] + np.where(base[rows] >= 0, ol[np.maximum(base[rows], 0)], 0), job["T"])
    for delta in (False, True):
        job = E.encode_list_jobs(K["ENC_SPLIT"], delta)
        assert job["L"].tolist() == [12287, 12288, 12289, 32767, 32768]


def test_minhash_chunks_sit_on_the_pass_boundary(orc, K):
    from hmse_amd import IngestConfig
    sub = K["MH_SUB"]
    data, cuts, facts = E.minhash_boundary_chunks(sub)
    rows, sh = facts["rows"], facts["shingles"]
    want = [sub - 1, sub, sub + 1, 2 * sub - 1, 2 * sub, 2 * sub + 1, 32765]
    for g in ("distinct", "abcd", "text"):
        assert sh[rows[g]].tolist() == want
    assert 32765 > 2 * sub + 1 and 32765 < 3 * sub
    for r in rows["distinct"]:                                        # load factor 0.75 in every full pass: all shingles differ
        c = facts["parts"][r]
        v = np.lib.stride_tricks.sliding_window_view(c, 4)
        u = np.ascontiguousarray(v).view(np.uint32).reshape(-1)
        assert np.unique(u).size == c.size - 3
    for r in rows["abcd"]:
        c = facts["parts"][r]
        assert np.unique(np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(c, 4)).view(np.uint32)).size == 4
    # the sentinel: for each of the shingles sub - 1, sub, 2 sub - 1, 2 sub it is once the last and once the first shingle with the 'b'
    firsts = sorted(p - 3 for p in facts["odd_at"])
    lasts = sorted(facts["odd_at"])
    for s in (sub - 1, sub, 2 * sub - 1, 2 * sub):
        assert s in firsts and s in lasts
    cfg = orc.default_cfg(**asdict(IngestConfig()))
    sig = orc.minhash_chunks(data, cuts, cfg, np.array(rows["sentinel"] + rows["plain"], np.uint64))
    plain = sig[-1]
    assert (plain == plain[0]).sum() < 128                            # 128 different seeds
    for s in sig[:-1]:
        assert int((s != plain).sum()) >= 16, "a sentinel chunk must depend on its odd shingles in at least 16 of the 128 hashes"
    # dropping any one shingle that holds the 'b' changes the signature: each of the five distinct shingles holds some minimum
    c = facts["parts"][rows["sentinel"][0]]
    p = facts["odd_at"][0]
    five = [c[p - 3 + j: p + 1 + j].tobytes() for j in range(4)] + [b"aaaa"]
    h = np.array([[orc.murmur3(s, seed) for seed in range(128)] for s in five], dtype=np.uint64)
    assert np.array_equal(h.min(axis=0).astype(np.uint32), sig[0])
    assert all((h.argmin(axis=0) == j).sum() >= 8 for j in range(5))


def test_planted_digests_collide_and_wrap(orc):
    dg, facts = E.planted_digests(20000)
    first4 = np.ascontiguousarray(dg[:, :4]).view("<u4").reshape(-1)
    fo, rc = orc.dedup(dg)
    uniq = np.flatnonzero(fo == np.arange(dg.shape[0]))
    same = uniq[first4[uniq] == np.frombuffer(bytes(facts["same_prefix"]), "<u4")[0]]
    assert same.size == 4096 and set(rc[same].tolist()) == {1, 2, 3, 4, 5}          # one home slot, 4096 different digests
    last = uniq[first4[uniq] == 0xFFFFFFFF]
    assert last.size == 4096
    for n in (dg.shape[0], 5000, 1 << 20):
        assert (0xFFFFFFFF & (E.table_slots(n) - 1)) == E.table_slots(n) - 1         # home slot = the last slot for every table size
    # n on both sides of a power of two of the size rule: the mask differs
    for n in (16384, 16385):
        assert n <= dg.shape[0]
    assert E.table_slots(16384) == 32768 and E.table_slots(16385) == 65536


def test_table_size_rule_is_the_library_s():
    import re
    src3, src4 = E._src("l3_dedup.hip"), E._src("l4_lsh.hip")
    for src in (src3, src4):
        assert re.search(r"uint64_t m = 1024;\s*while \(m < 2 \* n\) m <<= 1;", src)
    assert re.search(r"uint32_t slot = hsh & mask;", src3)


@pytest.mark.parametrize("bands,rows", [(4, 32), (8, 16), (16, 8)])
def test_lsh_population_has_equal_keys_over_different_rows(bands, rows, orc):
    from hmse_amd import IngestConfig
    sig = E.lsh_population(E.LSH_N, bands, rows)
    keys, base = orc.lsh(sig, orc.default_cfg(**asdict(IngestConfig(bands=bands, rows=rows))))
    pairs = E.equal_key_different_rows(sig, keys, rows)
    assert sum(pairs) >= 3 and max(pairs) >= 1, pairs
    assert (base >= 0).sum() > 10000                                    # and the planted whole-band copies are found


@pytest.mark.parametrize("spread", [False, True])
def test_hot_bucket_populations(spread, K):
    from hmse_amd import bandtable
    BT_HOT, BT_N = E.BT_HOT, E.BT_N
    P = K["BT_PIECE"]
    assert BT_HOT == [P - 1, P, P + 1, 2 * P, 2 * P + 1]
    nt = K["BT_NT"]
    assert BT_N == [nt - 1, nt, nt + 1, 2 * nt - 1, 2 * nt, 2 * nt + 1, 65535, 65536, 65537]
    for hot in BT_HOT:
        keys, facts = E.hot_bucket_keys(200_000, hot, spread)
        assert int(((keys[:, 1] & 0xFFFF) == facts["bucket"]).sum()) == hot
        ids = facts["hot_ids"]
        tiles = np.unique(ids // nt).size
        assert tiles == (200_000 + nt - 1) // nt if spread else tiles <= hot // nt + 2
        _, tables = bandtable.read_band_tables(bandtable.write_band_tables(keys.view(np.int32), 16))
        bh, start, cnt, got = tables[1]
        k = int(np.flatnonzero(bh == facts["bucket"])[0])
        assert int(cnt[k]) == hot and np.array_equal(got[int(start[k]): int(start[k]) + hot], np.sort(ids))
    # the header count of the hot bucket: a continuation header exactly from P + 1 ids on
    import struct
    for hot, pieces in zip(BT_HOT, (1, 1, 2, 2, 3)):
        keys, _ = E.hot_bucket_keys(200_000, hot, spread)
        one = bandtable.write_band_tables(keys[:, 1:2].view(np.int32), 16)
        nh = struct.unpack_from("<Q", one, 8 + 24)[0]
        hdr = np.frombuffer(one, bandtable.HDR_DTYPE, nh, 8 + 24 + 8)
        assert int((hdr["band_hash"] == 0x1234).sum()) == pieces, (hot, pieces)


@pytest.mark.parametrize("text", [False, True], ids=["random", "text"])
@pytest.mark.parametrize("mib", [1, 2])
def test_dense_cut_piece_has_more_chunks_than_twice_the_expected_count_and_few_candidates(orc, K, mib, text):
    """The facts tests/test_gpu_stream_gl4.py's dense-piece test relies on, from the oracle: a nominal piece of dense_cut_piece() holds more
    chunks than `2 * piece / avg_size + 64` (what a signature row of the captured global-L4 stream held before it was sized like every other
    array of the chain), no more than the chain's worst case `piece / min_size + segments + 2`, every chunk different (all of them are
    stored), and so few cut candidates that the fixed candidate list never overflows (status bit 2 cannot stand in for the row's bit 7).
    The formulas are written out, not read from the library: retune a size and this fails first."""
    from hmse_amd import IngestConfig
    cfg = IngestConfig(seg_size=1 << 20)
    oc = orc.default_cfg(**asdict(cfg))
    G = orc.gear_table()
    ms, ml = orc.cdc_masks(oc)
    pairs = E.dense_pairs(G, ms)
    assert pairs, "no byte pair whose alternating run passes the HARD mask: a cut just behind min_size cannot be forced for the default configuration"
    assert pairs[0] in E.dense_pairs(G, ml)                   # (the hard mask's bits include the easy mask's)
    piece = mib << 20
    data = E.dense_cut_piece(pairs[0], piece, seed=5, text=text)
    assert data.size == piece and np.array_equal(data, E.dense_cut_piece(pairs[0], piece, seed=5, text=text))      # deterministic
    cuts = orc.cdc(data, oc)
    n_chunks = len(cuts) - 1
    segments = piece // cfg.seg_size
    assert n_chunks > 2 * (piece // cfg.avg_size) + 64
    assert n_chunks <= piece // cfg.min_size + segments + 2
    assert int(np.diff(cuts.astype(np.int64)).min()) >= 1 and int(np.median(np.diff(cuts.astype(np.int64)))) == E.DENSE_CUT_FILL + E.DENSE_CUT_RUN
    dg = orc.sha256_chunks(data, cuts)
    assert len(np.unique(dg, axis=0)) == n_chunks
    assert int(E.gear_candidates(data, G, ml).sum()) < E.l2_cand_capacity(piece, cfg, K)
    # the planted near-duplicates: same cut points, every chunk different from its original AND from every other chunk
    twin = E.dense_cut_near_duplicate(data)
    assert np.array_equal(orc.cdc(twin, oc), cuts)
    both = np.concatenate([dg, orc.sha256_chunks(twin, cuts)])
    assert len(np.unique(both, axis=0)) >= 2 * n_chunks - 1    # (the last period may end in front of its flipped byte)
