"""GPU: near-duplicate search over the MinHash/LSH index (hmse_amd.similarity; hmse_l4_index_build / hmse_l4_query) against the
numpy reference of tests/similarity_ref.py, on synthetic signatures (planted bands, a crowded band run, planted key collisions)
and on ingested corpora, stores and sidecars."""
import hashlib
import os
import sys

import numpy as np
import pytest

import similarity_ref as ref

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _planted(rng, n_s, n_q, bands, self_join):
    """Families of near-duplicates: a member copies its family's base, changes each hash with a probability drawn per member, then
    takes 1..bands whole bands back from the base.  Exact copies give ties at 128.  One band run is crowded: in query mode >= 20 k
    stored ids and at most 16 queries share band 0, in self-join mode about 2 k ids."""
    R = 128 // bands
    rnd = lambda n: rng.integers(0, 2**32, (n, 128), dtype=np.uint64).astype(np.uint32)
    base = rnd(max(1, n_s // 20))

    def members(n):
        fam = rng.integers(0, len(base), n)
        out = base[fam].copy()
        p = rng.uniform(0, 0.6, (n, 1))
        flip = rng.random((n, 128)) < p
        out[flip] = rnd(n)[flip]
        for k in range(n):
            for b in rng.choice(bands, rng.integers(1, bands + 1), replace=False):
                out[k, b * R:(b + 1) * R] = base[fam[k], b * R:(b + 1) * R]
        return out

    S = rnd(n_s)
    fam_s = rng.random(n_s) < 0.7
    S[fam_s] = members(int(fam_s.sum()))
    dup = rng.integers(0, n_s, n_s // 50)
    S[rng.integers(0, n_s, dup.size)] = S[dup]
    crowd = rng.choice(n_s, 2000 if self_join else 20000, replace=False)
    X = rnd(1)[0, :R]
    S[crowd, :R] = X
    if self_join:
        return S, S, crowd
    Q = rnd(n_q)
    fam_q = rng.random(n_q) < 0.8
    Q[fam_q] = members(int(fam_q.sum()))
    cp = rng.random(n_q) < 0.05
    Q[cp] = S[rng.integers(0, n_s, int(cp.sum()))]
    Q[rng.choice(n_q, 16, replace=False), :R] = X
    return S, Q, crowd


def _t(a, dev, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("bands", [4, 8, 16])
@pytest.mark.parametrize("self_join", [False, True])
def test_kernel_equals_reference_on_planted_signatures(dev, bands, self_join):
    import torch
    from hmse_amd import IngestConfig, ops
    rng = np.random.default_rng(1000 + bands + 7 * self_join)
    S, Q, crowd = _planted(rng, 50000, 5000, bands, self_join)
    cfg = ops.search_cfg(IngestConfig(), bands)
    sig_s = _t(S.view(np.int32), dev)
    sig_q = _t(Q.view(np.int32), dev)
    keys_s = ops.l4_lsh(sig_s, cfg)[0].cpu().numpy()
    keys_q = ops.l4_lsh(sig_q, cfg)[0].cpu().numpy()
    # planted 32-bit key collisions: chunks whose band rows are unique (outside every family and the crowd) take the key of a
    # crowded or family chunk; equal keys, different rows: no candidate
    R = 128 // bands
    lone = np.setdiff1d(np.arange(len(S)), crowd)[:: 97][:300]
    for j, s in enumerate(lone):
        b = j % bands
        rows = S[:, b * R:(b + 1) * R]
        if (rows == rows[s]).all(1).sum() != 1 or (Q[:, b * R:(b + 1) * R] == rows[s]).all(1).any():
            continue
        keys_s[s, b] = keys_s[crowd[j % len(crowd)], b]
    if self_join:
        keys_q = keys_s
    sk, si = ops.l4_index_build(_t(keys_s, dev))
    pairs = ref.candidate_pairs(S, Q, bands, self_join)
    for top_k in (1, 8, 64):
        for min_score in (0, 64, 120):
            ids, sc, nh, nc = ops.l4_query(sig_q, _t(keys_q, dev), sig_s, sk, si, cfg, top_k, min_score, exclude_self=self_join)
            w_ids, w_sc, w_nh, w_nc = ref.select(*pairs, len(Q), top_k, min_score)
            assert np.array_equal(nc.cpu().numpy(), w_nc), (top_k, min_score)
            assert np.array_equal(nh.cpu().numpy(), w_nh), (top_k, min_score)
            assert np.array_equal(ids.cpu().numpy(), w_ids), (top_k, min_score)
            assert np.array_equal(sc.cpu().numpy(), w_sc), (top_k, min_score)
    nc0 = ref.select(*pairs, len(Q), 1, 0)[3]
    assert nc0.max() >= (1900 if self_join else 20000)          # the crowded run was exercised
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [0, 1, 1000, 70001])
def test_index_build_equals_stable_argsort(dev, n):
    from hmse_amd import ops
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 2**32, (n, 4), dtype=np.uint64).astype(np.uint32)
    if n > 10:
        keys[:, 1] = rng.integers(0, 50, n)                     # many equal keys: stability decides
        keys[:, 2] = 0xFFFFFFFF - rng.integers(0, 3, n)         # the top of the u32 range
    sk, si = ops.l4_index_build(_t(keys.view(np.int32), dev))
    assert sk.shape == (4, n) and si.shape == (4, n)
    for b in range(4):
        o = np.argsort(keys[:, b], kind="stable")
        assert np.array_equal(si[b].cpu().numpy(), o)
        assert np.array_equal(sk[b].cpu().numpy().view(np.uint32), keys[o, b])


def _corpus():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import variants_dataset
    from hmse_amd import corpus
    return np.concatenate([variants_dataset(corpus.wiki_synth(3 << 20, seed=42)), corpus.wiki_synth(2 << 20, seed=42)])


@pytest.fixture(scope="module")
def ingested(dev):
    import torch
    from hmse_amd import IngestConfig, ingest
    cfg = IngestConfig(seg_size=1 << 20)
    data = _corpus()
    res = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    return cfg, data, res


def _same(h, w):
    ids, sc, nh, nc = w
    assert np.array_equal(h.n_candidates.cpu().numpy(), nc)
    assert np.array_equal(h.n_hits.cpu().numpy(), nh)
    assert np.array_equal(h.ids.cpu().numpy(), ids)
    assert np.array_equal(h.scores.cpu().numpy(), sc)


def test_self_join_agrees_with_the_ingest_base_rule(ingested):
    from hmse_amd import similarity
    cfg, data, res = ingested
    ix = similarity.SimilarityIndex.from_result(res, cfg)
    d = ix.near_duplicates(top_k=64)
    S = res.sig.cpu().numpy().view(np.uint32)
    _same(d, ref.search(S, S, cfg.bands, 64, self_join=True))
    base = res.base.cpu().numpy()
    ids, nh, nc = d.ids.cpu().numpy(), d.n_hits.cpu().numpy(), d.n_candidates.cpu().numpy()
    checked = 0
    for i in range(len(S)):
        if nc[i] > 64:
            continue
        earlier = [c for c in ids[i, :nh[i]] if c < i]
        assert base[i] == (min(earlier) if earlier else -1), i
        checked += 1
    assert checked > 0.9 * len(S) and (base >= 0).sum() > 20


def test_query_by_bytes(ingested, dev, orc):
    import torch
    from dataclasses import asdict
    from hmse_amd import similarity
    cfg, data, res = ingested
    ix = similarity.SimilarityIndex.from_result(res, cfg)
    S = res.sig.cpu().numpy().view(np.uint32)
    # the query's signatures are the oracle's: cdc cuts, then MinHash of every chunk
    q = data[(2 * MIB) + 12345: (4 * MIB) + 999].copy()
    oc = orc.default_cfg(**asdict(cfg))
    cuts, sig = ix.query_signatures(torch.from_numpy(q).to(dev))
    o_cuts = orc.cdc(q, oc)
    assert np.array_equal(cuts.cpu().numpy().astype(np.uint64), o_cuts)
    assert np.array_equal(sig.cpu().numpy().view(np.uint32), orc.minhash_chunks(q, o_cuts, oc))
    # a segment-aligned copy of stored bytes: every chunk's twin (equal signature) first, at 128, the smallest such id
    seg = data[MIB: 3 * MIB]
    h = ix.query(torch.from_numpy(seg).to(dev), top_k=8)
    _, sq = ix.query_signatures(torch.from_numpy(seg).to(dev))
    sq = sq.cpu().numpy().view(np.uint32)
    for j in range(len(sq)):
        twin = np.nonzero((S == sq[j]).all(1))[0]
        assert len(twin) and h.ids[j, 0].item() == twin.min() and h.scores[j, 0].item() == 128
    # an edited copy (about 0.5 % of its bytes): the reference
    ed = data[: 3 * MIB].copy()
    pos = np.random.default_rng(5).integers(0, ed.size, ed.size // 200)
    ed[pos] = np.random.default_rng(6).integers(97, 123, pos.size, dtype=np.uint8)
    h = ix.query(torch.from_numpy(ed).to(dev), top_k=8, min_score=10)
    _, sq = ix.query_signatures(torch.from_numpy(ed).to(dev))
    _same(h, ref.search(S, sq.cpu().numpy().view(np.uint32), cfg.bands, 8, 10))
    assert (h.n_hits > 0).float().mean().item() > 0.1      # 4 x 32 bands: a band survives with probability s^32 (the S-curve)


def _all_equal(a, b):
    for f in ("ids", "scores", "n_hits", "n_candidates"):
        assert np.array_equal(getattr(a, f).cpu().numpy(), getattr(b, f).cpu().numpy()), f


def test_stores_sidecars_and_locate(ingested, dev):
    import torch
    from hmse_amd import bandtable, ingest, manifest, ops, similarity
    cfg, data, res = ingested
    m = manifest.Manifest.from_bytes(manifest.build_manifest(res).to_bytes())
    side = bandtable.write_band_tables_device(res.band_keys, cfg.band_bits, signatures=res.sig)
    srcs = [similarity.SimilarityIndex.from_store(m, cfg, dev, band_tables=side), similarity.SimilarityIndex.from_store(m, cfg, dev),
            similarity.SimilarityIndex.from_result(res, cfg)]
    q = torch.from_numpy(data[MIB // 2: 2 * MIB]).to(dev)
    outs = [(ix.near_duplicates(top_k=16), ix.query(q, top_k=4, min_score=30)) for ix in srcs]
    for o in outs[1:]:
        _all_equal(o[0], outs[0][0]); _all_equal(o[1], outs[0][1])
    ids = torch.arange(srcs[0].n, device=dev)
    locs = [ix.locate(ids) for ix in srcs]
    for lc in locs[1:]:
        assert all(torch.equal(getattr(lc, f), getattr(locs[0], f)) for f in ("ptr", "offsets", "lengths"))
    # refused sidecars: another banding, truncated
    k16 = ops.l4_lsh(res.sig, cfg.with_(bands=16, rows=8))[0]
    with pytest.raises(ValueError):
        similarity.SimilarityIndex.from_store(m, cfg, dev, band_tables=bandtable.write_band_tables_device(k16, cfg.band_bits, signatures=res.sig))
    with pytest.raises(ValueError):
        similarity.SimilarityIndex.from_store(m, cfg, dev, band_tables=side[: len(side) - 1000])
    with pytest.raises(ValueError):
        similarity.SimilarityIndex.from_store(m, cfg, dev, band_tables=bandtable.write_band_tables_device(res.band_keys, cfg.band_bits))
    # a 2-shard store with two sidecars: locate() names refcount offsets per id, and their bytes hash to the id's digest
    parts = [data[: 3 * MIB], data[3 * MIB:]]
    rs = ingest.ingest_shards_local([torch.from_numpy(p).to(dev) for p in parts], cfg)
    st = manifest.Store.from_bytes(manifest.merge_manifests([manifest.build_manifest(r, i, 2) for i, r in enumerate(rs)]).to_bytes())
    sides = [bandtable.write_band_tables_device(r.band_keys, cfg.band_bits, signatures=r.sig) for r in rs]
    ix = similarity.SimilarityIndex.from_store(st, cfg, dev, band_tables=sides)
    assert ix.n == sum(len(s.index) for s in st.shards)
    idx = np.concatenate([s.index for s in st.shards])
    loc = ix.locate(torch.arange(ix.n, device=dev))
    ptr, off, ln = loc.ptr.cpu().numpy(), loc.offsets.cpu().numpy(), loc.lengths.cpu().numpy()
    assert np.array_equal(np.diff(ptr), idx["refcount"].astype(np.int64))
    for g in range(ix.n):
        for o in off[ptr[g]: ptr[g + 1]]:
            assert hashlib.sha256(data[o: o + ln[g]].tobytes()).digest() == idx["sha256"][g].tobytes()
    _all_equal(ix.near_duplicates(top_k=8), similarity.SimilarityIndex.from_store(st, cfg, dev).near_duplicates(top_k=8))
    # refused stores: an unmerged part, a multi-rank stream's part
    with pytest.raises(ValueError, match="merge_manifests"):
        similarity.SimilarityIndex.from_store(manifest.build_manifest(rs[1], 1, 2), cfg, dev)
    p = manifest.Manifest.from_bytes(m.to_bytes())
    p.pieces = np.zeros(1, manifest.PIECE_DTYPE)
    with pytest.raises(ValueError, match="pieces"):
        similarity.SimilarityIndex.from_store(p, cfg, dev)
    with pytest.raises(ValueError, match="pieces"):
        similarity.SimilarityIndex.from_store(manifest.Store([p]), cfg, dev)


def test_rebanding_a_4x32_store_at_16x8(ingested):
    from hmse_amd import similarity
    cfg, data, res = ingested
    S = res.sig.cpu().numpy().view(np.uint32)
    d4 = similarity.SimilarityIndex.from_result(res, cfg).near_duplicates(top_k=64)
    d16 = similarity.SimilarityIndex.from_result(res, cfg, bands=16).near_duplicates(top_k=64)
    _same(d16, ref.search(S, S, 16, 64, self_join=True))
    nc4, nc16 = d4.n_candidates.cpu().numpy(), d16.n_candidates.cpu().numpy()
    assert (nc16 >= nc4).all() and (nc16 > nc4).any()
    i4, i16 = d4.ids.cpu().numpy(), d16.ids.cpu().numpy()
    for i in np.nonzero(nc16 <= 64)[0]:
        assert set(i4[i][i4[i] >= 0]) <= set(i16[i][i16[i] >= 0])


def test_edges(ingested, dev):
    import torch
    from hmse_amd import similarity
    cfg, data, res = ingested
    empty = similarity.SimilarityIndex(torch.zeros((0, 128), dtype=torch.int32, device=dev), cfg)
    h = empty.query(torch.from_numpy(data[:100000]).to(dev), top_k=5)
    assert h.ids.shape[1] == 5 and (h.ids == -1).all() and (h.n_hits == 0).all() and (h.n_candidates == 0).all()
    assert empty.near_duplicates().ids.shape == (0, 8)
    ix = similarity.SimilarityIndex.from_result(res, cfg)
    h = ix.query(torch.zeros(0, dtype=torch.uint8, device=dev))
    assert h.ids.shape == (0, 8) and h.cuts.tolist() == [0]
    S = res.sig.cpu().numpy().view(np.uint32)
    for tiny in (b"ab", b"abc"):
        t = torch.frombuffer(bytearray(tiny), dtype=torch.uint8).to(dev)
        h = ix.query(t, top_k=3)
        _, sq = ix.query_signatures(t)
        assert h.cuts.tolist() == [0, len(tiny)]
        _same(h, ref.search(S, sq.cpu().numpy().view(np.uint32), cfg.bands, 3))
