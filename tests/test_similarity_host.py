"""CPU: the near-duplicate search's numpy reference on hand-built signatures, the C-ABI's workspace sizes and argument checks
(all before any launch, so they hold without a GPU), and that hmse_amd.similarity refuses host tensors."""
import ctypes as C

import numpy as np
import pytest

import similarity_ref as ref


def _sig(n, seed):
    return np.random.default_rng(seed).integers(0, 2**32, (n, 128), dtype=np.uint64).astype(np.uint32)


def test_reference_counts_a_candidate_equal_in_several_bands_once():
    S = _sig(4, 1)
    Q = S[[0]].copy()
    Q[0, 100:] ^= 1                                            # bands 0..2 of 4 equal to S[0], band 3 not
    S[2, :32] = Q[0, :32]                                      # S[2] shares band 0 only
    qi, c, score = ref.candidate_pairs(S, Q, 4)
    assert list(c) == [0, 2] and list(qi) == [0, 0]
    assert list(score) == [100, 32]
    ids, sc, nh, nc = ref.select(qi, c, score, 1, 8, 0)
    assert list(ids[0, :3]) == [0, 2, -1] and list(sc[0, :3]) == [100, 32, 0] and nh[0] == 2 and nc[0] == 2


def test_reference_ties_min_score_top_k_and_self_exclusion():
    S = _sig(6, 2)
    S[3] = S[1]; S[5] = S[1]                                   # three equal signatures: ties at 128 go by id
    S[4, :32] = S[1, :32]                                      # one band shared: score 32
    ids, sc, nh, nc = ref.search(S, S[[1]], 4, 8)
    assert list(ids[0, :5]) == [1, 3, 5, 4, -1] and list(sc[0, :4]) == [128, 128, 128, 32]
    assert nh[0] == 4 and nc[0] == 4
    ids, sc, nh, nc = ref.search(S, S[[1]], 4, 2)               # top_k truncates, n_candidates does not
    assert list(ids[0]) == [1, 3] and nh[0] == 2 and nc[0] == 4
    ids, sc, nh, nc = ref.search(S, S[[1]], 4, 8, min_score=33)  # min_score drops the 32, not the count
    assert list(ids[0, :4]) == [1, 3, 5, -1] and nh[0] == 3 and nc[0] == 4
    ids, sc, nh, nc = ref.search(S, S, 4, 8, self_join=True)    # c != i
    assert list(ids[1, :4]) == [3, 5, 4, -1] and nc[1] == 3 and nc[0] == 0 and nh[0] == 0 and ids[0, 0] == -1
    ids16, _, _, nc16 = ref.search(S, S, 16, 8, self_join=True)  # finer bands: a superset of candidates
    assert (nc16 >= nc).all()


def _lib_cfg(bands=4):
    from hmse_amd import IngestConfig, _lib
    return _lib.hip_lib(), IngestConfig().with_(bands=bands, rows=128 // bands).to_c()


def test_workspace_sizes():
    L, c = _lib_cfg()
    for n in (0, 1, 255, 257, 100000):
        idx = L.hmse_workspace_bytes(26, n, C.byref(c))
        qry = L.hmse_workspace_bytes(27, n, C.byref(c))
        assert idx >= 8 * n and qry >= 8 * n * 4
    L16, c16 = _lib_cfg(16)
    assert L16.hmse_workspace_bytes(27, 1000, C.byref(c16)) > L.hmse_workspace_bytes(27, 1000, C.byref(c))
    bad = _lib_cfg(4)[1]
    bad.rows = 16                                               # 4 x 16 != 128: no size
    assert L.hmse_workspace_bytes(27, 1000, C.byref(bad)) == 0


FAKE = 1 << 40       # never dereferenced: every call below is refused before any launch


def _query(L, c, n_q=10, n_s=10, top_k=8, min_score=0, flags=0, **null):
    p = {k: (None if k in null else FAKE) for k in ("sig_q", "keys_q", "sig_s", "sk", "si", "ids", "sc", "nh", "nc", "st", "ws")}
    return L.hmse_l4_query(p["sig_q"], p["keys_q"], n_q, p["sig_s"], n_s, p["sk"], p["si"], C.byref(c), top_k, min_score, flags,
                           p["ids"], p["sc"], p["nh"], p["nc"], p["st"], p["ws"], 1 << 30, None)


def test_query_refuses_bad_arguments_before_any_launch():
    L, c = _lib_cfg()
    EINVAL = -1
    assert _query(L, c, top_k=0) == EINVAL and _query(L, c, top_k=65) == EINVAL
    assert _query(L, c, min_score=129) == EINVAL
    assert _query(L, c, flags=2) == EINVAL
    assert _query(L, c, n_q=1 << 32) == EINVAL and _query(L, c, n_s=1 << 32) == EINVAL
    for name in ("sig_q", "keys_q", "sig_s", "sk", "si", "ids", "sc", "nh", "nc", "st"):
        assert _query(L, c, **{name: True}) == EINVAL, name
    for bands, rows in ((3, 42), (32, 4), (4, 16), (0, 128)):
        bad = _lib_cfg()[1]
        bad.bands, bad.rows = bands, rows
        assert _query(L, bad) == EINVAL, (bands, rows)


def test_index_build_refuses_bad_arguments_before_any_launch():
    L, _ = _lib_cfg()
    call = lambda keys=FAKE, n=10, bands=4, sk=FAKE, si=FAKE, st=FAKE: L.hmse_l4_index_build(keys, n, bands, sk, si, st, FAKE, 1 << 30, None)
    for bands in (0, 3, 32):
        assert call(bands=bands) == -1
    assert call(n=1 << 32) == -1
    assert call(keys=None) == -1 and call(sk=None) == -1 and call(si=None) == -1 and call(st=None) == -1


def test_similarity_refuses_host_tensors():
    import torch
    from hmse_amd import IngestConfig, ops, similarity
    with pytest.raises(ops.HmseError, match="HBM"):
        similarity.SimilarityIndex(torch.zeros((4, 128), dtype=torch.int32), IngestConfig())
    with pytest.raises(ops.HmseError, match="HBM"):
        ops.l4_index_build(torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.search_cfg(IngestConfig(), 3)


def test_exported_symbols_include_the_search():
    from hmse_amd import _lib
    assert {"hmse_l4_index_build", "hmse_l4_query"} <= set(_lib.EXPORTED_SYMBOLS)
