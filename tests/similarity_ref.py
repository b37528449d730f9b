"""numpy reference of the near-duplicate search (hmse_amd/similarity.py), written without the GPU's algorithm: no band keys, no
sorted runs.  Stored chunks are grouped by the BYTES of each band (np.unique over the band rows), candidate pairs are formed from
those groups, only those pairs are scored, then ordered and truncated.  Key collisions cannot make a candidate by construction."""
import numpy as np


def _band_groups(rows: np.ndarray):
    """-> group label of every row (equal rows, equal label)."""
    v = np.ascontiguousarray(rows).view(np.dtype((np.void, rows.shape[1] * rows.itemsize))).ravel()
    _, inv = np.unique(v, return_inverse=True)
    return inv.ravel()


def candidate_pairs(S: np.ndarray, Q: np.ndarray, bands: int, self_join: bool = False):
    """-> (query index, stored id, score) of every candidate pair, each pair once, sorted by (query, id)."""
    S = np.ascontiguousarray(S).view(np.uint32)
    Q = np.ascontiguousarray(Q).view(np.uint32)
    n, q, R = len(S), len(Q), 128 // bands
    keys = []
    for b in range(bands):
        if n == 0 or q == 0:
            break
        lab = _band_groups(np.concatenate([S[:, b * R:(b + 1) * R], Q[:, b * R:(b + 1) * R]]))
        ls, lq = lab[:n], lab[n:]
        order = np.argsort(ls, kind="stable")                 # stored ids grouped by band content
        cnt = np.bincount(ls, minlength=lab.max() + 1)
        start = np.cumsum(cnt) - cnt
        per_q = cnt[lq]
        tot = int(per_q.sum())
        if tot == 0:
            continue
        qi = np.repeat(np.arange(q, dtype=np.int64), per_q)
        pos = np.repeat(start[lq] - (np.cumsum(per_q) - per_q), per_q) + np.arange(tot)
        keys.append(qi * n + order[pos])
    if not keys:
        z = np.zeros(0, np.int64)
        return z, z, z.astype(np.int32)
    k = np.unique(np.concatenate(keys))
    qi, c = k // n, k % n
    if self_join:
        keep = qi != c
        qi, c = qi[keep], c[keep]
    score = np.zeros(len(qi), np.int32)
    for a in range(0, len(qi), 1 << 18):                       # scored in blocks: a crowded band makes many pairs
        score[a:a + (1 << 18)] = (Q[qi[a:a + (1 << 18)]] == S[c[a:a + (1 << 18)]]).sum(1)
    return qi, c, score


def select(qi, c, score, q: int, top_k: int, min_score: int):
    """Candidate pairs -> (ids int64 [q, top_k] (-1 pad), scores int32 [q, top_k] (0 pad), n_hits [q], n_candidates [q])."""
    n_cand = np.bincount(qi, minlength=q).astype(np.int64)
    keep = score >= min_score
    qi, c, score = qi[keep], c[keep], score[keep]
    o = np.lexsort((c, -score.astype(np.int64), qi))          # by query, score descending, id ascending
    qi, c, score = qi[o], c[o], score[o]
    first = np.searchsorted(qi, np.arange(q))
    rank = np.arange(len(qi)) - first[qi] if len(qi) else np.zeros(0, np.int64)
    t = rank < top_k
    ids = np.full((q, top_k), -1, np.int64)
    sc = np.zeros((q, top_k), np.int32)
    ids[qi[t], rank[t]] = c[t]
    sc[qi[t], rank[t]] = score[t]
    n_hits = np.minimum(np.bincount(qi, minlength=q), top_k).astype(np.int64)
    return ids, sc, n_hits, n_cand


def search(S, Q, bands: int, top_k: int, min_score: int = 0, self_join: bool = False):
    qi, c, score = candidate_pairs(S, Q, bands, self_join)
    return select(qi, c, score, len(Q), top_k, min_score)
