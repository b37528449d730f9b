"""The oracle of the approximate search (include/hmse.h hmse_approx_*; hmse_amd/find.py find_approx) in plain Python: Sellers' dynamic
programme, one column per text byte, no bit tricks.

  * ed(a, b): Levenshtein's distance — insertion, deletion and substitution cost 1 each;
  * d(e) = min over 0 <= s <= e of ed(pat, C[s:e]) for an end 1 <= e <= N: the last value of the column D[i][e] with D[0][e] = 0,
    D[i][0] = i, D[i][e] = min(D[i-1][e-1] + (pat[i-1] != C[e-1]), D[i-1][e] + 1, D[i][e-1] + 1);
  * e is an occurrence iff d(e) <= k; it is reported as (e - 1, d(e)): the match's LAST byte and its errors;
  * ignore_case folds A-Z to a-z on both sides: bytes.lower() (bytes >= 0x80 stay);
  * partition: the end e of chunk c (byte e - 1 lies in it) is a scan end iff e - cuts[c] >= W = m + k, a seam end otherwise;
  * span: the largest s with ed(pat, C[s:e]) == d(e).
"""
import bisect


def fold(b: bytes, ic: bool) -> bytes:
    return bytes(b).lower() if ic else bytes(b)


def ed(a: bytes, b: bytes) -> int:
    col = list(range(len(a) + 1))
    for ch in b:
        new = [col[0] + 1]
        for i in range(1, len(a) + 1):
            new.append(min(col[i - 1] + (a[i - 1] != ch), col[i] + 1, new[i - 1] + 1))
        col = new
    return col[-1]


def distances(pat: bytes, text: bytes, col=None):
    """-> [d(e) for e = 1 .. len(text)].  `col`: the column to start from (None: D[i] = i, the column in front of the text's first byte)."""
    m = len(pat)
    col = list(range(m + 1)) if col is None else list(col)
    out = []
    for ch in text:
        new = [0]
        for i in range(1, m + 1):
            new.append(min(col[i - 1] + (pat[i - 1] != ch), col[i] + 1, new[i - 1] + 1))
        col = new
        out.append(col[m])
    return out


def find(corpus: bytes, pat: bytes, k: int, ic: bool = False):
    """-> [(offset of the last byte, errors)] of every occurrence, ascending."""
    return [(e, d) for e, d in enumerate(distances(fold(pat, ic), fold(corpus, ic))) if d <= k]


def _column_step(col, neq, first):
    """One text byte for many columns at once (numpy, rows = independent texts): the same recurrence; the chain new[i-1] + 1 along a
    column is a running minimum of new[j] - j."""
    import numpy as np
    m = col.shape[1] - 1
    ar = np.arange(m + 1, dtype=col.dtype)
    t = np.empty_like(col)
    t[:, 0] = first
    np.minimum(col[:, :-1] + neq, col[:, 1:] + 1, out=t[:, 1:])
    return np.minimum.accumulate(t - ar, axis=1) + ar


def find_np(corpus: bytes, pat: bytes, k: int, ic: bool = False, block: int = 1024):
    """find() for long texts: the corpus in blocks of `block` bytes, all blocks stepped side by side, each from a fresh column W = m + k
    bytes in front of it (at the corpus's first byte the fresh column is the true one).  By the window fact — which
    tests/test_approx_host.py checks against find() — the values <= k are the true ones and the others stay above k."""
    import numpy as np
    p, c = np.frombuffer(fold(pat, ic), np.uint8), np.frombuffer(fold(corpus, ic), np.uint8)
    m, n, W = len(p), len(c), len(p) + k
    if n == 0:
        return []
    base = np.arange(0, n, block, dtype=np.int64)
    fresh = np.broadcast_to(np.arange(m + 1, dtype=np.int16), (base.size, m + 1))
    col = fresh.copy()
    offs, errs = [], []
    for step in range(block + W):
        idx = base - W + step
        ch = c[np.clip(idx, 0, n - 1)]
        col = _column_step(col, (p[None, :] != ch[:, None]).astype(np.int16), 0)
        col[idx < 0] = fresh[0]                                                     # in front of the corpus: still the fresh column
        if step >= W:
            hit = (col[:, m] <= k) & (idx < n)
            offs.append(idx[hit])
            errs.append(col[hit, m])
    o, d = np.concatenate(offs), np.concatenate(errs)
    order = np.argsort(o, kind="stable")
    return list(zip(o[order].tolist(), d[order].astype(np.int64).tolist()))


def spans_np(corpus: bytes, pat: bytes, occ, ic: bool = False):
    """span() for many occurrences [(o, d)] of one pattern at once -> [start] (o + 1 where span() gives None): the anchored columns
    (D[0][t] = t) of the reversed pattern over C[o], C[o - 1], ..., all occurrences stepped side by side."""
    import numpy as np
    if not occ:
        return []
    p, c = np.frombuffer(fold(pat, ic), np.uint8)[::-1], np.frombuffer(fold(corpus, ic), np.uint8)
    m = len(p)
    o, d = np.array([x for x, _ in occ], np.int64), np.array([x for _, x in occ], np.int64)
    col = np.broadcast_to(np.arange(m + 1, dtype=np.int16), (o.size, m + 1)).copy()
    start = o + 1
    open_ = np.ones(o.size, bool)
    for s in range(m + int(d.max())):
        q = o - s
        live = open_ & (q >= 0) & (s < m + d)
        ch = c[np.clip(q, 0, len(c) - 1)]
        col = _column_step(col, (p[None, :] != ch[:, None]).astype(np.int16), s + 1)
        got = live & (col[:, m] == d)
        start[got] = q[got]
        open_ &= ~got
    return start.tolist()


def scan_hits(raw: bytes, raw_off, pats, ks, mult=None, ic: bool = False):
    """The scan's contract -> (sorted hit words position << 8 | errors << 3 | pattern, counts per pattern weighted by mult): the ends of
    every record with W bytes of the record in front of them, records looked at on their own."""
    words, counts = [], [0] * len(pats)
    for r in range(len(raw_off) - 1):
        rec = raw[raw_off[r]: raw_off[r + 1]]
        for j, (p, k) in enumerate(zip(pats, ks)):
            for o, d in (find_np if len(rec) > 2048 else find)(rec, p, k, ic):
                if o + 1 >= len(p) + k:
                    words.append(((raw_off[r] + o) << 8) | (d << 3) | j)
                    counts[j] += 1 if mult is None else mult[r]
    return sorted(words), counts


def split(occ, W: int, cuts):
    """occ = find(...) over the corpus that `cuts` divides -> (scan ends, seam ends)."""
    scan, seam = [], []
    for o, d in occ:
        c = bisect.bisect_right(cuts, o) - 1                                       # the chunk of byte o (empty chunks hold nothing)
        (scan if o + 1 - cuts[c] >= W else seam).append((o, d))
    return scan, seam


def span(corpus: bytes, pat: bytes, o: int, d: int, ic: bool = False):
    """The start of the occurrence whose last byte is o and whose errors are d: the largest s with ed(pat, C[s:o+1]) == d, looked for
    among texts of at most len(pat) + d bytes; None if no such text attains d."""
    p, c = fold(pat, ic), fold(corpus, ic)
    for s in range(o, max(o + 1 - (len(p) + d), 0) - 1, -1):
        if ed(p, c[s: o + 1]) == d:
            return s
    return None


def best_ends(occ):
    """occ ascending -> of every run of consecutive offsets the entry with the fewest errors, the leftmost on ties."""
    out, run = [], []
    for o, d in occ:
        if run and o != run[-1][0] + 1:
            out.append(min(run, key=lambda x: (x[1], x[0])))
            run = []
        run.append((o, d))
    if run:
        out.append(min(run, key=lambda x: (x[1], x[0])))
    return out


def noisy(rng, pat: bytes, edits: int, alphabet: bytes) -> bytes:
    """pat after `edits` random edits (substitution, insertion or deletion at random places)."""
    b = bytearray(pat)
    for _ in range(edits):
        op = int(rng.integers(0, 3))
        if op == 0 and b:
            b[int(rng.integers(0, len(b)))] = alphabet[int(rng.integers(0, len(alphabet)))]
        elif op == 1:
            b.insert(int(rng.integers(0, len(b) + 1)), alphabet[int(rng.integers(0, len(alphabet)))])
        elif b:
            del b[int(rng.integers(0, len(b)))]
    return bytes(b)


def plant(rng, corpus: bytearray, pats, ks, alphabet: bytes, copies: int = 3):
    """Writes `copies` noisy copies of every pattern (0 .. k + 1 edits each, the first one with none) into corpus, each at a seeded
    place of a slot of its own (no copy damages another).  Every pattern must fit its slot: then each has an occurrence."""
    size = len(corpus) // max(len(pats) * copies, 1)
    assert all(len(p) <= size for p in pats), "the corpus is too small for the copies"
    for j, (p, k) in enumerate(zip(pats, ks)):
        for c in range(copies):
            s = noisy(rng, p, 0 if c == 0 else int(rng.integers(0, k + 2)), alphabet)[:size]
            o = (j * copies + c) * size + int(rng.integers(0, size - len(s) + 1))
            corpus[o: o + len(s)] = s
    return corpus
