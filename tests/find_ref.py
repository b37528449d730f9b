"""Plain-Python reference of hmse_amd.find (exact byte-pattern search), on the INPUT bytes — independent of any store.

  * an occurrence of pattern p in corpus C is any offset o with C[o : o + len(p)] == p; overlapping occurrences all count
    (b"aa" occurs 3 times in b"aaaa"): a bytes.find loop that restarts at o + 1;
  * ignore_case: bytes.lower() on both sides (ASCII A-Z -> a-z, every other value, >= 0x80 included, as it is);
  * the partition rule: chunk k covers [cuts[k], cuts[k + 1]); an occurrence (o, m) starts in exactly one chunk k and is an IN-RECORD
    hit iff o + m <= cuts[k + 1], otherwise a SEAM hit of chunk k (then o >= cuts[k + 1] - (m - 1)); a seam hit may run over any
    number of following chunks and belongs to the chunk it starts in only.
"""
import bisect


def occurrences(corpus: bytes, pattern: bytes, ignore_case: bool = False) -> list:
    """All offsets of `pattern` in `corpus`, ascending."""
    corpus, pattern = bytes(corpus), bytes(pattern)
    assert len(pattern) >= 1
    if ignore_case:
        corpus, pattern = corpus.lower(), pattern.lower()
    out, start = [], 0
    while True:
        o = corpus.find(pattern, start)
        if o < 0:
            return out
        out.append(o)
        start = o + 1


def find(corpus: bytes, patterns, ignore_case: bool = False):
    """-> (counts [P], ptr [P + 1], offsets [ptr[P]]): the shape of hmse_amd.find.Found as Python lists."""
    counts, ptr, offsets = [], [0], []
    for p in patterns:
        occ = occurrences(corpus, p, ignore_case)
        counts.append(len(occ))
        offsets.extend(occ)
        ptr.append(len(offsets))
    return counts, ptr, offsets


def chunk_of(cuts, o: int) -> int:
    """The chunk an offset starts in: the k with cuts[k] <= o < cuts[k + 1] (zero-length chunks hold no offset)."""
    k = bisect.bisect_right(cuts, o) - 1
    assert cuts[k] <= o < cuts[k + 1]
    return k


def split(corpus: bytes, patterns, cuts, ignore_case: bool = False):
    """The partition rule -> (in_record, seam): two sorted lists of (offset, pattern index)."""
    cuts = [int(c) for c in cuts]
    in_record, seam = [], []
    for j, p in enumerate(patterns):
        for o in occurrences(corpus, p, ignore_case):
            k = chunk_of(cuts, o)
            if o + len(p) <= cuts[k + 1]:
                in_record.append((o, j))
            else:
                assert o >= max(cuts[k], cuts[k + 1] - (len(p) - 1))
                seam.append((o, j))
    return sorted(in_record), sorted(seam)


def scan_hits(raw: bytes, raw_off, patterns, ignore_case: bool = False, mult=None):
    """What hmse_find_scan finds: matches lying wholly inside one record [raw_off[r], raw_off[r + 1]) of `raw`.
    -> (sorted list of (position in raw, pattern index), counts [P] weighted by mult[record] (None: 1 each))."""
    raw = bytes(raw)
    hits, counts = [], [0] * len(patterns)
    for r in range(len(raw_off) - 1):
        a, b = int(raw_off[r]), int(raw_off[r + 1])
        for j, p in enumerate(patterns):
            for o in occurrences(raw[a:b], p, ignore_case):
                hits.append((a + o, j))
                counts[j] += 1 if mult is None else int(mult[r])
    return sorted(hits), counts
