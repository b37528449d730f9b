"""Plain-Python restatement of the regex search's definitions (hmse_amd/regex.py, include/hmse.h hmse_regex_*), with the standard `re`
module as the oracle.  Independent of hmse_amd.regex apart from taking `reach` as a number.

C is the corpus, r a pattern (bytes), R = reach (1..256).  Start o is an occurrence iff some l with 1 <= l <= min(R, N - o) has
C[o : o + l] in L(r); its length is the largest such l.  Empty matches are never reported; every start counts."""
import re


def compiled(pattern: bytes, ignore_case: bool = False, dotall: bool = False):
    return re.compile(b"(?:" + pattern + b")", (re.IGNORECASE if ignore_case else 0) | (re.DOTALL if dotall else 0))


def length_at(rx, corpus: bytes, o: int, reach: int, n: int | None = None) -> int:
    """The oracle for one start: rx.match(C, o, e) with e = min(N, o + R) decides whether any prefix matches; if so the largest l in
    e - o down to 1 with rx.fullmatch(C, o, o + l) is the length (0: no occurrence; an empty match is none)."""
    e = min(len(corpus) if n is None else n, o + reach)
    if rx.match(corpus, o, e) is None:
        return 0
    full = rx.fullmatch
    for l in range(e - o, 0, -1):
        if full(corpus, o, o + l) is not None:
            return l
    return 0


class Longest:
    """length_at without its e - o fullmatch calls per occurrence, by `re` alone.  With the window's end at e, the pattern
    (?:r)(?!(?s:.{T + 1})) matches at o iff some match of r from o leaves at most T bytes of the window, that is iff some
    C[o : o + l] in L(r) has l >= (e - o) - T.  That predicate falls monotonically as the demanded l grows, so the largest l for
    which it holds — which is length_at's answer — is found by galloping up from the end of re's own (leftmost-priority) match and
    halving.  tests/test_regex_host.py checks it against length_at itself on a sample of every sixteenth pattern's starts."""

    def __init__(self, pattern: bytes, ignore_case: bool = False, dotall: bool = False):
        self.flags = (re.IGNORECASE if ignore_case else 0) | (re.DOTALL if dotall else 0)
        self.pattern, self.rx, self.tails = pattern, compiled(pattern, ignore_case, dotall), {}

    def at_least(self, corpus: bytes, o: int, e: int, l: int) -> bool:
        t = (e - o) - l
        rx = self.tails.get(t)
        if rx is None:
            rx = self.tails[t] = re.compile(b"(?:" + self.pattern + b")(?!(?s:.{%d}))" % (t + 1), self.flags)
        return rx.match(corpus, o, e) is not None

    def length_at(self, corpus: bytes, o: int, reach: int, n: int | None = None) -> int:
        e = min(len(corpus) if n is None else n, o + reach)
        m = self.rx.match(corpus, o, e)
        if m is None:
            return 0
        lo, step = m.end() - o, 1                                    # some match of lo bytes exists (lo may be 0: the empty one)
        while lo + step <= e - o and self.at_least(corpus, o, e, lo + step):
            lo, step = lo + step, 2 * step
        hi = min(lo + step, e - o + 1)                               # no match of hi bytes or more
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if self.at_least(corpus, o, e, mid):
                lo = mid
            else:
                hi = mid
        return lo


def find(corpus: bytes, pattern: bytes, reach: int, ignore_case: bool = False, dotall: bool = False, n: int | None = None, start: int = 0):
    """-> [(o, length)] ascending: every occurrence with start <= o < n.  Only the starts at which (?=(?:r)) matches are asked: an
    occurrence at o is a match of r at o that ends within 256 bytes, so none is lost (the lookahead knows neither the exact window nor
    that empty matches do not count — the oracle then decides).  The lookahead is run block by block with 256 bytes of overhang, so
    that a long run of one byte does not make it quadratic."""
    lg = Longest(pattern, ignore_case, dotall)
    n = len(corpus) if n is None else n
    ahead = re.compile(b"(?=(?:" + pattern + b"))", lg.flags)
    out = []
    for s in range(start, n, 512):
        for m in ahead.finditer(corpus, s, min(s + 512 + 256, n)):
            if m.start() >= s + 512:
                break
            l = lg.length_at(corpus, m.start(), reach, n)
            if l:
                out.append((m.start(), l))
    return out


def split(corpus: bytes, found, reach: int, cuts):
    """The partition rule: `found` = find(...) of the corpus, cuts the chunk boundaries (ascending, cuts[0] = 0, cuts[-1] = N; equal
    neighbours are empty chunks).  Start o in chunk k is a SEAM start iff cuts[k + 1] - o < reach, else a SCAN start (its answer then
    depends on the chunk's bytes only).  -> (scan [(o, length)], seam [(o, length)]), both ascending."""
    scan, seam = [], []
    k = 0
    for o, l in found:
        while cuts[k + 1] <= o:
            k += 1
        (seam if cuts[k + 1] - o < reach else scan).append((o, l))
    return scan, seam


def scan_hits(raw: bytes, raw_off, pattern: bytes, reach: int, mult=None, ignore_case: bool = False, dotall: bool = False):
    """What hmse_regex_scan reports: for every record [raw_off[r], raw_off[r + 1]) of raw and every start p in it with
    raw_off[r + 1] - p >= reach, the occurrence of the pattern in the RECORD's bytes.  -> (sorted [p << 8 | (length - 1)], count = the
    sum of mult[r] over the hits (mult None: 1 each))."""
    hits, count = [], 0
    for r in range(len(raw_off) - 1):
        a, b = int(raw_off[r]), int(raw_off[r + 1])
        for p, l in find(raw, pattern, reach, ignore_case, dotall, b, a):
            if b - p >= reach:
                hits.append((p << 8) | (l - 1))
                count += 1 if mult is None else int(mult[r])
    return hits, count


def nonoverlapping(offsets, lengths):
    """Of one pattern's occurrences, ascending by offset: the first, then each next one that starts at or behind the previous kept
    one's end (leftmost-longest, grep -o).  -> the kept indices."""
    keep, end = [], -1
    for i, (o, l) in enumerate(zip(offsets, lengths)):
        if o >= end:
            keep.append(i)
            end = o + l
    return keep
