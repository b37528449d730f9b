"""Plain-Python restatement of the asserting regex search's definitions (hmse_amd/regex.py Regex(assertions=True),
include/hmse_regexa.h), with the standard `re` module under re.MULTILINE as the oracle.  Independent of hmse_amd.regex apart from taking
`reach` as a number.

C is the corpus [0, N), r a pattern with ^ $ \\A \\Z \\b \\B, R = reach (1..256).  Start o is an occurrence iff some l with
1 <= l <= min(R, N - o) has C[o : o + l] matching r IN CONTEXT: every assertion sees the real bytes C[o - 1] and C[o + l], or the text's
edge at 0 and N.  Its length is the largest such l.  Empty matches are never reported; every start counts.

`re` is always run on the WHOLE buffer with pos = o, never with endpos or on a slice: either would fake an edge.  "C[o : o + l] matches in
context" is (?:r)(?=[\\s\\S]{N - o - l}\\Z) matched at o: the look-ahead pins the end and backtracking explores every alternative.  That is
O(N) per question and O(reach) questions per start, so whole buffers stay at a few hundred bytes; in a large buffer the interesting bytes
are planted in filler the pattern cannot touch and only the starts of windows around them are asked (find(..., lo, hi))."""
import re

_WORD = frozenset(b"0123456789_abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")


def _flags(ignore_case: bool, dotall: bool) -> int:
    return re.MULTILINE | (re.IGNORECASE if ignore_case else 0) | (re.DOTALL if dotall else 0)


class Oracle:
    def __init__(self, pattern: bytes, ignore_case: bool = False, dotall: bool = False):
        self.pattern, self.flags = pattern, _flags(ignore_case, dotall)
        self.any = re.compile(b"(?:" + pattern + b")", self.flags)
        self.tails = {}

    def matches(self, corpus: bytes, o: int, l: int) -> bool:
        """C[o : o + l] matches in context"""
        t = len(corpus) - o - l
        rx = self.tails.get(t)
        if rx is None:
            rx = self.tails[t] = re.compile(b"(?:" + self.pattern + b")(?=[\\s\\S]{%d}\\Z)" % t, self.flags)
        return rx.match(corpus, o) is not None

    def length_at(self, corpus: bytes, o: int, reach: int) -> int:
        if self.any.match(corpus, o) is None:                        # no match of any length from o (the empty one included)
            return 0
        for l in range(min(reach, len(corpus) - o), 0, -1):
            if self.matches(corpus, o, l):
                return l
        return 0

    def find(self, corpus: bytes, reach: int, lo: int = 0, hi: int | None = None):
        """-> [(o, length)] ascending: every occurrence with lo <= o < hi (hi None: N)."""
        out = []
        for o in range(lo, len(corpus) if hi is None else hi):
            l = self.length_at(corpus, o, reach)
            if l:
                out.append((o, l))
        return out


def find(corpus: bytes, pattern: bytes, reach: int, ignore_case: bool = False, dotall: bool = False, lo: int = 0, hi: int | None = None):
    return Oracle(pattern, ignore_case, dotall).find(corpus, reach, lo, hi)


def lengths(corpus: bytes, pattern: bytes, reach: int, ignore_case: bool = False, dotall: bool = False):
    """-> [length at every start] (0: no occurrence), what Regex.match_all returns."""
    orc = Oracle(pattern, ignore_case, dotall)
    return [orc.length_at(corpus, o, reach) for o in range(len(corpus))]


def is_seam(o: int, reach: int, cuts, k: int) -> bool:
    """The partition rule: start o of the non-empty chunk k is a SEAM start iff it is the chunk's first byte (the byte in front lies in
    another chunk) or cuts[k + 1] - o <= reach (the walk, or its one byte of look-ahead, may leave the chunk); else a SCAN start."""
    return o == cuts[k] or cuts[k + 1] - o <= reach


def split(found, reach: int, cuts):
    """`found` = find(...) of the corpus, cuts the chunk boundaries (ascending, cuts[0] = 0, cuts[-1] = N; equal neighbours are empty
    chunks).  -> (scan [(o, length)], seam [(o, length)]), both ascending."""
    scan, seam = [], []
    k = 0
    for o, l in found:
        while cuts[k + 1] <= o:
            k += 1
        (seam if is_seam(o, reach, cuts, k) else scan).append((o, l))
    return scan, seam


def scan_hits(raw: bytes, raw_off, pattern: bytes, reach: int, mult=None, ignore_case: bool = False, dotall: bool = False, windows=None):
    """What hmse_regexa_scan reports: for every record [raw_off[r], raw_off[r + 1]) of raw and every start p in it with p > raw_off[r] and
    raw_off[r + 1] - p > reach, the occurrence of the pattern — the byte in front, the match and its look-ahead byte all lie in the record,
    so `raw` as the text gives the record's own answer.  `windows`: [(lo, hi)] of raw positions to ask (None: all).
    -> (sorted [p << 8 | (length - 1)], count = the sum of mult[r] over the hits (mult None: 1 each))."""
    orc = Oracle(pattern, ignore_case, dotall)
    hits, count = [], 0
    for r in range(len(raw_off) - 1):
        a, b = int(raw_off[r]), int(raw_off[r + 1])
        for lo, hi in ([(a, b)] if windows is None else windows):
            for p in range(max(lo, a + 1), min(hi, b - reach)):
                l = orc.length_at(raw, p, reach)
                if l:
                    hits.append((p << 8) | (l - 1))
                    count += 1 if mult is None else int(mult[r])
    return sorted(hits), count


def kind(corpus: bytes, i: int) -> int:
    """EDGE = 0, NL = 1, WORD = 2, OTHER = 3"""
    return 0 if i < 0 or i >= len(corpus) else 1 if corpus[i] == 0x0A else 2 if corpus[i] in _WORD else 3
