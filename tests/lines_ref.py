"""Plain-Python reference of hmse_amd.find lines / text / grep (include/hmse.h hmse_lines_*), on the INPUT bytes — independent of any store.

For a corpus C of N bytes, a delimiter byte value d, an offset 0 <= o < N, before = b >= 0, after = a >= 0, reach = R >= 1:
  * start: look at positions o-1, o-2, ..., max(o-R, 0) in that order; start = 1 + the position of the (b+1)-th byte equal to d met on
    the way; fewer are met: start = max(o-R, 0), and START_CUT is set iff o-R > 0 (reaching the corpus's first byte is no cut);
  * end: look at positions o, o+1, ..., min(o+R, N)-1; end = the position of the (a+1)-th byte equal to d; fewer are met:
    end = min(o+R, N), and END_CUT is set iff o+R < N;
  * the extent is C[start : end): it never holds the closing delimiter, and a delimiter AT o closes o's own line;
  * lines(): per pattern the distinct (start, end) pairs of its occurrences, ascending, each with the number of occurrences that gave it
    and the OR of their flags.
"""
START_CUT, END_CUT, BAD = 1, 2, 128


def extent(C: bytes, o: int, d: int = 0x0A, b: int = 0, a: int = 0, R: int = 1 << 16):
    """-> (start, end, flags) of offset o; (0, 0, BAD) for an o outside the corpus."""
    N = len(C)
    if not 0 <= o < N:
        return 0, 0, BAD
    flags = 0
    need, start = b + 1, None
    for p in range(o - 1, max(o - R, 0) - 1, -1):
        if C[p] == d:
            need -= 1
            if need == 0:
                start = p + 1
                break
    if start is None:
        start = max(o - R, 0)
        if o - R > 0:
            flags |= START_CUT
    need, end = a + 1, None
    for p in range(o, min(o + R, N)):
        if C[p] == d:
            need -= 1
            if need == 0:
                end = p
                break
    if end is None:
        end = min(o + R, N)
        if o + R < N:
            flags |= END_CUT
    return start, end, flags


def split_extent(C: bytes, o: int, d: int, b: int, a: int):
    """What bytes.split gives when nothing is cut: line i is the one with L_i <= o <= R_i (R_i: the position of its closing delimiter,
    or N); -> (start of line max(i - b, 0), end of line i + a, or N if there is none)."""
    parts = bytes(C).split(bytes([d]))
    L, p = [], 0
    for s in parts:
        L.append(p)
        p += len(s) + 1
    Rr = [l + len(s) for l, s in zip(L, parts)]
    i = next(k for k in range(len(parts)) if L[k] <= o <= Rr[k])
    return L[max(i - b, 0)], (Rr[i + a] if i + a < len(parts) else len(C))


def lines(C: bytes, found, d: int = 0x0A, before: int = 0, after: int = 0, reach: int = 1 << 16):
    """found = (counts [P], ptr [P + 1], offsets) as find_ref.find gives them -> dict of lists in the shape of hmse_amd.find.Lines."""
    counts, ptr, offsets = found
    out = {"ptr": [0], "start": [], "end": [], "flags": [], "hits": [], "counts": []}
    for j in range(len(counts)):
        groups = {}
        for o in offsets[ptr[j]: ptr[j + 1]]:
            s, e, f = extent(C, int(o), d, before, after, reach)
            assert f != BAD
            g = groups.setdefault((s, e), [0, 0])
            g[0] += 1
            g[1] |= f
        for (s, e), (h, f) in sorted(groups.items()):
            out["start"].append(s); out["end"].append(e); out["flags"].append(f); out["hits"].append(h)
        out["counts"].append(len(groups))
        out["ptr"].append(len(out["start"]))
    return out


def text(C: bytes, start, end):
    """-> (the bytes of every extent back to back, off [L + 1])."""
    off, parts = [0], []
    for s, e in zip(start, end):
        parts.append(bytes(C[int(s): int(e)]))
        off.append(off[-1] + len(parts[-1]))
    return b"".join(parts), off


def tables(corpus: bytes, cuts):
    """A chunk map over `corpus`: exact dedupe of the chunks in order of first appearance -> (raw, raw_off, slot)."""
    seen, recs, slot = {}, [], []
    for k in range(len(cuts) - 1):
        c = bytes(corpus[cuts[k]: cuts[k + 1]])
        if c not in seen:
            seen[c] = len(recs)
            recs.append(c)
        slot.append(seen[c])
    raw_off = [0]
    for r in recs:
        raw_off.append(raw_off[-1] + len(r))
    return b"".join(recs), raw_off, slot
