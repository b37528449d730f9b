"""The definitions of include/hmse_subst.h in plain Python: the splice, the per-position form the kernel computes, the rules a call is
refused for, translate.  No numpy, no torch: lists of ints and bytes."""
LITERAL, FILL = 0, 1


def replacement(edit, reps, fill):
    """R_i of the edit (start, end, sel)"""
    s, e, r = edit
    return reps[r] * (e - s) if fill else reps[r]


def edits_ok(N, edits, reps, fill):
    """the edit rule end[i-1] <= start[i] <= end[i] <= N, sel[i] < n_rep, and in fill mode every replacement exactly one byte"""
    prev = 0
    for s, e, r in edits:
        if not (prev <= s <= e <= N) or not 0 <= r < len(reps):
            return False
        prev = e
    return not fill or all(len(r) == 1 for r in reps)


def splice(corpus, edits, reps, fill=False):
    """-> (O, out_off): O = C[0:start[0]) R_0 C[end[0]:start[1]) R_1 ... C[end[n-1]:N), out_off[i] = where R_i begins, out_off[n] = |O|"""
    assert edits_ok(len(corpus), edits, reps, fill)
    out, out_off, at = [], [], 0
    size = 0
    for ed in edits:
        s, e, _ = ed
        out.append(corpus[at:s]); size += s - at
        out_off.append(size)
        r = replacement(ed, reps, fill)
        out.append(r); size += len(r)
        at = e
    out.append(corpus[at:]); size += len(corpus) - at
    return b"".join(out), out_off + [size]


def out_offsets(N, edits, reps, fill=False):
    """out_off by its formula: start[i] + sum_{j<i} (|R_j| - (end[j] - start[j])), and |O| last"""
    off, grow = [], 0
    for ed in edits:
        off.append(ed[0] + grow)
        grow += len(replacement(ed, reps, fill)) - (ed[1] - ed[0])
    return off + [N + grow]


def per_position(corpus, edits, reps, out_off, fill=False):
    """the same output, byte by byte: the last edit i with out_off[i] <= p covers p with R_i, or p is the corpus byte p - D"""
    n, N = len(edits), len(corpus)
    out = bytearray()
    for p in range(out_off[n]):
        i = -1
        for j in range(n):                                  # (out_off never descends; among equal values the last one)
            if out_off[j] <= p:
                i = j
        if i >= 0:
            r = replacement(edits[i], reps, fill)
            if p < out_off[i] + len(r):
                out.append(r[p - out_off[i]])
                continue
        if n == 0:
            D = 0
        elif i + 1 < n:
            D = out_off[i + 1] - edits[i + 1][0]
        else:
            D = out_off[n] - N
        out.append(corpus[p - D])
    return bytes(out)


def translate(N, edits, out_off, q):
    """corpus offset q in 0..N -> output offset: inside a replaced range the start of its replacement, else where the kept byte went"""
    n = len(edits)
    for i, (s, e, _) in enumerate(edits):
        if s <= q < e:
            return out_off[i]
    c = sum(1 for _, e, _ in edits if e <= q)                # the edits in front of q (an insertion AT q lies in front of byte q)
    return q + (out_off[c] - edits[c][0] if c < n else out_off[n] - N)


def leftmost_longest(matches):
    """grep -o's chain over (start, length) pairs of one regex, every start with its longest match: the first, then each next one that
    starts at or behind the previous kept one's end"""
    kept, at = [], 0
    for s, ln in sorted(matches):
        if s >= at:
            kept.append((s, ln))
            at = s + ln
    return kept
