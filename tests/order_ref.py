"""The definitions of include/hmse_order.h in plain Python (the code under test is not imported): the folded text of a range, its key at
a depth bit for bit, the common prefix of two ranges, and the order of grouped ranges with its runs of equal texts and its ranks."""
KEY_BYTES, R_MORE = 7, 8


def fold_byte(b: int) -> int:
    """A..Z become a..z; every other value, bytes >= 0x80 included, stays as it is"""
    return b | 0x20 if 0x41 <= b <= 0x5A else b


def text_of(corpus: bytes, start: int, end: int, ignore_case: bool = False) -> bytes:
    t = corpus[start:end]
    return bytes(fold_byte(b) for b in t) if ignore_case else t


def key_of_text(text: bytes, depth: int) -> int:
    """the key of an (already folded) text at a depth: seven bytes from there on, zeros beyond the end, and r = min(L - depth, 8)"""
    assert 0 <= depth <= len(text)
    k = 0
    for j in range(KEY_BYTES):
        k = (k << 8) | (text[depth + j] if depth + j < len(text) else 0)
    return (k << 4) | min(len(text) - depth, R_MORE)


def key(corpus: bytes, start: int, end: int, depth: int, ignore_case: bool = False) -> int:
    return key_of_text(text_of(corpus, start, end, ignore_case), depth)


def keys(corpus: bytes, starts, ends, depths, ignore_case: bool = False):
    return [key(corpus, s, e, d, ignore_case) for s, e, d in zip(starts, ends, depths)]


def lcp(corpus: bytes, starts, ends, rep, frm, ignore_case: bool = False):
    """per range: frm[i] + the bytes that agree with the partner's from text index frm[i] on.  The bytes in front of it are NOT looked at."""
    out = []
    for i, r in enumerate(rep):
        a, b = text_of(corpus, starts[i], ends[i], ignore_case), text_of(corpus, starts[r], ends[r], ignore_case)
        t, m = frm[i], min(len(a), len(b))
        assert t <= m
        if r == i:
            t = len(a)
        while r != i and t < m and a[t] == b[t]:
            t += 1
        out.append(t)
    return out


def order(corpus: bytes, starts, ends, ptr, ignore_case: bool = False, unique: bool = False):
    """-> dict(ptr, index, start, end, first, count, distinct, total, rank_of) as lists: the fields of find.Sorted.  Group j's ranges are
    [ptr[j], ptr[j + 1]); per group sorted by (folded text, start, index); `first` where a position's text differs from its predecessor's
    in the group; unique keeps those positions, and count then has the sizes of the runs they open (else 1 everywhere)."""
    n, G = len(starts), len(ptr) - 1
    out = dict(ptr=[0], index=[], start=[], end=[], first=[], count=[], distinct=[], total=[], rank_of=[-1] * n)
    for j in range(G):
        members = sorted(range(ptr[j], ptr[j + 1]), key=lambda i: (text_of(corpus, starts[i], ends[i], ignore_case), starts[i], i))
        texts = [text_of(corpus, starts[i], ends[i], ignore_case) for i in members]
        first = [p == 0 or texts[p] != texts[p - 1] for p in range(len(members))]
        heads = [p for p, f in enumerate(first) if f]
        runs = [b - a for a, b in zip(heads, heads[1:] + [len(members)])]
        for p, i in enumerate(members):
            out["rank_of"][i] = p
        keep = heads if unique else range(len(members))
        out["index"] += [members[p] for p in keep]
        out["first"] += [True] * len(heads) if unique else first
        out["count"] += runs if unique else [1] * len(members)
        out["distinct"].append(len(heads))
        out["total"].append(len(members))
        out["ptr"].append(len(out["index"]))
    out["start"] = [starts[i] for i in out["index"]]
    out["end"] = [ends[i] for i in out["index"]]
    return out
