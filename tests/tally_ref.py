"""The definitions of include/hmse_tally.h in plain Python (the code under test is not imported): the folded text of a range, its key bit
for bit, whether two ranges are the same, and the tally of grouped ranges with its order and representatives."""
M1, M2 = 0x9E3779B1, 0x85EBCA6B
K_LEN, K_SEED = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93
MIX1, MIX2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53
U32, U64 = (1 << 32) - 1, (1 << 64) - 1


def fold_byte(b: int) -> int:
    """A..Z become a..z; every other value, bytes >= 0x80 included, stays as it is"""
    return b | 0x20 if 0x41 <= b <= 0x5A else b


def text_of(corpus: bytes, start: int, end: int, ignore_case: bool = False) -> bytes:
    t = corpus[start:end]
    return bytes(fold_byte(b) for b in t) if ignore_case else t


def key_of_text(text: bytes, seed: int = 0, key_bits: int = 64) -> int:
    """the key of an (already folded) text"""
    assert 1 <= key_bits <= 64
    a1 = a2 = 0
    p1 = p2 = 1
    for b in text:
        a1 = (a1 + (b + 1) * p1) & U32
        a2 = (a2 + (b + 1) * p2) & U32
        p1, p2 = (p1 * M1) & U32, (p2 * M2) & U32
    x = ((a1 | (a2 << 32)) ^ ((len(text) * K_LEN) & U64) ^ ((seed * K_SEED) & U64)) & U64
    x ^= x >> 33
    x = (x * MIX1) & U64
    x ^= x >> 33
    x = (x * MIX2) & U64
    x ^= x >> 33
    return x & ((1 << key_bits) - 1)


def key(corpus: bytes, start: int, end: int, ignore_case: bool = False, seed: int = 0, key_bits: int = 64) -> int:
    return key_of_text(text_of(corpus, start, end, ignore_case), seed, key_bits)


def keys(corpus: bytes, starts, ends, ignore_case: bool = False, seed: int = 0, key_bits: int = 64):
    return [key(corpus, s, e, ignore_case, seed, key_bits) for s, e in zip(starts, ends)]


def same(corpus: bytes, starts, ends, rep, ignore_case: bool = False):
    return [int(text_of(corpus, starts[i], ends[i], ignore_case) == text_of(corpus, starts[r], ends[r], ignore_case)) for i, r in enumerate(rep)]


def signed(x: int) -> int:
    """the u64 bits as the int64 a tensor carries"""
    return x - (1 << 64) if x >> 63 else x


def tally(corpus: bytes, starts, ends, ptr, ignore_case: bool = False, top=None):
    """-> dict(ptr, start, end, count, distinct, total, value_of) as lists: the fields of find.Tally.  Group j's ranges are
    [ptr[j], ptr[j + 1]); per group the distinct texts, each with its count and its representative (smallest start, then smallest
    index), ordered by count descending, then the representative's start, then its index; `top` keeps the first k per group."""
    n, G = len(starts), len(ptr) - 1
    out = dict(ptr=[0], start=[], end=[], count=[], distinct=[], total=[], value_of=[-1] * n)
    for j in range(G):
        members = {}
        for i in range(ptr[j], ptr[j + 1]):
            members.setdefault(text_of(corpus, starts[i], ends[i], ignore_case), []).append(i)
        values = []
        for t, idx in members.items():
            r = min(idx, key=lambda i: (starts[i], i))
            values.append((-len(idx), starts[r], r, idx))
        values.sort()
        out["distinct"].append(len(values))
        out["total"].append(ptr[j + 1] - ptr[j])
        for c, _, r, idx in values[:top]:
            for i in idx:
                out["value_of"][i] = len(out["start"])
            out["start"].append(starts[r]); out["end"].append(ends[r]); out["count"].append(-c)
        out["ptr"].append(len(out["start"]))
    return out
