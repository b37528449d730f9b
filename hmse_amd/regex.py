"""Regular expressions compiled on the host into the bounded DFA that hmse_regex_scan / hmse_regex_seams walk (include/hmse.h `hmse_regex`).

numpy only: importable and usable without a GPU (device=None keeps the numpy arrays).  Definitions (tests/regex_ref.py restates them in
plain Python with the standard `re` module as the oracle):
  * a regex r denotes a set of byte strings L(r); start o of a buffer is an OCCURRENCE iff some l with 1 <= l <= min(reach, n - o) has
    buf[o : o + l] in L(r); its LENGTH is the largest such l.  Empty matches are never reported, every start counts (overlapping ones
    included), and a match is at most HMSE_REGEX_MAX_LEN = 256 bytes: `x.*y` reports the longest match within 256 bytes.
  * syntax (bytes only): literal bytes; the metacharacters \\ . [ ] ( ) | ? * + { } ^ $ escaped to be literal; \\n \\r \\t \\f \\v, \\xHH,
    \\d \\D \\w \\W \\s \\S (ASCII), \\ plus ASCII punctuation; `.` (any byte but 0x0A; dotall: any byte); classes [...] and [^...] with
    ranges and those escapes ([ ] ^ - \\ escaped inside); groups ( ) and (?: ) (nothing is captured); alternation (an empty alternative
    is allowed); ? * + {m} {m,} {m,n} with m <= n <= 256.  What is accepted means what it means to `re` in bytes mode; everything else
    (anchors and \\b unless assertions=True, back-references, octal, lazy and possessive forms, a quantifier on a quantifier or on
    nothing, other (? forms, {,n}) is refused with a RegexError naming the byte offset.
  * ignore_case closes every literal and class under ASCII case BEFORE a class is negated (re.IGNORECASE on bytes); bytes >= 0x80
    are untouched; the data is never folded.
Compiled form (deterministic): Glushkov position automaton -> subset construction -> minimal DFA.  State 0 is the dead state (its row
is all 0), state 1 the start, the others in BFS order from the start over the classes in ascending order; `classmap` u8[256] (bytes with
equal columns share a class, classes numbered by their smallest byte); `table` u16[n_states * n_classes] = next state, OR-ed with
HMSE_REGEX_ACCEPT iff the next state accepts; `reach` = the longest path from the start through live states if that graph is acyclic,
else 256.
assertions=True (opt-in; the default accepts and refuses exactly as above): the parser additionally takes the zero-width assertions ^ $ \\A
\\Z \\b \\B with the meaning of re.MULTILINE on bytes — between the previous byte a and the next byte b (the text is the whole buffer;
its ends are the EDGE): ^ iff a is the edge or 0x0A, $ iff b is, \\A iff a is the edge, \\Z iff b is, \\b iff exactly one of a, b is an
ASCII word byte, \\B otherwise.  An occurrence's assertions are evaluated against the real buf[o - 1] and buf[o + l].  Refused with the
offset: a quantifier directly on an assertion (a group that holds one may be quantified), \\b in a class, \\z, \\G, look-around, inline
flags; a pattern that can match nothing non-empty is refused as "matches nothing but the empty string".  Compiled form
(include/hmse_regexa.h; tests/regexa_ref.py is the oracle): an assertion is a 16-bit mask over (kind before, kind after),
kinds EDGE = 0, NL = 1, WORD = 2, OTHER = 3; Glushkov with masks; a state is (positions, kind of the byte just read); four start states
`start` (by the kind in front) numbered first, then BFS; the classes refine the kinds and EDGE is one more, the last (`edge_class`), whose
column leads to state 0; the accept flag of table[s * n_classes + c] says that a match may end just BEFORE a byte of class c; the walk
reads reach + 1 classes.  Out of scope: look-around, Unicode word classes, CR handling, multi-byte line terminators.
Both forms are one pipeline with two front ends: the passes from _byte_columns to _reach below are shared; what a
state is and when it accepts is Regex._subsets / _minimise and Regex._subsets_asserting / _minimise_asserting.  The kernels that walk
either table are hmse_amd/csrc/regex_core.h; tests/golden/regex_compiled.json pins the compiled form.
"""
from __future__ import annotations

import numpy as np

HMSE_REGEX_MAX_LEN = 256
HMSE_REGEX_MAX_TABLE = 16384
HMSE_REGEX_ACCEPT = 0x8000
MAX_STATES = 32767
_MAX_POSITIONS = 4096          # literal / class positions after expanding the counted repeats
_MAX_SUBSETS = 1 << 16         # states of the subset construction (before it is minimised)

_ALL = (1 << 256) - 1
_PUNCT = frozenset(b"!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~")
_HEX = frozenset(b"0123456789abcdefABCDEF")


def _mask(values) -> int:
    m = 0
    for v in values:
        m |= 1 << v
    return m


_DIGIT = _mask(range(0x30, 0x3A))
_WORD = _DIGIT | _mask(range(0x41, 0x5B)) | _mask(range(0x61, 0x7B)) | (1 << 0x5F)
_SPACE = _mask(b" \t\n\r\f\v")
_CATEGORY = {ord("d"): _DIGIT, ord("D"): _ALL & ~_DIGIT, ord("w"): _WORD, ord("W"): _ALL & ~_WORD, ord("s"): _SPACE, ord("S"): _ALL & ~_SPACE}
_CONTROL = {ord("n"): 0x0A, ord("r"): 0x0D, ord("t"): 0x09, ord("f"): 0x0C, ord("v"): 0x0B}
_UPPER, _LOWER = _mask(range(0x41, 0x5B)), _mask(range(0x61, 0x7B))


def _close_case(m: int) -> int:
    return m | ((m & _UPPER) << 32) | ((m & _LOWER) >> 32)


# ---- assertions (assertions=True): the KIND of a byte, and an assertion as a 16-bit mask over (kind of the byte before, kind of the byte after)
EDGE, NL, WORD, OTHER = 0, 1, 2, 3
_FULL = 0xFFFF


def byte_kind(b: int) -> int:
    return NL if b == 0x0A else WORD if (_WORD >> b) & 1 else OTHER


def _pairs(holds) -> int:
    return sum(1 << (a * 4 + b) for a in range(4) for b in range(4) if holds(a, b))


_ASSERTION = {"^": _pairs(lambda a, b: a in (EDGE, NL)), "$": _pairs(lambda a, b: b in (EDGE, NL)),
              "A": _pairs(lambda a, b: a == EDGE), "Z": _pairs(lambda a, b: b == EDGE),
              "b": _pairs(lambda a, b: (a == WORD) != (b == WORD)), "B": _pairs(lambda a, b: (a == WORD) == (b == WORD))}


_KIND_OF = np.array([byte_kind(b) for b in range(256)], np.int64)


class RegexError(ValueError):
    """A pattern outside the syntax or above a cap; `offset` is the byte offset in the pattern (None for a cap)."""

    def __init__(self, what: str, offset=None):
        super().__init__(f"regex: {what}" + (f" at offset {offset}" if offset is not None else ""))
        self.offset = offset


# ---- parser: pattern -> tree of ("set", mask) | ("cat", [..]) | ("alt", [..]) | ("rep", node, m, n or None) ------------------------------
class _Parser:
    def __init__(self, pat: bytes, ignore_case: bool, dotall: bool, assertions: bool = False):
        self.p, self.i, self.ic, self.dotall, self.assertions = pat, 0, ignore_case, dotall, assertions

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):                                    # only an unmatched ')' stops alt() early
            raise RegexError("unbalanced ')'", self.i)
        return node

    def alt(self):
        alts = [self.cat()]
        while self.i < len(self.p) and self.p[self.i] == 0x7C:      # |
            self.i += 1
            alts.append(self.cat())
        return alts[0] if len(alts) == 1 else ("alt", alts)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in b"|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        at = self.i
        c = self.p[at]
        if c in b"?*+{":
            raise RegexError("a quantifier with nothing in front", at)
        if c in b"}]":
            raise RegexError(f"an unescaped {chr(c)!r}", at)
        if c in b"^$":
            if not self.assertions:
                raise RegexError(f"the anchor {chr(c)!r} (line anchors are out of scope)", at)
            self.i += 1
            return self.asserted(_ASSERTION[chr(c)])
        if self.assertions and c == 0x5C and self.p[at + 1: at + 2] in (b"A", b"Z", b"b", b"B"):
            self.i += 2
            return self.asserted(_ASSERTION[chr(self.p[at + 1])])
        node = self.atom()
        q = self.quantifier()
        if q is None:
            return node
        if self.i < len(self.p) and self.p[self.i] in b"?+":
            raise RegexError("a lazy or possessive quantifier", self.i)
        if self.i < len(self.p) and self.p[self.i] in b"*{":
            raise RegexError("a quantifier on a quantifier", self.i)
        return ("rep", node, q[0], q[1])

    def asserted(self, mask: int):
        if self.i < len(self.p) and self.p[self.i] in b"?*+{":
            raise RegexError("a quantifier on an assertion (quantify a group that holds it)", self.i)
        return ("assert", mask)

    def quantifier(self):
        if self.i >= len(self.p):
            return None
        c, at = self.p[self.i], self.i
        if c == 0x3F:
            self.i += 1
            return 0, 1
        if c == 0x2A:
            self.i += 1
            return 0, None
        if c == 0x2B:
            self.i += 1
            return 1, None
        if c != 0x7B:
            return None
        j = self.p.find(b"}", at)
        body = self.p[at + 1: j] if j >= 0 else b""
        lo, comma, hi = body.partition(b",")
        if j < 0 or not lo.isdigit() or (hi and not hi.isdigit()) or len(lo) > 4 or len(hi) > 4:
            raise RegexError("an unescaped '{' that is no {m}, {m,} or {m,n}", at)
        m = int(lo)
        n = m if not comma else (int(hi) if hi else None)
        if m > HMSE_REGEX_MAX_LEN or (n is not None and (n > HMSE_REGEX_MAX_LEN or n < m)):
            raise RegexError(f"a repeat count outside m <= n <= {HMSE_REGEX_MAX_LEN}", at)
        self.i = j + 1
        return m, n

    def atom(self):
        at = self.i
        c = self.p[at]
        if c == 0x28:                                               # (
            self.i += 1
            if self.i < len(self.p) and self.p[self.i] == 0x3F:
                if self.p[self.i + 1: self.i + 2] != b":":
                    raise RegexError("a (? form other than (?:", at)
                self.i += 2
            node = self.alt()
            if self.i >= len(self.p):
                raise RegexError("unbalanced '('", at)
            self.i += 1                                             # )
            return node
        if c == 0x5B:
            return ("set", self.klass())
        if c == 0x2E:
            self.i += 1
            return ("set", _ALL if self.dotall else _ALL & ~(1 << 0x0A))
        if c == 0x5C:
            kind, v = self.escape()
            m = v if kind == "set" else 1 << v
        else:
            self.i += 1
            m = 1 << c
        return ("set", _close_case(m) if self.ic else m)

    def escape(self):
        """At a backslash -> ("byte", value) or ("set", mask)."""
        at = self.i
        if at + 1 >= len(self.p):
            raise RegexError("a backslash at the end", at)
        c = self.p[at + 1]
        self.i = at + 2
        if c in _CONTROL:
            return "byte", _CONTROL[c]
        if c in _CATEGORY:
            return "set", _CATEGORY[c]
        if c == 0x78:                                               # \xHH
            h = self.p[at + 2: at + 4]
            if len(h) != 2 or h[0] not in _HEX or h[1] not in _HEX:
                raise RegexError("\\x without two hex digits", at)
            self.i = at + 4
            return "byte", int(h, 16)
        if c in _PUNCT:
            return "byte", c
        raise RegexError(f"the escape \\{chr(c) if 0x20 < c < 0x7F else hex(c)}", at)

    def klass(self):
        at = self.i
        self.i += 1
        neg = self.i < len(self.p) and self.p[self.i] == 0x5E
        if neg:
            self.i += 1
        m = 0
        while True:
            if self.i >= len(self.p):
                raise RegexError("a class without its ']'", at)
            c, here = self.p[self.i], self.i
            if c == 0x5D:
                self.i += 1
                break
            if c in b"[^-":
                raise RegexError(f"an unescaped {chr(c)!r} inside a class", here)
            if c == 0x5C:
                kind, v = self.escape()
            else:
                kind, v = "byte", c
                self.i += 1
            if self.p[self.i: self.i + 1] == b"-":                  # a range (a '-' must be escaped to be literal)
                dash = self.i
                nxt = self.p[dash + 1: dash + 2]
                if kind == "set" or not nxt or nxt in (b"]", b"[", b"^", b"-"):
                    raise RegexError("an unescaped '-' inside a class that forms no range", dash)
                self.i = dash + 1
                if nxt == b"\\":
                    kind2, hi = self.escape()
                    if kind2 == "set":
                        raise RegexError("a range that ends in a class escape", dash + 1)
                else:
                    hi = nxt[0]
                    self.i += 1
                if hi < v:
                    raise RegexError("a descending range", here)
                m |= _mask(range(v, hi + 1))
            else:
                m |= v if kind == "set" else 1 << v
        if self.ic:
            m = _close_case(m)
        if m == 0 or (neg and m == _ALL):
            raise RegexError("an empty class", at)
        return _ALL & ~m if neg else m


# ---- tree -> Glushkov automaton ---------------------------------------------------------------------------------------------------------
def _positions(node) -> int:
    k = node[0]
    if k == "set":
        return 1
    if k == "assert":
        return 0
    if k == "rep":
        m, n = node[2], node[3]
        return _positions(node[1]) * max(m + 1 if n is None else n, 1)
    return sum(_positions(c) for c in node[1])


def _glushkov(node, sym, follow):
    """-> (nullable, first, last) as position bit sets; appends to sym (the byte set of every position) and follow."""
    k = node[0]
    if k == "set":
        p = len(sym)
        sym.append(node[1])
        follow.append(0)
        return False, 1 << p, 1 << p
    if k == "alt":
        nu, fi, la = False, 0, 0
        for c in node[1]:
            a, b, d = _glushkov(c, sym, follow)
            nu, fi, la = nu or a, fi | b, la | d
        return nu, fi, la
    if k == "cat":
        nu, fi, la = True, 0, 0
        for c in node[1]:
            nu, fi, la = _concat((nu, fi, la), _glushkov(c, sym, follow), follow)
        return nu, fi, la
    _, body, m, n = node                                            # rep: m copies, then a star or n - m optional copies
    acc = (True, 0, 0)
    for _ in range(m):
        acc = _concat(acc, _glushkov(body, sym, follow), follow)
    if n is None:
        _, fi, la = _glushkov(body, sym, follow)
        _link(la, fi, follow)
        acc = _concat(acc, (True, fi, la), follow)
    else:
        for _ in range(n - m):
            _, fi, la = _glushkov(body, sym, follow)
            acc = _concat(acc, (True, fi, la), follow)
    return acc


def _link(last: int, first: int, follow):
    p = 0
    while last:
        if last & 1:
            follow[p] |= first
        last >>= 1
        p += 1


def _concat(a, b, follow):
    _link(a[2], b[1], follow)
    return a[0] and b[0], a[1] | (b[1] if a[0] else 0), b[2] | (a[2] if b[0] else 0)


# ---- the same with assertions: nullable is a mask, first / last map a position to a mask, follow[p] maps a successor to a mask ----------
def _or(d, e):
    d = dict(d)
    for p, m in e.items():
        d[p] = d.get(p, 0) | m
    return d


def _and(d, mask: int):
    return {p: m & mask for p, m in d.items() if m & mask}


def _link_masked(last, first, follow):
    for p, mp in last.items():
        f = follow[p]
        for q, mq in first.items():
            if mp & mq:
                f[q] = f.get(q, 0) | (mp & mq)


def _concat_masked(a, b, follow):
    _link_masked(a[2], b[1], follow)
    return a[0] & b[0], _or(a[1], _and(b[1], a[0])), _or(b[2], _and(a[2], b[0]))


def _glushkov_masked(node, sym, follow):
    """_glushkov with assertions: everything zero-width between two consumed bytes sees the same (kind before, kind after), so a sequence
    ANDs masks and an alternation ORs them.  A star contributes the full mask for zero iterations; further empty iterations only shrink it."""
    k = node[0]
    if k == "assert":
        return node[1], {}, {}
    if k == "set":
        p = len(sym)
        sym.append(node[1])
        follow.append({})
        return 0, {p: _FULL}, {p: _FULL}
    if k == "alt":
        nu, fi, la = 0, {}, {}
        for c in node[1]:
            a, b, d = _glushkov_masked(c, sym, follow)
            nu, fi, la = nu | a, _or(fi, b), _or(la, d)
        return nu, fi, la
    if k == "cat":
        acc = (_FULL, {}, {})
        for c in node[1]:
            acc = _concat_masked(acc, _glushkov_masked(c, sym, follow), follow)
        return acc
    _, body, m, n = node
    acc = (_FULL, {}, {})
    for _ in range(m):
        acc = _concat_masked(acc, _glushkov_masked(body, sym, follow), follow)
    if n is None:
        _, fi, la = _glushkov_masked(body, sym, follow)
        _link_masked(la, fi, follow)
        acc = _concat_masked(acc, (_FULL, fi, la), follow)
    else:
        for _ in range(n - m):
            _, fi, la = _glushkov_masked(body, sym, follow)
            acc = _concat_masked(acc, (_FULL, fi, la), follow)
    return acc


def _by_pair(d):
    """{position: mask} -> for each of the 16 (before, after) pairs the bit set of the positions whose mask holds it"""
    out = [0] * 16
    for p, m in d.items():
        j = 0
        while m:
            if m & 1:
                out[j] |= 1 << p
            m >>= 1
            j += 1
    return out


# ---- Glushkov automaton -> table: the passes both forms run.  What a state IS and when it accepts is the forms' own (Regex._subsets /
# _minimise, Regex._subsets_asserting / _minimise_asserting) -----------------------------------------------------------------------------
def _byte_columns(sym, by_kind: bool):
    """-> (cols, col_kind, byte_col): the distinct sets of positions that hold a byte — by_kind: of (positions, the byte's kind) — in
    order of their smallest byte, the kind of every column (None without by_kind) and the column of every byte"""
    pos_of = [0] * 256                                              # positions whose set holds byte b
    for p, m in enumerate(sym):
        bit, b = 1 << p, 0
        while m:
            if m & 1:
                pos_of[b] |= bit
            m >>= 1
            b += 1
    cols, col_kind, col_of, byte_col = [], [], {}, []
    for b in range(256):
        key = (pos_of[b], byte_kind(b) if by_kind else None)
        c = col_of.setdefault(key, len(cols))
        if c == len(cols):
            cols.append(key[0])
            col_kind.append(key[1])
        byte_col.append(c)
    return cols, col_kind, byte_col


def _state_id(ids, order, key) -> int:
    """the number of the subset construction's state `key`, a new one at the end of `order` if it has none"""
    j = ids.get(key)
    if j is None:
        j = ids[key] = len(order)
        if j >= _MAX_SUBSETS:
            raise RegexError(f"the subset construction exceeds {_MAX_SUBSETS} states (the table holds {HMSE_REGEX_MAX_TABLE} entries)")
        order.append(key)
    return j


def _fold_dead(trans, accepts, starts):
    """States from which no state with a true accepts[s] is reachable fold into the dead state 0 -> (live, trans).  A pattern none of
    whose starts keeps a successor is refused."""
    n, k = len(trans), len(trans[0])
    back = [[] for _ in range(n)]
    for s, row in enumerate(trans):
        for t in set(row):
            back[t].append(s)
    live = [False] * n
    stack = [s for s in range(n) if accepts[s]]
    for s in stack:
        live[s] = True
    while stack:
        for q in back[stack.pop()]:
            if not live[q]:
                live[q] = True
                stack.append(q)
    live[0] = False
    trans = [[t if live[t] else 0 for t in row] if live[s] else [0] * k for s, row in enumerate(trans)]
    if not any(any(trans[s]) for s in starts):
        raise RegexError("the pattern matches nothing but the empty string")
    return live, trans


def _refine(block, trans):
    """Moore: split the blocks of the partition block[s] by their rows until none splits -> block[s]"""
    n_blocks = len(set(block))
    while True:
        sig = {}
        block = [sig.setdefault((block[s], tuple(block[t] for t in trans[s])), len(sig)) for s in range(len(trans))]
        if len(sig) == n_blocks:
            return block
        n_blocks = len(sig)


def _number(block, trans, starts):
    """Number the blocks: dead 0, the starts' in their order, the others in BFS order over the columns in ascending order
    -> (rows, reps, num): the numbered states' rows, their first member states, the number of every block"""
    rep = {}
    for s in range(len(trans)):
        rep.setdefault(block[s], s)
    num, queue = {block[0]: 0}, []
    for s in starts:
        if block[s] not in num:
            num[block[s]] = len(num)
            queue.append(block[s])
    for b in queue:
        for t in trans[rep[b]]:
            if block[t] not in num:
                num[block[t]] = len(num)
                queue.append(block[t])
    reps = [rep[b] for b in num]                                    # (num is in the order of the numbers)
    return [[num[block[t]] for t in trans[r]] for r in reps], reps, num


def _classes(rows, byte_col, asserting: bool):
    """Bytes with equal columns — asserting: AND equal kinds — share a class, numbered by their smallest byte; asserting: EDGE is one
    more class, the last, whose column leads nowhere -> (classmap, keep, nxt): keep = the smallest byte of every class, nxt int64[m, nc]"""
    full = np.array(rows, np.int64)[:, np.array(byte_col)]          # [m, 256]
    seen, classmap, keep = {}, np.zeros(256, np.uint8), []
    for b in range(256):
        key = (full[:, b].tobytes(), byte_kind(b) if asserting else None)
        c = seen.get(key)
        if c is None:
            c = seen[key] = len(keep)
            keep.append(b)
        classmap[b] = c
    nxt = full[:, keep]
    if asserting:
        nxt = np.concatenate([nxt, np.zeros((len(rows), 1), np.int64)], axis=1)
    return classmap, keep, nxt


def _min_len(nxt, starts, accepts) -> int:
    """the shortest non-empty match: the steps from a start to the first state t with accepts[t]"""
    seen, frontier = set(starts), sorted(set(starts))
    for step in range(1, len(nxt) + 1):
        frontier = sorted({int(t) for s in frontier for t in nxt[s] if t})
        if any(accepts[t] for t in frontier):
            if step <= HMSE_REGEX_MAX_LEN:
                return step
            break
        frontier = [t for t in frontier if t not in seen]
        seen.update(frontier)
    raise RegexError(f"the shortest non-empty match has more than HMSE_REGEX_MAX_LEN = {HMSE_REGEX_MAX_LEN} bytes")


def _reach(nxt) -> int:
    """the longest path through the live states, 256 if they hold a cycle"""
    m = len(nxt)
    succ = [sorted({int(t) for t in nxt[s] if t}) for s in range(m)]
    indeg = [0] * m
    for s in range(1, m):
        for t in succ[s]:
            indeg[t] += 1
    depth, ready, done = [0] * m, [s for s in range(1, m) if indeg[s] == 0], 0
    while ready:
        s = ready.pop()
        done += 1
        for t in succ[s]:
            depth[t] = max(depth[t], depth[s] + 1)
            indeg[t] -= 1
            if indeg[t] == 0:
                ready.append(t)
    return min(max(depth), HMSE_REGEX_MAX_LEN) if done == m - 1 else HMSE_REGEX_MAX_LEN


class Regex:
    """A compiled regular expression (module docstring).  .n_states, .n_classes, .reach, .min_len; .table (uint16 numpy), .classmap
    (uint8 numpy); .match_at(buf, o) simulates the table on the host.  With a device: .rx (ops.Regex: the arrays in HBM and the
    `hmse_regex` header) and .resident_bytes.
    assertions=True: the ASSERTING form (module docstring; include/hmse_regexa.h) — .asserting, .start (the four start states, by the kind
    of the byte in front), .edge_class (= n_classes - 1), .rx an ops.RegexA; match_at / match_all evaluate the assertions against the real
    bytes around the match in `buf`, whose ends are the text's edges."""

    def __init__(self, pattern, ignore_case: bool = False, dotall: bool = False, device=None, assertions: bool = False):
        if isinstance(pattern, str) or not isinstance(pattern, (bytes, bytearray, memoryview)):
            raise RegexError(f"a pattern is bytes, got a {type(pattern).__name__} (encode it)")
        self.pattern, self.ignore_case, self.dotall = bytes(pattern), bool(ignore_case), bool(dotall)
        self.asserting, self.start, self.edge_class = bool(assertions), (1, 1, 1, 1), None
        tree = _Parser(self.pattern, self.ignore_case, self.dotall, self.asserting).parse()
        n_pos = _positions(tree)
        if n_pos > _MAX_POSITIONS:
            raise RegexError(f"{n_pos} literal / class positions after expanding the counted repeats; the compiler takes {_MAX_POSITIONS}")
        sym, follow = [], []
        if self.asserting:
            _, first, last = _glushkov_masked(tree, sym, follow)
            self._minimise_asserting(*self._subsets_asserting(sym, follow, first, last))
        else:
            nullable, first, last = _glushkov(tree, sym, follow)
            trans, accept, cols = self._subsets(sym, follow, nullable, first, last)
            self._minimise(trans, accept, cols)
        self.dev, self.rx, self.resident_bytes, self._lists = None, None, 0, None
        if device is not None:
            import torch
            from . import ops
            self.dev = torch.device(device)
            arrays = torch.from_numpy(self.table.view(np.int16).copy()).to(self.dev), torch.from_numpy(self.classmap.copy()).to(self.dev)
            if self.asserting:
                self.rx = ops.RegexA(*arrays, self.n_states, self.n_classes, self.reach, self.start)
            else:
                self.rx = ops.Regex(*arrays, self.n_states, self.n_classes, self.reach)
            self.resident_bytes = self.table.nbytes + self.classmap.nbytes

    # -- the plain form: a state is (positions just read, at the start); state 0 = dead, 1 = start; a state accepts or not --
    @staticmethod
    def _subsets(sym, follow, nullable, first, last):
        cols, _, byte_col = _byte_columns(sym, False)
        order = [(0, False), (0, True)]
        ids = {key: i for i, key in enumerate(order)}
        trans = [[0] * len(cols)]
        s = 1
        while s < len(order):
            ps, init = order[s]
            nxt, p = first if init else 0, 0
            while ps:
                if ps & 1:
                    nxt |= follow[p]
                ps >>= 1
                p += 1
            trans.append([_state_id(ids, order, (nxt & c, False)) if nxt & c else 0 for c in cols])
            s += 1
        return trans, [nullable if init else (ps & last) != 0 for ps, init in order], byte_col

    def _minimise(self, trans, accept, byte_col):
        live, trans = _fold_dead(trans, accept, (1,))
        # Moore: refine {dead} {accepting} {the others} until no block splits
        block = _refine([0 if not live[s] else (2 if accept[s] else 1) for s in range(len(trans))], trans)
        rows, reps, _ = _number(block, trans, (1,))
        m = len(rows)
        classmap, keep, nxt = _classes(rows, byte_col, False)
        nc = len(keep)
        if m > MAX_STATES or m * nc > HMSE_REGEX_MAX_TABLE:
            raise RegexError(f"the minimal DFA has {m} states x {nc} classes = {m * nc} table entries; the caps are {MAX_STATES} states and "
                             f"HMSE_REGEX_MAX_TABLE = {HMSE_REGEX_MAX_TABLE} entries")
        accb = np.array([i > 0 and accept[r] for i, r in enumerate(reps)], bool)
        self.n_states, self.n_classes = m, nc
        self.classmap = classmap
        self.table = (nxt | np.where(accb[nxt], HMSE_REGEX_ACCEPT, 0)).astype(np.uint16).reshape(-1)    # the flag: the NEXT state accepts
        self.accepting = accb
        self.min_len = _min_len(nxt, (1,), accb)
        self.reach = _reach(nxt)

    # -- the asserting form: a state is (positions just read, kind of the byte just read, is a start); states 1..4 = the starts by the kind
    #    in front; a state has a 4-bit signature: bit b = it accepts when the NEXT byte has kind b (b = EDGE included) --
    @staticmethod
    def _subsets_asserting(sym, follow, first, last):
        cols, col_kind, byte_col = _byte_columns(sym, True)          # the columns refine the kinds: 0x0A alone, word bytes, the rest
        first_by, last_by = _by_pair(first), _by_pair(last)
        follow_by = [_by_pair(f) for f in follow]
        order = [None] + [(0, a, True) for a in range(4)]
        ids = {key: i for i, key in enumerate(order)}
        trans, sig = [[0] * len(cols)], [0]
        s = 1
        while s < len(order):
            ps, a, init = order[s]
            nxt = [0, 0, 0, 0]                                        # by the kind of the byte read next
            if init:
                for b in (NL, WORD, OTHER):
                    nxt[b] = first_by[a * 4 + b]
                sig.append(0)                                         # (a start's flags are never looked at: the walk reports from i = 1 on)
            else:
                sig.append(sum(1 << b for b in range(4) if ps & last_by[a * 4 + b]))
                p = 0
                while ps:
                    if ps & 1:
                        f = follow_by[p]
                        for b in (NL, WORD, OTHER):
                            nxt[b] |= f[a * 4 + b]
                    ps >>= 1
                    p += 1
            trans.append([_state_id(ids, order, (nxt[kind] & c, kind, False)) if nxt[kind] & c else 0 for c, kind in zip(cols, col_kind)])
            s += 1
        return trans, sig, byte_col

    def _minimise_asserting(self, trans, sig, byte_col):
        starts = (1, 2, 3, 4)
        live, trans = _fold_dead(trans, sig, starts)
        # Moore from the partition by the 4-bit accept signature; a start without a live successor keeps a (zero) row of its own: the
        # header's start[] never names the dead state
        block = _refine([0 if not live[s] and s not in starts else (1 if not live[s] else 2 + sig[s]) for s in range(len(trans))], trans)
        rows, reps, num = _number(block, trans, starts)
        m = len(rows)
        classmap, keep, nxt = _classes(rows, byte_col, True)         # EDGE is one more class, the last
        nc = len(keep) + 1
        if m > MAX_STATES or nc > 256 or m * nc > HMSE_REGEX_MAX_TABLE:
            raise RegexError(f"the minimal DFA has {m} states x {nc} classes = {m * nc} table entries; the caps are {MAX_STATES} states, 256 "
                             f"classes and HMSE_REGEX_MAX_TABLE = {HMSE_REGEX_MAX_TABLE} entries")
        kinds = np.array([byte_kind(b) for b in keep] + [EDGE])
        sga = np.array([sig[r] if i else 0 for i, r in enumerate(reps)], np.int64)
        flag = (sga[:, None] >> kinds[None, :]) & 1                  # the flag: a match may end just BEFORE a byte of this class
        self.n_states, self.n_classes, self.edge_class = m, nc, nc - 1
        self.classmap = classmap
        self.table = (nxt | np.where(flag != 0, HMSE_REGEX_ACCEPT, 0)).astype(np.uint16).reshape(-1)
        self.accept_sig = sga.astype(np.uint8)
        self.accepting = sga != 0
        self.start = tuple(num[block[s]] for s in starts)
        self.min_len = _min_len(nxt, self.start, self.accepting)
        self.reach = _reach(nxt)

    def _match_at_asserting(self, buf, o: int) -> int:
        n, nc, (tab, cm) = len(buf), self.n_classes, self._lists
        s, best = self.start[byte_kind(buf[o - 1]) if o else EDGE], 0
        for i in range(self.reach + 1):                              # the read at i = reach is look-ahead only
            e = tab[s * nc + (cm[buf[o + i]] if o + i < n else self.edge_class)]
            if i and e & HMSE_REGEX_ACCEPT:
                best = i
            s = e & 0x7FFF
            if s == 0:
                break
        return best

    def _match_all_asserting(self, buf) -> np.ndarray:
        data = np.frombuffer(bytes(buf), np.uint8)
        n = data.size
        cls = np.append(self.classmap[data].astype(np.int64), self.edge_class)       # cls[n]: the look-ahead beyond the text
        before = np.append(EDGE, _KIND_OF[data[:-1]]) if n else np.zeros(0, np.int64)
        best = np.zeros(n, np.int64)
        idx, state = np.arange(n), np.array(self.start, np.int64)[before]
        tab = self.table.astype(np.int64)
        for i in range(self.reach + 1):
            if idx.size == 0:
                break
            e = tab[state * self.n_classes + cls[idx + i]]
            if i:
                best[idx[(e & HMSE_REGEX_ACCEPT) != 0]] = i
            state = e & 0x7FFF
            alive = state != 0                                       # (the EDGE column leads to state 0: no walk reads beyond cls[n])
            idx, state = idx[alive], state[alive]
        return best

    def match_at(self, buf, o: int) -> int:
        """The length of the occurrence at buf[o] (the longest match of 1..min(reach, len(buf) - o) bytes), or 0."""
        if self._lists is None:                                      # (plain lists: indexing a numpy array element by element is slow)
            self._lists = self.table.tolist(), self.classmap.tolist()
        if self.asserting:
            return self._match_at_asserting(buf, o)
        s, best, nc, (tab, cm) = 1, 0, self.n_classes, self._lists
        for i in range(min(self.reach, len(buf) - o)):
            e = tab[s * nc + cm[buf[o + i]]]
            s = e & 0x7FFF
            if s == 0:
                break
            if e & HMSE_REGEX_ACCEPT:
                best = i + 1
        return best

    def match_all(self, buf) -> np.ndarray:
        """match_at for every start of buf at once -> int64[len(buf)] (numpy: one step of all live walks per trip)."""
        if self.asserting:
            return self._match_all_asserting(buf)
        cls = self.classmap[np.frombuffer(bytes(buf), np.uint8)].astype(np.int64)
        n = cls.size
        best = np.zeros(n, np.int64)
        idx, state = np.arange(n), np.ones(n, np.int64)
        tab = self.table.astype(np.int64)
        for i in range(self.reach):
            keep = idx + i < n
            idx, state = idx[keep], state[keep]
            if idx.size == 0:
                break
            e = tab[state * self.n_classes + cls[idx + i]]
            state = e & 0x7FFF
            best[idx[(e & HMSE_REGEX_ACCEPT) != 0]] = i + 1
            alive = state != 0
            idx, state = idx[alive], state[alive]
        return best
