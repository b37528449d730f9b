"""Exact byte-pattern search over a store: where does this byte string occur?

Today's answer — read.read_store(...), .cpu(), bytes.find on the host — decodes the whole corpus, moves it over PCIe and scans every
duplicate chunk once per occurrence.  A corpus of N bytes holds only U <= N unique record bytes, so a StoreFinder decodes every record
ONCE (read.StoreReader.decode), keeps the records and the chunk map in HBM, and answers a query with
  scan    every pattern is looked for once per stored record (hmse_find_scan: each unique byte read once);
  place   every in-record hit belongs to every chunk that maps to the record, POINTERs included (sort, hmse_find_place);
  seams   only the max(m) - 1 bytes in front of each chunk boundary get a second look, through the chunk map (hmse_find_seams).
Definitions (tests/find_ref.py restates them in plain Python):
  * C is the N bytes read.read_store(store) returns (a multi-rank stream's store: in stream order); patterns are P >= 0 byte strings of
    1..256 bytes, equal ones may repeat and each is answered on its own;
  * an occurrence of pattern j is any offset o with C[o : o + m_j] == pat_j; overlapping occurrences all count;
  * ignore_case folds the ASCII letters A-Z to a-z on both sides, every other byte value (>= 0x80 included) compares exactly:
    bytes.lower() on both sides;
  * result: counts int64[P], and in CSR form ptr int64[P + 1], offsets int64[ptr[P]] — ascending per pattern, no offset twice.
Sorting, prefix sums and searchsorted go through torch (plumbing, as SimilarityIndex.locate does); the byte work runs in the HIP kernels
of hmse_amd/csrc/find.hip.  There is no CPU path.  Patterns, a PatternSet and a Regex go through ONE count / locate flow
(StoreFinder._count, _locate over a _Query); find, find_set and find_regex add only what is theirs.

A whole dictionary (up to 2^20 distinct patterns) is compiled once into a PatternSet and answered by StoreFinder.count_set / find_set with
ONE scan and ONE seam pass (hmse_amd/csrc/findset.hip; include/hmse.h hmse_findset_*): the same definitions, the same Found.  count and
find do not route there.

From a hit to its line: StoreFinder.lines turns the offsets of a Found into the extents of the lines (delimited records) they lie in,
with context and counts, StoreFinder.text returns their bytes, grep = lines(find(...)) (hmse_amd/csrc/lines.hip; include/hmse.h
hmse_lines_* has the definitions, tests/lines_ref.py restates them in plain Python).  The walk goes through the chunk map on the device:
nothing is read back, and a record that several chunks map to is looked at with the neighbours of each of its places.  Out of scope:
delimiters of more than one byte, CR stripping, merging the overlapping context of neighbouring hits (grep's "--" groups).

Regular expressions: a regex.Regex (compiled on the host into a bounded DFA, hmse_amd/regex.py has the syntax and the definitions) is
answered by StoreFinder.count_regex / find_regex / grep_regex with the same three steps — scan of the unique records, place, seams
(hmse_amd/csrc/regex_core.h, built by regex.hip; include/hmse.h hmse_regex_*) — split by START: a start whose record still holds `reach` bytes is a scan
start, the last reach - 1 starts of every chunk are seam starts.  The result is a RegexFound: a Found with the lengths of the matches.
A Regex compiled with assertions=True (^ $ \\A \\Z \\b \\B) goes through the same kernels' asserting form (hmse_amd/csrc/regexa.hip; include/hmse_regexa.h), whose scan
leaves a record's first start and its last `reach` ones to the seams as well.  Out of scope: captures, lazy matching, matches over
256 bytes, Unicode classes, look-around, assertions in a PatternSet or in the approximate search, several regexes fused into one
automaton, multi-byte line delimiters, routing find / find_set through the DFA.

Approximate search: StoreFinder.count_approx / find_approx / grep_approx answer "where does something within k edits of this string
occur?" (Levenshtein distance: insertion, deletion and substitution cost 1 each; patterns of 1..64 bytes, 0 <= k <= 16, k < len(pattern))
with the same three steps — scan, place, seams (hmse_amd/csrc/approx.hip, Myers' bit-vector algorithm; include/hmse.h hmse_approx_* has
the definitions, tests/approx_ref.py restates them in plain Python) — split by END: an end with m + k bytes of its record in front of it
is a scan end, the first m + k - 1 ends of every chunk are seam ends.  The result is an ApproxFound: a Found with the errors of every
occurrence, whose `offsets` are the matches' LAST bytes (every end within k edits counts, so the neighbouring ends of one fuzzy match
are each reported; best_ends keeps one per run).  With k = 0 they are find's offsets + m - 1.  StoreFinder.spans gives the (start, end)
of every occurrence, as text() accepts them.  Out of scope: patterns over 64 bytes, Hamming-only and transposition distances, weighted
costs, errors inside a regex, a dictionary of approximate patterns (PatternSet), routing find through this path.

Tally: StoreFinder.tally answers "which values did the expression take, and how often each" (grep -o RX | sort | uniq -c | sort -rn) for
the ranges of a RegexFound, a Lines or any (start, end) pair: per group the distinct texts with their counts and a representative
occurrence, most frequent first (hmse_amd/csrc/tally.hip; include/hmse_tally.h has the definitions, tests/tally_ref.py restates them in
plain Python).  Ranges are bucketed by a 64-bit key of their bytes (hmse_tally_keys) and a bucket's members are then compared with its
first member byte for byte (hmse_tally_same): a key that merely agrees proves nothing, and what does not equal its bucket's first member
waits for the next round under another seed.  tally_regex = tally(nonoverlapping(find_regex(rx))).  Out of scope: texts compared under
anything but byte or ASCII-folded equality, weighting occurrences, lexicographic ordering of values, tallying across several stores,
several short ranges packed into one wavefront, approximate (k-error) grouping of values.

Substitute: StoreFinder.substitute writes the corpus with the ranges of a RegexFound, a Lines or any (start, end) pair replaced
(sed 's/RX/repl/g'), StoreFinder.redact overwrites them with one byte so that lengths and offsets stay; the result, a Substituted, holds
the edited corpus in HBM as ingest.ingest_shard takes it (hmse_amd/csrc/subst.hip; include/hmse_subst.h has the definitions,
tests/subst_ref.py restates them in plain Python).  The groups' ranges are merged by a stable sort on start and checked here; the one
hmse_subst_apply call proves them again, and the out_off it is given, before it writes a byte.  substitute_regex =
substitute(nonoverlapping(find_regex(rx))).  Out of scope: captures and back-references, `&` (the whole match inside a replacement),
case-preserving replacement, editing the store's records in place without re-ingest, several stores, fill patterns longer than one byte.

Sort: StoreFinder.sort orders the ranges of a RegexFound, a Lines, a Tally or any (start, end) pair by the texts they cover, as Python
orders bytes (grep -o RX | sort; with unique=True sort -u, with its counts sort | uniq -c): per group the input indices in order, which
positions open a new text, and every range's rank (hmse_amd/csrc/order.hip; include/hmse_order.h has the definitions, tests/order_ref.py
restates them in plain Python).  A most-significant-bytes-first radix sort in rounds (order_ranges): the unresolved ranges are keyed by
seven bytes at their bucket's depth (hmse_order_keys) and stable-sorted by (bucket, key); what the key could not split is compared with
its bucket's first member (hmse_order_lcp), and the bucket goes on at the smallest common prefix.  sort_regex =
sort(nonoverlapping(find_regex(rx))).  Out of scope: descending order (flip a group), numeric, version, locale or key-field (-k)
comparison, merging several Sorteds or several stores, sorting the store's records themselves, several short ranges packed into one
wavefront.
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .read import StoreReader
from .regex import Regex, RegexError  # noqa: F401

MAX_PATTERN_LEN = ops.FIND_MAX_LEN
GROUP = ops.FIND_MAX_PATTERNS      # patterns per launch; more are answered in groups
APPROX_GROUP, APPROX_MAX_LEN, APPROX_MAX_K = ops.APPROX_MAX_PATTERNS, ops.APPROX_MAX_LEN, ops.APPROX_MAX_K
HMSE_FINDSET_MAX_PATTERNS = ops.FINDSET_MAX_PATTERNS     # distinct patterns of a PatternSet


@dataclass
class Found:
    ptr: torch.Tensor            # int64 [P + 1]: pattern j's occurrences are offsets[ptr[j]:ptr[j + 1]]
    offsets: torch.Tensor        # int64 corpus offsets, ascending per pattern
    counts: torch.Tensor         # int64 [P] occurrences per pattern


@dataclass
class RegexFound(Found):
    lengths: torch.Tensor = None  # int64, aligned with offsets: occurrence i is corpus[offsets[i] : offsets[i] + lengths[i]]


@dataclass
class ApproxFound(Found):
    errors: torch.Tensor = None   # int64, aligned with offsets: the edit distance of occurrence i; offsets[i] is the match's LAST byte
    patterns: tuple = ()          # the patterns (bytes) and ignore_case the occurrences were found with: what spans() needs
    ignore_case: bool = False


@dataclass
class Lines:
    ptr: torch.Tensor            # int64 [P + 1]: pattern j's extents are [ptr[j] : ptr[j + 1])
    start: torch.Tensor          # int64 [L] corpus offsets; per pattern ascending by (start, end), no (start, end) pair twice
    end: torch.Tensor            # int64 [L]
    flags: torch.Tensor          # uint8 [L]  HMSE_LINES_START_CUT | HMSE_LINES_END_CUT (of any of the extent's occurrences)
    hits: torch.Tensor           # int64 [L]  occurrences of the pattern that fell into this extent
    counts: torch.Tensor         # int64 [P]  extents per pattern (with before = after = 0 and no cut: matching lines, grep -c)


@dataclass
class Tally:
    ptr: torch.Tensor            # int64 [G + 1]: group j's values are [ptr[j] : ptr[j + 1]), count descending, then start, then index
    start: torch.Tensor          # int64 [D] the representative occurrence of each value: the member with the smallest (start, index)
    end: torch.Tensor            # int64 [D]
    count: torch.Tensor          # int64 [D] ranges per value
    distinct: torch.Tensor       # int64 [G] distinct values per group, before `top`
    total: torch.Tensor          # int64 [G] ranges per group
    value_of: torch.Tensor       # int64 [n] aligned with the input: the index of each occurrence's value, -1 where `top` cut it
    rounds: int = 0              # key / compare rounds the grouping took (1 unless keys collided)


@dataclass
class Sorted:
    ptr: torch.Tensor            # int64 [G + 1]: group j's positions are [ptr[j] : ptr[j + 1]), texts ascending, equal ones by (start, index)
    index: torch.Tensor          # int64 the input index at every position (of a Tally: the index of the value)
    start: torch.Tensor          # int64 the ranges in order
    end: torch.Tensor            # int64
    first: torch.Tensor          # bool  this position's text differs from its predecessor's in the group (a group's first position: True)
    count: torch.Tensor          # int64 the size of the run of equal texts a `first` position opens; with unique=False 1 everywhere
    distinct: torch.Tensor       # int64 [G] distinct texts per group
    total: torch.Tensor          # int64 [G] ranges per group
    rank_of: torch.Tensor        # int64 [n] aligned with the input: every range's position inside its group in the full order, before `unique`
    rounds: int = 0              # key / LCP rounds the ordering took


@dataclass
class Substituted:
    data: torch.Tensor           # uint8 [n_bytes_out] in HBM: the edited corpus; ingest.ingest_shard(data, cfg) takes it as it is
    start: torch.Tensor          # int64 [n_edits] the merged edits, ascending: corpus[start[i] : end[i]) was replaced
    end: torch.Tensor            # int64 [n_edits]
    sel: torch.Tensor            # int64 [n_edits] the replacement (the group) of every edit
    out_off: torch.Tensor        # int64 [n_edits + 1]: edit i's replacement begins at data[out_off[i]]; out_off[-1] = n_bytes_out
    n_edits: int
    n_bytes_in: int
    n_bytes_out: int

    def translate(self, offsets: torch.Tensor) -> torch.Tensor:
        """Corpus offsets (int64, 0..n_bytes_in, on the edits' device) -> offsets into `data`: a kept byte goes where it was written, an
        offset inside a replaced range to the start of its replacement, n_bytes_in to n_bytes_out.  searchsorted plumbing, no kernel."""
        if offsets.dtype != torch.int64 or offsets.device != self.start.device:
            raise ValueError(f"translate: offsets are int64 on the edits' device {self.start.device}, got {offsets.dtype} on {offsets.device}")
        q = offsets.reshape(-1)
        if q.numel() and (int(q.min()) < 0 or int(q.max()) > self.n_bytes_in):
            raise ValueError(f"translate: an offset lies outside 0..n_bytes_in = {self.n_bytes_in}")
        tail = torch.tensor([self.n_bytes_in], dtype=torch.int64, device=q.device)
        shift = self.out_off - torch.cat([self.start, tail])                     # of the kept bytes in front of edit c (behind the last: c = n)
        c = torch.searchsorted(self.end, q, right=True)                          # the edits that end at or in front of q lie in front of it
        return torch.minimum(q + shift[c], self.out_off[c]).reshape(offsets.shape)


def tally_ranges(start, end, group, n_groups: int, keys, same, top=None, max_rounds: int = 64) -> Tally:
    """The grouping of StoreFinder.tally over any tensors' device (tests run it on CPU tensors with plain-Python stand-ins):
    `keys(start, end, seed)` -> int64 keys and `same(start, end, rep)` -> 0 / 1 per range are the two ops calls.  Torch plumbing only,
    no host loop over the occurrences.  U, the unresolved ranges, stays ordered by (start, index); a round keys U under seed = round,
    stable-sorts it by (group, key), so that the first member of every run is the run's smallest-start member, compares every member
    with it and resolves those that equal it.  Every round resolves at least the first member of every bucket; RuntimeError naming the
    figures when more than max_rounds would be needed."""
    n, dev = start.numel(), start.device
    ar = lambda k: torch.arange(k, dtype=torch.int64, device=dev)
    value_rep = torch.full((n,), -1, dtype=torch.int64, device=dev)                 # per range: the index of its value's representative
    U = torch.sort(start, stable=True)[1]
    rounds = 0
    while U.numel():
        if rounds >= int(max_rounds):
            raise RuntimeError(f"tally: {U.numel()} of {n} ranges are unresolved after max_rounds = {max_rounds} rounds "
                               f"({int((value_rep == ar(n)).sum())} distinct values so far)")
        s, e, g = start[U].contiguous(), end[U].contiguous(), group[U]
        k = keys(s, e, rounds)
        o = torch.sort(k, stable=True)[1]                                        # by (group, key): two stable sorts
        o = o[torch.sort(g[o], stable=True)[1]]
        ks, gs = k[o], g[o]
        new = torch.ones(o.numel(), dtype=torch.bool, device=dev)
        new[1:] = (ks[1:] != ks[:-1]) | (gs[1:] != gs[:-1])
        first = torch.nonzero(new).reshape(-1)
        rep = torch.empty_like(o)
        rep[o] = o[first[torch.cumsum(new, 0) - 1]]                              # every run's first member, broadcast
        sm = same(s, e, rep) != 0
        value_rep[U[sm]] = U[rep[sm]]
        U = U[~sm]
        rounds += 1
    # the values: the ranges that represent themselves, ordered by (group, count descending, start, index)
    reps = torch.nonzero(value_rep == ar(n)).reshape(-1)
    cnt = torch.bincount(value_rep, minlength=n)[reps] if n else reps
    o = torch.sort(start[reps], stable=True)[1]
    o = o[torch.sort(cnt[o], stable=True, descending=True)[1]]
    o = o[torch.sort(group[reps][o], stable=True)[1]]
    reps, cnt = reps[o], cnt[o]
    g = group[reps]
    distinct = torch.bincount(g, minlength=n_groups)
    total = torch.bincount(group, minlength=n_groups)
    if top is not None:
        first_of = torch.zeros(n_groups + 1, dtype=torch.int64, device=dev)
        torch.cumsum(distinct, 0, out=first_of[1:])
        keep = ar(reps.numel()) - first_of[g] < int(top)                         # the rank inside the group
        reps, cnt, g = reps[keep], cnt[keep], g[keep]
    ptr = torch.zeros(n_groups + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(g, minlength=n_groups), 0, out=ptr[1:])
    index_of = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    index_of[reps] = ar(reps.numel())
    return Tally(ptr, start[reps], end[reps], cnt, distinct, total, index_of[value_rep], rounds)


ORDER_KEY_BYTES, ORDER_R_MORE = 7, 8          # include/hmse_order.h: text bytes in a key; the r of a text that goes on behind them


def order_ranges(start, end, group, n_groups: int, keys, lcp, unique: bool = False, max_rounds: int = 64, _skip: bool = True) -> Sorted:
    """The rounds of StoreFinder.sort over any tensors' device (tests run it on CPU tensors with plain-Python stand-ins):
    `keys(start, end, depth)` -> int64 keys and `lcp(start, end, rep, frm)` -> int64 common prefixes are the two ops calls.  Torch
    plumbing only, no host loop over the ranges.  P holds the ranges in their order so far — first by (group, start, index), and every
    sort is stable, so equal texts stay that way.  A bucket is a run of positions whose texts agree in their first `depth` bytes; it
    starts where `opens` is set.  A round keys the positions of the unfinished buckets at their depth and stable-sorts them by (bucket,
    key) in place; every run of equal keys is a sub-bucket, finished when it has one member or its key says the texts end within it
    (r <= 7: equal texts).  Every other sub-bucket asks lcp for its members' common prefix with its first member from depth + 7 on and
    goes on at the smallest of them, where the next keys split or finish it (_skip=False: at depth + 7, without the lcp call; the same
    result in more rounds).  RuntimeError naming the figures when more than max_rounds would be needed."""
    n, dev = start.numel(), start.device
    ar = lambda k: torch.arange(k, dtype=torch.int64, device=dev)
    P = torch.sort(start, stable=True)[1]                                        # by (group, start, index): two stable sorts
    P = P[torch.sort(group[P], stable=True)[1]]
    gP = group[P]
    opens = torch.ones(n, dtype=torch.bool, device=dev)
    opens[1:] = gP[1:] != gP[:-1]
    depth = torch.zeros(n, dtype=torch.int64, device=dev)                        # per position: its bucket's
    active = torch.ones(n, dtype=torch.bool, device=dev)
    rounds = 0
    while True:
        U = torch.nonzero(active).reshape(-1)
        m = U.numel()
        if m == 0:
            break
        if rounds >= int(max_rounds):
            raise RuntimeError(f"sort: {m} of {n} ranges are unresolved after max_rounds = {max_rounds} rounds "
                               f"(their buckets stand at depths {int(depth[U].min())}..{int(depth[U].max())})")
        idx, d = P[U], depth[U]
        bucket = torch.cumsum(opens, 0)[U]                                       # ascends with the positions
        k = keys(start[idx].contiguous(), end[idx].contiguous(), d.contiguous())
        o = torch.sort(k, stable=True)[1]                                        # by (bucket, key): two stable sorts; every bucket keeps its positions
        o = o[torch.sort(bucket[o], stable=True)[1]]
        idx, k = idx[o], k[o]
        P[U] = idx
        new = torch.ones(m, dtype=torch.bool, device=dev)
        new[1:] = (k[1:] != k[:-1]) | (bucket[1:] != bucket[:-1])
        opens[U] = new
        head = torch.nonzero(new).reshape(-1)                                    # every sub-bucket's first member
        sub = torch.cumsum(new, 0) - 1
        size = torch.diff(head, append=torch.full((1,), m, dtype=torch.int64, device=dev))
        done = (size[sub] == 1) | ((k & 15) < ORDER_R_MORE)
        active[U[done]] = False
        rest = torch.nonzero(~done).reshape(-1)
        if rest.numel():
            if _skip:
                at = torch.full((m,), -1, dtype=torch.int64, device=dev)
                at[rest] = ar(rest.numel())
                rep = at[head[sub[rest]]]                                        # the first member, as an index into the call's ranges
                ir = idx[rest]
                c = lcp(start[ir].contiguous(), end[ir].contiguous(), rep.contiguous(), (d[rest] + ORDER_KEY_BYTES).contiguous())
                least = torch.full((head.numel(),), 1 << 62, dtype=torch.int64, device=dev).scatter_reduce_(0, sub[rest], c, "amin")
                depth[U[rest]] = least[sub[rest]]                                # (the first member's own answer is its length: never below the others')
            else:
                depth[U[rest]] = d[rest] + ORDER_KEY_BYTES
        rounds += 1
    total = torch.bincount(group, minlength=n_groups)
    full_ptr = torch.zeros(n_groups + 1, dtype=torch.int64, device=dev)
    torch.cumsum(total, 0, out=full_ptr[1:])
    rank_of = torch.empty(n, dtype=torch.int64, device=dev)
    rank_of[P] = ar(n) - full_ptr[gP]
    distinct = torch.bincount(gP[opens], minlength=n_groups)
    if not unique:
        return Sorted(full_ptr, P, start[P], end[P], opens, torch.ones(n, dtype=torch.int64, device=dev), distinct, total, rank_of, rounds)
    head = torch.nonzero(opens).reshape(-1)
    count = torch.diff(head, append=torch.full((1,), n, dtype=torch.int64, device=dev))
    ptr = torch.zeros(n_groups + 1, dtype=torch.int64, device=dev)
    torch.cumsum(distinct, 0, out=ptr[1:])
    Ph = P[head]
    return Sorted(ptr, Ph, start[Ph], end[Ph], torch.ones(head.numel(), dtype=torch.bool, device=dev), count, distinct, total, rank_of, rounds)


# Something that can be searched for — a group of at most 32 patterns, a PatternSet's long entries, one Regex: its scan and seams calls
# (hits_cap -> (hits, n_hits, counts)), its place call and the width of the low field of its hit word.  StoreFinder._count and _locate
# are the one flow over it; the ops functions are looked up when a call is made.
_Query = namedtuple("_Query", "scan seams place low_bits")

HMSE_LINES_START_CUT, HMSE_LINES_END_CUT, HMSE_LINES_MAX_REACH = ops.LINES_START_CUT, ops.LINES_END_CUT, ops.LINES_MAX_REACH


def _lines_args(delim, before, after, reach):
    """The arguments lines and grep share -> (delimiter byte value, before, after, reach); ValueError before any device work."""
    if isinstance(delim, str) or not isinstance(delim, (bytes, bytearray, memoryview)) or len(bytes(delim)) != 1:
        raise ValueError(f"lines: delim is exactly one byte (bytes of length 1), got {delim!r}")
    before, after, reach = int(before), int(after), int(reach)
    if before < 0 or after < 0:
        raise ValueError(f"lines: before = {before} and after = {after} must not be negative")
    if not 1 <= reach <= HMSE_LINES_MAX_REACH:
        raise ValueError(f"lines: reach = {reach} lies outside 1..HMSE_LINES_MAX_REACH = {HMSE_LINES_MAX_REACH}")
    return bytes(delim)[0], min(before, 0xFFFFFFFF), min(after, 0xFFFFFFFF), reach


def pack_patterns(patterns):
    """A list of bytes-like patterns (bytes, bytearray, memoryview, uint8 numpy array) -> (uint8 numpy array of all of them back to
    back, list of P + 1 bounds).  ValueError for a str, an empty pattern or one over 256 bytes."""
    if isinstance(patterns, (str, bytes, bytearray, memoryview)) or (isinstance(patterns, np.ndarray) and patterns.ndim == 1 and patterns.dtype == np.uint8):
        raise ValueError("find: patterns is a LIST of byte strings (for one pattern: [pattern])")
    parts, off = [], [0]
    for i, p in enumerate(patterns):
        if isinstance(p, str):
            raise ValueError(f"find: pattern {i} is a str; patterns are bytes (encode it)")
        if isinstance(p, np.ndarray):
            if p.dtype != np.uint8 or p.ndim != 1:
                raise ValueError(f"find: pattern {i} is a {p.dtype} array of {p.ndim} dimensions; a numpy pattern is a 1-D uint8 array")
            b = p.tobytes()
        elif isinstance(p, (bytes, bytearray, memoryview)):
            b = bytes(p)
        else:
            raise ValueError(f"find: pattern {i} is a {type(p).__name__}; patterns are bytes-like")
        if not 1 <= len(b) <= MAX_PATTERN_LEN:
            raise ValueError(f"find: pattern {i} has {len(b)} bytes; a pattern has 1 to {MAX_PATTERN_LEN}")
        parts.append(b)
        off.append(off[-1] + len(b))
    return np.frombuffer(b"".join(parts), np.uint8), off


class PatternSet:
    """A dictionary of patterns compiled once for StoreFinder.count_set / find_set (include/hmse.h `hmse_findset`), usable against any
    number of stores and finders.  Accepts and refuses what pack_patterns does.  Equal patterns (after folding, when ignore_case) are
    stored once; `index` maps the caller's pattern j to its unique pattern and the results are expanded back through it.

    The unique patterns of 4 bytes or more are keyed by their first four bytes (u32, little endian), sorted by (h(key), key, length,
    bytes) with h(key) = key * 0x9E3779B1 mod 2^32 and stored back to back (upat / uoff / ukey / uid); `dir` (u32[2^b + 1], 2^b >= 2 U)
    maps the top b bits of h to their range of the sorted list and `bitmap` has bit (h >> 13) for every key.  Built on the host with
    sorts and searchsorted only: deterministic.  The unique patterns of 1..3 bytes have no four-byte key; they are kept aside
    (`short_ids`, `short_patterns`) and answered by the grouped kernels, 32 per launch.  device=None keeps the numpy arrays only."""

    def __init__(self, patterns, ignore_case: bool = False, device=None):
        flat, off = pack_patterns(patterns)
        self.ignore_case = bool(ignore_case)
        self.n_patterns = len(off) - 1
        blob = flat.tobytes()
        if self.ignore_case:
            blob = blob.lower()
        seen, uniq, index = {}, [], np.zeros(self.n_patterns, np.int64)
        for j in range(self.n_patterns):
            b = blob[off[j]: off[j + 1]]
            u = seen.get(b)
            if u is None:
                u = seen[b] = len(uniq)
                uniq.append(b)
            index[j] = u
        if len(uniq) > HMSE_FINDSET_MAX_PATTERNS:
            raise ValueError(f"find: {len(uniq)} distinct patterns; a PatternSet holds up to HMSE_FINDSET_MAX_PATTERNS = {HMSE_FINDSET_MAX_PATTERNS}")
        self.n_unique = len(uniq)
        self.index = index                                                       # int64 [P]: unique pattern of the caller's pattern j
        self.unique = uniq                                                       # the unique patterns (folded when ignore_case)
        self.short_ids = np.array([u for u, b in enumerate(uniq) if len(b) < ops.FINDSET_MIN_LEN], np.int64)
        self.short_patterns = [uniq[u] for u in self.short_ids]
        long_ids = np.array([u for u, b in enumerate(uniq) if len(b) >= ops.FINDSET_MIN_LEN], np.int64)
        key = np.array([int.from_bytes(uniq[u][:4], "little") for u in long_ids], np.uint64)
        h = (key * np.uint64(ops.FINDSET_HASH)) & np.uint64(0xFFFFFFFF)
        hl, kl, pl = h.tolist(), key.tolist(), [uniq[u] for u in long_ids]
        order = sorted(range(len(pl)), key=lambda i: (hl[i], kl[i], len(pl[i]), pl[i]))
        order = np.array(order, np.int64)
        n = len(order)
        self.n_entries = n
        self.uid = long_ids[order].astype(np.uint32)
        self.ukey = key[order].astype(np.uint32)
        ents = [uniq[u] for u in self.uid]
        self.uoff = np.zeros(n + 1, np.uint32)
        self.uoff[1:] = np.cumsum([len(b) for b in ents], dtype=np.int64)
        self.upat = np.frombuffer(b"".join(ents), np.uint8).copy()
        self.max_len = max([len(b) for b in ents], default=0)
        self.dir_bits = max(1, int(2 * n - 1).bit_length()) if n else 1          # 2^b >= 2 n
        hs = h[order]
        self.dir = np.searchsorted(hs >> np.uint64(32 - self.dir_bits), np.arange((1 << self.dir_bits) + 1, dtype=np.uint64), "left").astype(np.uint32)
        bit = (hs >> np.uint64(32 - ops.FINDSET_BITMAP_BITS)).astype(np.int64)
        self.bitmap = np.zeros(1 << (ops.FINDSET_BITMAP_BITS - 5), np.uint32)
        np.bitwise_or.at(self.bitmap, bit >> 5, (np.uint32(1) << (bit & 31).astype(np.uint32)))
        self.dev = None if device is None else torch.device(device)
        self.set = None
        self.resident_bytes = 0
        if self.dev is not None:
            t = lambda a: torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else a.dtype).copy()).to(self.dev)
            self.set = ops.FindSet(t(self.upat), t(self.uoff), t(self.ukey), t(self.uid), t(self.dir), t(self.bitmap), self.n_unique,
                                   self.dir_bits, self.max_len, self.ignore_case)
            self.index_d = torch.from_numpy(index).to(self.dev)
            self.short_ids_d = torch.from_numpy(self.short_ids).to(self.dev)
            self.short_pat = torch.from_numpy(np.frombuffer(b"".join(self.short_patterns), np.uint8).copy()).to(self.dev)
            self.resident_bytes = sum(x.numel() * x.element_size() for x in (self.set.upat, self.set.uoff, self.set.ukey, self.set.uid, self.set.dir,
                                                                              self.set.bitmap, self.index_d, self.short_ids_d, self.short_pat))

    def short_groups(self):
        """The bounds of the 1..3-byte patterns inside short_pat, 32 per group: [(first short pattern, bounds list)]."""
        off = [0]
        for b in self.short_patterns:
            off.append(off[-1] + len(b))
        n = len(self.short_patterns)
        return [(g, off[g: min(g + GROUP, n) + 1]) for g in range(0, n, GROUP)]


class StoreFinder:
    def __init__(self, store, device, verify: bool = True):
        """store: a Manifest or a merged Store (read.StoreReader refuses what cannot be read: unmerged parts, unresolved pointers).
        Decodes every record once; verify checks the SHA-256 of the decoded records where the store carries digests."""
        rd = StoreReader(store, device)
        self.dev = torch.device(device)
        self.n_bytes = int(rd.n_bytes)
        self.n_records = int(len(rd.kind))
        if self.n_records:
            self.raw, self.raw_off = rd.decode(verify=verify)
        else:
            self.raw = torch.zeros(0, dtype=torch.uint8, device=device)
            self.raw_off = torch.zeros(1, dtype=torch.int64, device=device)
        self.slot = rd._t(rd.slot.astype(np.int64), torch.int64)
        self.cuts = rd._t(rd.cuts, torch.int64)
        if self.slot.numel() and int(self.slot.max()) >= self.n_records:
            raise ValueError("find: the chunk map names a record outside the index")
        # how many chunks map to each record: an in-record hit occurs that often in the corpus
        self.mult = torch.bincount(self.slot, minlength=self.n_records).to(torch.int32) if self.n_records else torch.zeros(0, dtype=torch.int32, device=device)
        self.resident_bytes = sum(t.numel() * t.element_size() for t in (self.raw, self.raw_off, self.slot, self.cuts, self.mult))

    # ------------------------------------------------------------------ the groups of a query
    def _groups(self, patterns):
        flat, off = pack_patterns(patterns)
        n = len(off) - 1
        pat = torch.from_numpy(flat.copy()).to(self.dev) if n else None
        return pat, [off[g: min(g + GROUP, n) + 1] for g in range(0, n, GROUP)], n

    # ------------------------------------------------------------------ the one query flow
    def _q_group(self, pat, off, ignore_case) -> _Query:
        return _Query(lambda cap: ops.find_scan(self.raw, self.raw_off, self.mult, pat, off, ignore_case, hits_cap=cap),
                      lambda cap: ops.find_seams(self.raw, self.raw_off, self.cuts, self.slot, pat, off, ignore_case, hits_cap=cap),
                      lambda *a: ops.find_place(*a), 8)

    def _q_set(self, ps: PatternSet) -> _Query:
        return _Query(lambda cap: ops.findset_scan(self.raw, self.raw_off, self.mult, ps.set, hits_cap=cap),
                      lambda cap: ops.findset_seams(self.raw, self.raw_off, self.cuts, self.slot, ps.set, hits_cap=cap),
                      lambda *a: ops.findset_place(*a), ops.FINDSET_ID_BITS)

    def _q_regex(self, r: Regex) -> _Query:
        scan, seams = ("regexa_scan", "regexa_seams") if r.asserting else ("regex_scan", "regex_seams")     # (an asserting Regex: regexa.hip)
        return _Query(lambda cap: getattr(ops, scan)(self.raw, self.raw_off, self.mult, r.rx, hits_cap=cap),
                      lambda cap: getattr(ops, seams)(self.raw, self.raw_off, self.cuts, self.slot, r.rx, hits_cap=cap),
                      lambda *a: ops.find_place(*a), 8)                          # (a regex hit word is find's: the length - 1 in the low byte)

    def _count(self, q: _Query):
        """-> (occurrences int64[counters of q], in-record hits of the scan, seam hits): two count-only launches."""
        _, n_scan, c_scan = q.scan(0)
        _, n_seam, c_seam = q.seams(0)
        return c_scan + c_seam, n_scan, n_seam

    def _locate(self, q: _Query, n_scan: int, n_seam: int):
        """-> the hit words of q with CORPUS offsets, in up to two pieces: the in-record hits laid out at every chunk of their record
        (ascending), the seam hits (any order)."""
        found = []
        if n_scan:
            hits, _, c_scan = q.scan(n_scan)
            hits = torch.sort(hits)[0]                                           # by position in raw, then the low field
            rec_lo = torch.searchsorted(hits, self.raw_off << q.low_bits)        # first hit of every record
            per_chunk = (rec_lo[1:] - rec_lo[:-1])[self.slot]
            chunk_out = torch.zeros(self.slot.numel() + 1, dtype=torch.int64, device=self.dev)
            torch.cumsum(per_chunk, 0, out=chunk_out[1:])
            found.append(q.place(hits, self.raw_off, self.cuts, self.slot, chunk_out, int(c_scan.sum())))
        if n_seam:
            found.append(q.seams(n_seam)[0])
        return found

    def _empty(self, n: int, cls=Found):
        z = lambda k: torch.zeros(k, dtype=torch.int64, device=self.dev)
        return cls(z(n + 1), z(0), z(n)) if cls is Found else cls(z(n + 1), z(0), z(n), z(0))

    def _ptr(self, counts: torch.Tensor) -> torch.Tensor:
        ptr = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=self.dev)
        torch.cumsum(counts, 0, out=ptr[1:])
        return ptr

    @staticmethod
    def _total_within(counts: torch.Tensor, max_hits: int, largest_only: bool = False) -> int:
        """-> the sum of counts; ValueError naming the counts (or the ten largest) if it exceeds max_hits."""
        total = int(counts.sum())
        if total > int(max_hits):
            if not largest_only:
                raise ValueError(f"find: {total} occurrences exceed max_hits = {max_hits}; counts per pattern: {counts.tolist()}")
            top = torch.topk(counts, min(10, counts.numel()))
            worst = ", ".join(f"pattern {int(j)}: {int(c)}" for c, j in zip(top.values.tolist(), top.indices.tolist()))
            raise ValueError(f"find: {total} occurrences exceed max_hits = {max_hits}; the largest counts: {worst}")
        return total

    @staticmethod
    def _all_located(located: int, counted: int) -> None:
        if located != counted:
            raise ops.HmseError(-1, f"find: {located} occurrences located, {counted} counted")

    def count(self, patterns, ignore_case: bool = False) -> torch.Tensor:
        """Occurrences per pattern, int64[P] on the device: two count-only launches per 32 patterns, nothing is materialised."""
        pat, groups, n = self._groups(patterns)
        if n == 0 or self.n_records == 0:
            return torch.zeros(n, dtype=torch.int64, device=self.dev)
        return torch.cat([self._count(self._q_group(pat, off, ignore_case))[0] for off in groups])

    def find(self, patterns, ignore_case: bool = False, max_hits: int = 1 << 24) -> Found:
        """Every occurrence of every pattern.  Counts first: ValueError naming the counts if their sum exceeds max_hits."""
        pat, groups, n = self._groups(patterns)
        if n == 0 or self.n_records == 0:
            return self._empty(n)
        qs = [self._q_group(pat, off, ignore_case) for off in groups]
        counted = [self._count(q) for q in qs]
        counts = torch.cat([c[0] for c in counted])
        total = self._total_within(counts, max_hits)
        parts = []
        for q, (c, n_scan, n_seam) in zip(qs, counted):
            found = self._locate(q, n_scan, n_seam)
            if found:
                h = torch.cat(found)
                key = torch.sort(((h & 0xFF) << 56) | (h >> 8))[0]          # by (pattern, offset): offsets stay below 2^56
                parts.append(key & ((1 << 56) - 1))
        offsets = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=self.dev)
        ptr = self._ptr(counts)
        self._all_located(offsets.numel(), total)
        return Found(ptr, offsets, counts)

    # ------------------------------------------------------------------ from a hit to its line
    def lines(self, found, delim: bytes = b"\n", before: int = 0, after: int = 0, reach: int = 1 << 16) -> Lines:
        """The extents of the lines the occurrences lie in (module docstring; include/hmse.h hmse_lines_extent): per occurrence the
        line it lies in with `before` lines in front and `after` behind, looking at most `reach` bytes each way; per pattern the
        distinct (start, end) pairs, ascending, with the number of occurrences that gave each.  `found`: a Found, or an int64 device
        tensor of corpus offsets taken as one pattern (any order, equal ones count).  ONE hmse_lines_extent call over all offsets; the
        grouping is torch sorts.  ValueError for a delim that is not one byte, a negative before / after, a reach outside
        1..HMSE_LINES_MAX_REACH, an offset that is not below n_bytes."""
        d, before, after, reach = _lines_args(delim, before, after, reach)
        if isinstance(found, Found):
            offsets, counts = found.offsets, found.counts
        elif isinstance(found, torch.Tensor):
            offsets, counts = found.reshape(-1), None
        else:
            raise ValueError(f"lines: found is a Found or an int64 tensor of offsets, got a {type(found).__name__}")
        dev = self.dev
        if offsets.dtype != torch.int64 or offsets.device != self.raw.device or (counts is not None and counts.device != self.raw.device):
            raise ValueError(f"lines: the offsets are {offsets.dtype} on {offsets.device}; they are int64 on the finder's device {self.raw.device}")
        n = offsets.numel()
        if counts is None:
            counts = torch.full((1,), n, dtype=torch.int64, device=dev)
        P = counts.numel()
        if int(counts.sum()) != n:
            raise ValueError(f"lines: found.counts sum to {int(counts.sum())}, found.offsets has {n} entries")
        z = lambda k, dt=torch.int64: torch.zeros(k, dtype=dt, device=dev)
        if n == 0:
            return Lines(z(P + 1), z(0), z(0), z(0, torch.uint8), z(0), z(P))
        if self.n_bytes == 0:
            raise ValueError(f"lines: offset {int(offsets[0])} is not below n_bytes = 0")
        start, end, flags, st = ops.lines_extent(self.raw, self.raw_off, self.cuts, self.slot, offsets.contiguous(), d, before, after, reach)
        if st & 1:
            bad = offsets[(flags & ops.LINES_BAD) != 0]
            raise ValueError(f"lines: offset {int(bad[0])} is not below n_bytes = {self.n_bytes} ({bad.numel()} of {n} offsets are not)")
        pat = torch.repeat_interleave(torch.arange(P, dtype=torch.int64, device=dev), counts)
        order = torch.sort(end, stable=True)[1]                                  # by (pattern, start, end): three stable sorts
        order = order[torch.sort(start[order], stable=True)[1]]
        order = order[torch.sort(pat[order], stable=True)[1]]
        pat, start, end, flags = pat[order], start[order], end[order], flags[order]
        new = torch.ones(n, dtype=torch.bool, device=dev)
        new[1:] = (pat[1:] != pat[:-1]) | (start[1:] != start[:-1]) | (end[1:] != end[:-1])
        first = torch.nonzero(new).reshape(-1)
        L = first.numel()
        gid = torch.cumsum(new, 0) - 1
        hits = torch.diff(first, append=torch.full((1,), n, dtype=torch.int64, device=dev))
        cut = lambda bit: (z(L).index_add_(0, gid, (flags & bit).to(torch.int64)) > 0).to(torch.uint8) * bit
        per = torch.bincount(pat[first], minlength=P)
        ptr = z(P + 1)
        torch.cumsum(per, 0, out=ptr[1:])
        return Lines(ptr, start[first], end[first], cut(ops.LINES_START_CUT) | cut(ops.LINES_END_CUT), hits, per)

    def text(self, lines, max_bytes: int = 1 << 30):
        """The bytes of every extent back to back -> (uint8 tensor, int64 off[L + 1]: extent i is bytes[off[i] : off[i + 1]]).  `lines`:
        a Lines, a Tally (the representative occurrence of every value), a Sorted (the ranges in their order) or a (start, end) pair of
        int64 device tensors (any ranges of the corpus; they may overlap and be empty).  One hmse_lines_gather call.  ValueError naming the total if it exceeds max_bytes."""
        if isinstance(lines, (Lines, Tally, Sorted)):                            # (a Tally: the representative occurrence of every value; a Sorted: the ranges in order)
            start, end = lines.start, lines.end
        elif isinstance(lines, (tuple, list)) and len(lines) == 2 and all(isinstance(t, torch.Tensor) for t in lines):
            start, end = (t.reshape(-1) for t in lines)
        else:
            raise ValueError(f"text: lines is a Lines or a (start, end) pair of tensors (or a Tally: its representatives), got a {type(lines).__name__}")
        if start.dtype != torch.int64 or end.dtype != torch.int64 or start.numel() != end.numel() or start.device != end.device or start.device != self.raw.device:
            raise ValueError(f"text: start and end are int64 tensors of one length on the finder's device {self.raw.device}")
        n, dev = start.numel(), self.dev
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n == 0:
            return torch.zeros(0, dtype=torch.uint8, device=dev), off
        if bool((end < start).any()):
            raise ValueError("text: an extent ends in front of its start")
        torch.cumsum(end - start, 0, out=off[1:])
        total = int(off[-1])
        if total > int(max_bytes):
            raise ValueError(f"text: the extents hold {total} bytes, which exceeds max_bytes = {max_bytes}")
        return ops.lines_gather(self.raw, self.raw_off, self.cuts, self.slot, start.contiguous(), end.contiguous(), off, total), off

    def grep(self, patterns, ignore_case: bool = False, delim: bytes = b"\n", before: int = 0, after: int = 0, reach: int = 1 << 16,
             max_hits: int = 1 << 24) -> Lines:
        """lines(find(patterns, ignore_case, max_hits), delim, before, after, reach): per pattern the lines that hold it."""
        _lines_args(delim, before, after, reach)
        return self.lines(self.find(patterns, ignore_case, max_hits), delim, before, after, reach)

    # ------------------------------------------------------------------ from ranges to the values they cover
    def tally(self, what, ignore_case: bool = False, top=None, max_rounds: int = 64, _key_bits: int = 64) -> Tally:
        """Per group the distinct texts among the ranges, with counts and a representative occurrence (module docstring;
        include/hmse_tally.h).  `what`: a RegexFound (offsets and lengths, one group per regex), a Lines (each extent counts once, one
        group per pattern), a (start, end) pair of int64 device tensors taken as one group, or a (start, end, ptr) triple with group
        j's ranges at [ptr[j] : ptr[j + 1]).  top = k keeps the k most frequent values of every group.  One hmse_tally_keys and one
        hmse_tally_same call per round (one round unless 64-bit keys collide; _key_bits is for tests); the grouping is torch sorts.
        ValueError for a plain Found or ApproxFound (they carry no lengths: use spans() or pass a (start, end) pair), a top below 1,
        ranges that descend or leave the corpus; RuntimeError when max_rounds rounds do not resolve every range."""
        dev = self.dev
        if top is not None and int(top) < 1:
            raise ValueError(f"tally: top = {top} must be at least 1 (None keeps every value)")
        if isinstance(what, RegexFound):
            start, end, ptr = what.offsets, what.offsets + what.lengths, what.ptr
        elif isinstance(what, Lines):
            start, end, ptr = what.start, what.end, what.ptr
        elif isinstance(what, Found):
            raise ValueError(f"tally: what is a {type(what).__name__}, which has offsets but no lengths; tally takes a RegexFound, a Lines, the (start, end) of "
                             "spans(), or any (start, end) pair of tensors")
        elif isinstance(what, (tuple, list)) and len(what) in (2, 3) and all(isinstance(t, torch.Tensor) for t in what):
            start, end = (t.reshape(-1) for t in what[:2])
            ptr = what[2].reshape(-1) if len(what) == 3 else None
        else:
            raise ValueError(f"tally: what is a RegexFound, a Lines, a (start, end) pair or a (start, end, ptr) triple of tensors, got a {type(what).__name__}")
        if any(t.dtype != torch.int64 or t.device != self.raw.device for t in (start, end) + (() if ptr is None else (ptr,))) or start.numel() != end.numel():
            raise ValueError(f"tally: start, end and ptr are int64 tensors on the finder's device {self.raw.device}, start and end of one length")
        n = start.numel()
        if ptr is None:
            ptr = torch.tensor([0, n], dtype=torch.int64, device=dev)
        G = ptr.numel() - 1
        per = ptr[1:] - ptr[:-1]
        if G < 0 or (G == 0 and n) or (G > 0 and (int(ptr[0]) != 0 or int(ptr[-1]) != n or bool((per < 0).any()))):
            raise ValueError(f"tally: ptr does not split the {n} ranges into groups (it ascends from 0 to {n})")
        z = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)
        if n == 0 or G == 0:
            return Tally(z(max(G, 0) + 1), z(0), z(0), z(0), z(max(G, 0)), z(max(G, 0)), z(0), 0)
        if bool(((start < 0) | (end < start) | (end > self.n_bytes)).any()):
            raise ValueError(f"tally: a range descends or leaves the corpus of n_bytes = {self.n_bytes}")
        group = torch.repeat_interleave(torch.arange(G, dtype=torch.int64, device=dev), per)
        keys = lambda s, e, seed: ops.tally_keys(self.raw, self.raw_off, self.cuts, self.slot, s, e, ignore_case, seed, _key_bits)
        same = lambda s, e, rep: ops.tally_same(self.raw, self.raw_off, self.cuts, self.slot, s, e, rep, ignore_case)
        return tally_ranges(start.contiguous(), end.contiguous(), group, G, keys, same, top, max_rounds)

    def tally_regex(self, rx, ignore_case: bool = False, top=None, max_hits: int = 1 << 24) -> Tally:
        """tally(nonoverlapping(find_regex(rx, max_hits)), ignore_case, top): per regex the values its leftmost-longest matches took,
        most frequent first (grep -o RX | sort | uniq -c | sort -rn).  ignore_case folds the VALUES; how the regex matches is the Regex's own."""
        return self.tally(nonoverlapping(self.find_regex(rx, max_hits)), ignore_case, top)

    # ------------------------------------------------------------------ from ranges to their lexicographic order
    def sort(self, what, ignore_case: bool = False, unique: bool = False, max_rounds: int = 64, _skip: bool = True) -> Sorted:
        """Per group the ranges in the order of their texts, as Python orders bytes; equal texts by (start, index) (module docstring;
        include/hmse_order.h).  `what`: what tally takes — a RegexFound (one group per regex), a Lines, a (start, end) pair of int64
        device tensors taken as one group, a (start, end, ptr) triple with group j's ranges at [ptr[j] : ptr[j + 1]) — or a Tally: its
        representatives are ordered and `index` points into the tally's values, so t.count[s.index] is uniq -c in lexicographic order.
        ignore_case folds A..Z before comparing.  unique=True keeps the first position of every run of equal texts (sort -u), `count`
        then has the runs' sizes (sort | uniq -c).  One hmse_order_keys and at most one hmse_order_lcp call per round; the rest is torch
        sorts.  ValueError for a plain Found or ApproxFound (they carry no lengths: use spans() or pass a (start, end) pair), ranges
        that descend or leave the corpus; RuntimeError when max_rounds rounds do not resolve every range (a chain a, aa, aaa, ...
        finishes eight ranges a round)."""
        dev = self.dev
        if isinstance(what, RegexFound):
            start, end, ptr = what.offsets, what.offsets + what.lengths, what.ptr
        elif isinstance(what, (Lines, Tally)):
            start, end, ptr = what.start, what.end, what.ptr
        elif isinstance(what, Found):
            raise ValueError(f"sort: what is a {type(what).__name__}, which has offsets but no lengths; sort takes a RegexFound, a Lines, a Tally, the (start, end) of "
                             "spans(), or any (start, end) pair of tensors")
        elif isinstance(what, (tuple, list)) and len(what) in (2, 3) and all(isinstance(t, torch.Tensor) for t in what):
            start, end = (t.reshape(-1) for t in what[:2])
            ptr = what[2].reshape(-1) if len(what) == 3 else None
        else:
            raise ValueError(f"sort: what is a RegexFound, a Lines, a Tally, a (start, end) pair or a (start, end, ptr) triple of tensors, got a {type(what).__name__}")
        if any(t.dtype != torch.int64 or t.device != self.raw.device for t in (start, end) + (() if ptr is None else (ptr,))) or start.numel() != end.numel():
            raise ValueError(f"sort: start, end and ptr are int64 tensors on the finder's device {self.raw.device}, start and end of one length")
        n = start.numel()
        if ptr is None:
            ptr = torch.tensor([0, n], dtype=torch.int64, device=dev)
        G = ptr.numel() - 1
        per = ptr[1:] - ptr[:-1]
        if G < 0 or (G == 0 and n) or (G > 0 and (int(ptr[0]) != 0 or int(ptr[-1]) != n or bool((per < 0).any()))):
            raise ValueError(f"sort: ptr does not split the {n} ranges into groups (it ascends from 0 to {n})")
        z = lambda k, dt=torch.int64: torch.zeros(k, dtype=dt, device=dev)
        if n == 0 or G == 0:
            return Sorted(z(max(G, 0) + 1), z(0), z(0), z(0), z(0, torch.bool), z(0), z(max(G, 0)), z(max(G, 0)), z(0), 0)
        if bool(((start < 0) | (end < start) | (end > self.n_bytes)).any()):
            raise ValueError(f"sort: a range descends or leaves the corpus of n_bytes = {self.n_bytes}")
        group = torch.repeat_interleave(torch.arange(G, dtype=torch.int64, device=dev), per)
        keys = lambda s, e, d: ops.order_keys(self.raw, self.raw_off, self.cuts, self.slot, s, e, d, ignore_case)
        lcp = lambda s, e, rep, frm: ops.order_lcp(self.raw, self.raw_off, self.cuts, self.slot, s, e, rep, frm, ignore_case)
        return order_ranges(start.contiguous(), end.contiguous(), group, G, keys, lcp, unique, max_rounds, _skip)

    def sort_regex(self, rx, ignore_case: bool = False, unique: bool = False, max_hits: int = 1 << 24) -> Sorted:
        """sort(nonoverlapping(find_regex(rx, max_hits)), ignore_case, unique): per regex its leftmost-longest matches in the order of
        their texts (grep -o RX | sort [-u]).  ignore_case folds the VALUES; how the regex matches is the Regex's own."""
        return self.sort(nonoverlapping(self.find_regex(rx, max_hits)), ignore_case, unique)

    # ------------------------------------------------------------------ from ranges to the corpus without them
    def _edits(self, where: str, what, repl, fill: bool):
        """-> (start, end, sel, rep, rep_off) of substitute / redact: the groups' ranges merged by a stable sort on start, each edit's
        replacement the one of its group.  Every refusal comes in front of every launch."""
        dev = self.dev
        if isinstance(what, RegexFound):
            start, end, ptr = what.offsets, what.offsets + what.lengths, what.ptr
        elif isinstance(what, Lines):
            start, end, ptr = what.start, what.end, what.ptr
        elif isinstance(what, Found):
            raise ValueError(f"{where}: what is a {type(what).__name__}, which has offsets but no lengths; {where} takes a RegexFound, a Lines, the (start, end) of "
                             "spans(), or any (start, end) pair of tensors")
        elif isinstance(what, (tuple, list)) and len(what) in (2, 3) and all(isinstance(t, torch.Tensor) for t in what):
            start, end = (t.reshape(-1) for t in what[:2])
            ptr = what[2].reshape(-1) if len(what) == 3 else None
        else:
            raise ValueError(f"{where}: what is a RegexFound, a Lines, a (start, end) pair or a (start, end, ptr) triple of tensors, got a {type(what).__name__}")
        if any(t.dtype != torch.int64 or t.device != self.raw.device for t in (start, end) + (() if ptr is None else (ptr,))) or start.numel() != end.numel():
            raise ValueError(f"{where}: start, end and ptr are int64 tensors on the finder's device {self.raw.device}, start and end of one length")
        n = start.numel()
        if ptr is None:
            ptr = torch.tensor([0, n], dtype=torch.int64, device=dev)
        G = ptr.numel() - 1
        per = ptr[1:] - ptr[:-1]
        if G < 0 or (G == 0 and n) or (G > 0 and (int(ptr[0]) != 0 or int(ptr[-1]) != n or bool((per < 0).any()))):
            raise ValueError(f"{where}: ptr does not split the {n} ranges into groups (it ascends from 0 to {n})")
        name = "fill" if fill else "repl"
        if isinstance(repl, (bytes, bytearray)):
            reps, one = [bytes(repl)], True
        elif isinstance(repl, (tuple, list)) and all(isinstance(r, (bytes, bytearray)) for r in repl):
            reps, one = [bytes(r) for r in repl], False
            if len(reps) != G:
                raise ValueError(f"{where}: {name} has {len(reps)} entries, what has {G} groups (one bytes for all, or one per group)")
        else:
            raise ValueError(f"{where}: {name} is bytes, or a sequence with one bytes per group, got a {type(repl).__name__}")
        if fill and any(len(r) != 1 for r in reps):
            raise ValueError(f"{where}: fill is one byte (or one byte per group), got lengths {[len(r) for r in reps]}")
        if n and bool(((start < 0) | (end < start) | (end > self.n_bytes)).any()):
            raise ValueError(f"{where}: a range descends or leaves the corpus of n_bytes = {self.n_bytes}")
        if one or G == 0:
            sel = torch.zeros(n, dtype=torch.int64, device=dev)
        else:
            sel = torch.repeat_interleave(torch.arange(G, dtype=torch.int64, device=dev), per)
        order = torch.sort(start, stable=True)[1]
        start, end, sel = start[order].contiguous(), end[order].contiguous(), sel[order].contiguous()
        if n > 1 and bool((start[1:] < end[:-1]).any()):
            raise ValueError(f"{where}: ranges overlap (within a group or between groups); edits may touch, they may not overlap")
        lens = [len(r) for r in reps]
        rep = torch.from_numpy(np.frombuffer(b"".join(reps), dtype=np.uint8).copy()).to(dev)
        rep_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
        return start, end, sel, rep, rep_off

    def _substitute(self, where: str, what, repl, fill: bool, max_bytes: int) -> Substituted:
        start, end, sel, rep, rep_off = self._edits(where, what, repl, fill)
        n, dev = start.numel(), self.dev
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if fill or n == 0:
            out_off[:n] = start
            out_off[n] = self.n_bytes
        else:                                                                    # out_off[i] = start[i] + sum_{j < i} (|R_j| - (end[j] - start[j]))
            grow = (rep_off[1:] - rep_off[:-1])[sel] - (end - start)
            torch.cumsum(grow, 0, out=out_off[1:])
            out_off[:n] += start
            out_off[n] += self.n_bytes
        total = int(out_off[-1]) if n else self.n_bytes
        if total > int(max_bytes):
            raise ValueError(f"{where}: the output holds {total} bytes, which exceeds max_bytes = {max_bytes}")
        data = ops.subst_apply(self.raw, self.raw_off, self.cuts, self.slot, start, end, sel, rep, rep_off, out_off, total, fill)
        return Substituted(data, start, end, sel, out_off, n, self.n_bytes, total)

    def substitute(self, what, repl, max_bytes: int = 1 << 34) -> Substituted:
        """The corpus with every range of `what` replaced (sed 's/RX/repl/g' once the ranges are a regex's; include/hmse_subst.h has the
        definitions).  `what`: a RegexFound (one group per regex), a Lines, a (start, end) pair of int64 device tensors taken as one
        group, or a (start, end, ptr) triple with group j's ranges at [ptr[j] : ptr[j + 1]).  `repl`: bytes, one for all, or a sequence
        with one bytes per group; empty deletes.  The groups' ranges are merged by a stable sort on start: empty ranges insert, several
        at one position in the order given.  One hmse_subst_apply call writes the output in HBM; ingest.ingest_shard takes
        `.data` as it is.  No edits gives the corpus itself.  ValueError in front of every launch for a plain Found or ApproxFound
        (they carry no lengths: use spans()), ranges that overlap (within or between groups; they may touch), descend or leave the
        corpus, a repl that does not match the groups, an output above max_bytes."""
        return self._substitute("substitute", what, repl, False, max_bytes)

    def redact(self, what, fill: bytes = b"*", max_bytes: int = 1 << 34) -> Substituted:
        """substitute in fill mode: every byte of every range becomes the fill byte (one byte, or one per group), so lengths and offsets
        are preserved: n_bytes_out == n_bytes_in."""
        return self._substitute("redact", what, fill, True, max_bytes)

    def substitute_regex(self, rx, repl, max_hits: int = 1 << 24, max_bytes: int = 1 << 34) -> Substituted:
        """substitute(nonoverlapping(find_regex(rx, max_hits)), repl): per regex its leftmost-longest matches replaced, like
        sed -E 's/RX/repl/g'.  Matches of different regexes that overlap raise ValueError."""
        return self.substitute(nonoverlapping(self.find_regex(rx, max_hits)), repl, max_bytes)

    def redact_regex(self, rx, fill: bytes = b"*", max_hits: int = 1 << 24, max_bytes: int = 1 << 34) -> Substituted:
        """redact(nonoverlapping(find_regex(rx, max_hits)), fill): every byte of every match becomes the fill byte."""
        return self.redact(nonoverlapping(self.find_regex(rx, max_hits)), fill, max_bytes)

    # ------------------------------------------------------------------ a whole dictionary in one pass
    def _set_of(self, pset: PatternSet):
        if not isinstance(pset, PatternSet):
            raise ValueError("find: count_set / find_set take a PatternSet (PatternSet(patterns, ignore_case, device))")
        if pset.dev is None or pset.dev != self.dev:
            raise ValueError(f"find: the PatternSet lives on {pset.dev}, the finder on {self.dev}")
        return pset

    def _count_unique(self, ps: PatternSet):
        """-> (occurrences int64[n_unique], in-record hits of the set's scan, its seam hits, [(unique ids, query, in-record hits, seam
        hits) of every group of short patterns])."""
        counts = torch.zeros(ps.n_unique, dtype=torch.int64, device=self.dev)
        n_scan = n_seam = 0
        if ps.n_entries:
            c, n_scan, n_seam = self._count(self._q_set(ps))
            counts += c
        short = []
        for g, off in ps.short_groups():
            q = self._q_group(ps.short_pat, off, ps.ignore_case)
            c, a, b = self._count(q)
            ids = ps.short_ids_d[g: g + len(off) - 1]
            counts[ids] = c
            short.append((ids, q, a, b))
        return counts, n_scan, n_seam, short

    def count_set(self, pset: PatternSet) -> torch.Tensor:
        """Occurrences per pattern of the set, int64[P] on the device: one scan and one seam pass for all patterns of 4 bytes or more
        (plus two count-only launches per 32 distinct patterns of 1..3 bytes); nothing is materialised."""
        ps = self._set_of(pset)
        if ps.n_patterns == 0 or self.n_records == 0:
            return torch.zeros(ps.n_patterns, dtype=torch.int64, device=self.dev)
        return self._count_unique(ps)[0][ps.index_d]

    def find_set(self, pset: PatternSet, max_hits: int = 1 << 24) -> Found:
        """Every occurrence of every pattern of the set.  Counts first: ValueError naming the total and the ten largest counts if the
        total exceeds max_hits."""
        ps = self._set_of(pset)
        dev, n = self.dev, ps.n_patterns
        if n == 0 or self.n_records == 0:
            return self._empty(n)
        cu, n_scan, n_seam, short = self._count_unique(ps)
        counts = cu[ps.index_d]
        total = self._total_within(counts, max_hits, largest_only=True)
        B, ID = ops.FINDSET_ID_BITS, (1 << ops.FINDSET_ID_BITS) - 1
        # unique pattern << 40 | corpus offset (positions stay below 2^40); the 1..3-byte patterns come from the grouped kernels
        keys = [((h & ID) << 40) | (h >> B) for h in self._locate(self._q_set(ps), n_scan, n_seam)]
        for ids, q, a, b in short:
            keys += [(ids[h & 0xFF] << 40) | (h >> 8) for h in self._locate(q, a, b)]
        found = torch.sort(torch.cat(keys))[0] & ((1 << 40) - 1) if keys else torch.zeros(0, dtype=torch.int64, device=dev)
        self._all_located(found.numel(), int(cu.sum()))
        # expand the unique patterns' lists back to the caller's patterns
        ptr_u, ptr = self._ptr(cu), self._ptr(counts)
        src = torch.repeat_interleave(ptr_u[:-1][ps.index_d] - ptr[:-1], counts) + torch.arange(total, dtype=torch.int64, device=dev)
        return Found(ptr, found[src], counts)

    # ------------------------------------------------------------------ regular expressions
    def _regexes(self, rx):
        rxs = [rx] if isinstance(rx, Regex) else list(rx)
        for r in rxs:
            if not isinstance(r, Regex):
                raise ValueError(f"find: count_regex / find_regex take a Regex or a list of them (regex.Regex(pattern, device=...)), got a {type(r).__name__}")
            if r.dev is None or r.dev != self.dev:
                raise ValueError(f"find: the Regex lives on {r.dev}, the finder on {self.dev}")
        return rxs

    def count_regex(self, rx) -> torch.Tensor:
        """Occurrences per regex, int64[P] on the device (`rx`: a Regex, or a list of them, answered one after the other): two
        count-only launches per regex, nothing is materialised."""
        rxs = self._regexes(rx)
        if not rxs or self.n_records == 0:
            return torch.zeros(len(rxs), dtype=torch.int64, device=self.dev)
        return torch.cat([self._count(self._q_regex(r))[0] for r in rxs])

    def find_regex(self, rx, max_hits: int = 1 << 24) -> RegexFound:
        """Every occurrence of every regex, with its length.  Counts first: ValueError naming the counts if their sum exceeds max_hits."""
        qs = [self._q_regex(r) for r in self._regexes(rx)]
        n = len(qs)
        if n == 0 or self.n_records == 0:
            return self._empty(n, RegexFound)
        counted = [self._count(q) for q in qs]
        counts = torch.cat([c[0] for c in counted])
        total = self._total_within(counts, max_hits)
        parts = []
        for q, (c, n_scan, n_seam) in zip(qs, counted):
            found = self._locate(q, n_scan, n_seam)
            if found:
                parts.append(torch.sort(torch.cat(found))[0])                # by corpus offset: one length per start
        h = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=self.dev)
        ptr = self._ptr(counts)
        self._all_located(h.numel(), total)
        return RegexFound(ptr, h >> 8, counts, (h & 0xFF) + 1)                   # the length split: length - 1 is the low byte

    def grep_regex(self, rx, delim: bytes = b"\n", before: int = 0, after: int = 0, reach: int = 1 << 16, max_hits: int = 1 << 24) -> Lines:
        """lines(find_regex(rx, max_hits), delim, before, after, reach): per regex the lines that hold a match's start."""
        _lines_args(delim, before, after, reach)
        return self.lines(self.find_regex(rx, max_hits), delim, before, after, reach)

    # ------------------------------------------------------------------ approximate search
    def _groups_approx(self, patterns, k):
        """_groups for the approximate search: 8 patterns per launch, each with its error bound -> (pat, [(bounds, ks)], n, the
        patterns as bytes).  ValueError before any device work."""
        flat, off = pack_patterns(patterns)
        n = len(off) - 1
        ks = [int(k)] * n if isinstance(k, (int, np.integer)) else [int(v) for v in k]
        if len(ks) != n:
            raise ValueError(f"find_approx: k has {len(ks)} entries for {n} patterns (an int, or one per pattern)")
        for j in range(n):
            m = off[j + 1] - off[j]
            if m > APPROX_MAX_LEN:
                raise ValueError(f"find_approx: pattern {j} has {m} bytes; an approximate pattern has 1 to HMSE_APPROX_MAX_LEN = {APPROX_MAX_LEN}")
            if not 0 <= ks[j] <= APPROX_MAX_K:
                raise ValueError(f"find_approx: k = {ks[j]} of pattern {j} lies outside 0..HMSE_APPROX_MAX_K = {APPROX_MAX_K}")
            if ks[j] >= m:
                raise ValueError(f"find_approx: k = {ks[j]} of pattern {j} is not below its length {m} (every position would match)")
        pat = torch.from_numpy(flat.copy()).to(self.dev) if n else None
        blob = flat.tobytes()
        groups = [(off[g: min(g + APPROX_GROUP, n) + 1], ks[g: g + APPROX_GROUP]) for g in range(0, n, APPROX_GROUP)]
        return pat, groups, n, tuple(blob[off[j]: off[j + 1]] for j in range(n))

    def _q_approx(self, pat, off, ks, ignore_case) -> _Query:
        return _Query(lambda cap: ops.approx_scan(self.raw, self.raw_off, self.mult, pat, off, ks, ignore_case, hits_cap=cap),
                      lambda cap: ops.approx_seams(self.raw, self.raw_off, self.cuts, self.slot, pat, off, ks, ignore_case, hits_cap=cap),
                      lambda *a: ops.find_place(*a), 8)                          # (the hit word's low byte: errors << 3 | pattern)

    def count_approx(self, patterns, k, ignore_case: bool = False) -> torch.Tensor:
        """Per pattern the ends within k edits of it (module docstring), int64[P] on the device: two count-only launches per 8
        patterns, nothing is materialised.  k: an int, or one per pattern."""
        pat, groups, n, _ = self._groups_approx(patterns, k)
        if n == 0 or self.n_records == 0:
            return torch.zeros(n, dtype=torch.int64, device=self.dev)
        return torch.cat([self._count(self._q_approx(pat, off, ks, ignore_case))[0] for off, ks in groups])

    def find_approx(self, patterns, k, ignore_case: bool = False, max_hits: int = 1 << 24) -> ApproxFound:
        """Every end within k edits of every pattern, with its errors; `offsets` are the matches' LAST bytes.  Counts first:
        ValueError naming the counts if their sum exceeds max_hits."""
        pat, groups, n, pats = self._groups_approx(patterns, k)
        z = lambda m: torch.zeros(m, dtype=torch.int64, device=self.dev)
        if n == 0 or self.n_records == 0:
            return ApproxFound(z(n + 1), z(0), z(n), z(0), pats, bool(ignore_case))
        qs = [self._q_approx(pat, off, ks, ignore_case) for off, ks in groups]
        counted = [self._count(q) for q in qs]
        counts = torch.cat([c[0] for c in counted])
        total = self._total_within(counts, max_hits)
        offs, errs = [], []
        for q, (c, n_scan, n_seam) in zip(qs, counted):
            found = self._locate(q, n_scan, n_seam)
            if found:
                h = torch.cat(found)
                order = torch.sort(((h & 7) << 56) | (h >> 8))[1]             # by (pattern, offset): offsets stay below 2^56
                offs.append((h >> 8)[order])
                errs.append(((h >> 3) & 31)[order])                           # the errors split out of the low byte
        offsets, errors = (torch.cat(offs), torch.cat(errs)) if offs else (z(0), z(0))
        self._all_located(offsets.numel(), total)
        return ApproxFound(self._ptr(counts), offsets, counts, errors, pats, bool(ignore_case))

    def spans(self, found: ApproxFound):
        """-> (start, end) int64 device tensors, aligned with found.offsets: occurrence i is corpus[start[i] : end[i]], end = offsets + 1
        and start the LARGEST one whose text has the occurrence's errors — the shortest best match.  The pair is what text() accepts.
        One hmse_approx_spans call per 8 patterns.  ValueError for a hit that cannot be (an offset outside the corpus, errors that no
        text ending there attains)."""
        if not isinstance(found, ApproxFound) or len(found.patterns) != found.counts.numel():
            raise ValueError("spans: found is the ApproxFound of find_approx")
        end = found.offsets + 1
        start = torch.empty_like(end)
        if end.numel() == 0:
            return start, end
        pat, groups, n, _ = self._groups_approx(list(found.patterns), 0)
        ptr = found.ptr.tolist()
        for g, (off, _) in enumerate(groups):
            a, b = ptr[g * APPROX_GROUP], ptr[min((g + 1) * APPROX_GROUP, n)]
            if a == b:
                continue
            j = torch.repeat_interleave(torch.arange(len(off) - 1, dtype=torch.int64, device=self.dev), found.counts[g * APPROX_GROUP: (g + 1) * APPROX_GROUP])
            words = (found.offsets[a:b] << 8) | (found.errors[a:b] << 3) | j
            s, st = ops.approx_spans(self.raw, self.raw_off, self.cuts, self.slot, pat, off, found.ignore_case, words.contiguous())
            if st & 1:
                raise ValueError("spans: an occurrence lies outside the corpus or has errors that no text ending there attains")
            start[a:b] = s
        return start, end

    def grep_approx(self, patterns, k, ignore_case: bool = False, delim: bytes = b"\n", before: int = 0, after: int = 0, reach: int = 1 << 16,
                    max_hits: int = 1 << 24) -> Lines:
        """lines(best_ends(find_approx(patterns, k, ignore_case, max_hits)), delim, before, after, reach): per pattern the lines that
        hold the last byte of a best end."""
        _lines_args(delim, before, after, reach)
        return self.lines(best_ends(self.find_approx(patterns, k, ignore_case, max_hits)), delim, before, after, reach)

    nonoverlapping = staticmethod(lambda found: nonoverlapping(found))


def nonoverlapping(found: RegexFound) -> RegexFound:
    """Per pattern the first occurrence, then each next one that starts at or behind the previous kept one's end: leftmost-longest,
    like grep -o.  Torch plumbing on the tensors' device: searchsorted for every occurrence's successor, then pointer doubling from
    each pattern's first occurrence — no host loop over the occurrences."""
    off, ln = found.offsets, found.lengths
    n, dev, P = off.numel(), off.device, found.counts.numel()
    if n == 0:
        return found
    pat = torch.repeat_interleave(torch.arange(P, dtype=torch.int64, device=dev), found.counts)
    key = (pat << 56) | off                                                      # ascending: by pattern, then offset (offsets stay below 2^56)
    nxt = torch.searchsorted(key, key + ln)                                      # the first occurrence of the pattern at or behind the end
    nxt = torch.where(nxt < found.ptr[1:][pat], nxt, torch.full_like(nxt, n))    # none in this pattern: the sink n
    nxt = torch.cat([nxt, torch.full((1,), n, dtype=torch.int64, device=dev)])
    kept = torch.zeros(n + 1, dtype=torch.bool, device=dev)
    kept[found.ptr[:-1][found.counts > 0]] = True
    for _ in range(max(1, int(n).bit_length())):                                 # after k trips: everything within 2^k - 1 hops of a start is marked
        kept[nxt[torch.nonzero(kept).reshape(-1)]] = True
        nxt = nxt[nxt]
    kept = kept[:n]
    counts = torch.bincount(pat[kept], minlength=P)
    ptr = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=ptr[1:])
    return RegexFound(ptr, off[kept], counts, ln[kept])


def best_ends(found: ApproxFound) -> ApproxFound:
    """Per pattern the ascending offsets fall into runs of consecutive integers — the neighbouring ends of one fuzzy match; of every
    run the end with the fewest errors is kept, the leftmost on ties.  Torch plumbing on the tensors' device: run ids by a prefix sum,
    the minimum of (errors, offset) per run by scatter_reduce — no host loop over the occurrences."""
    off, err = found.offsets, found.errors
    n, dev, P = off.numel(), off.device, found.counts.numel()
    if n == 0:
        return found
    pat = torch.repeat_interleave(torch.arange(P, dtype=torch.int64, device=dev), found.counts)
    new = torch.ones(n, dtype=torch.bool, device=dev)
    new[1:] = (pat[1:] != pat[:-1]) | (off[1:] != off[:-1] + 1)
    run = torch.cumsum(new, 0) - 1
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    key = (err << 56) | idx                                                      # fewest errors, then leftmost (indices ascend with offsets)
    best = torch.full((int(run[-1]) + 1,), (1 << 62), dtype=torch.int64, device=dev).scatter_reduce_(0, run, key, "amin")
    keep = best & ((1 << 56) - 1)
    counts = torch.bincount(pat[keep], minlength=P)
    ptr = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=ptr[1:])
    return ApproxFound(ptr, off[keep], counts, err[keep], found.patterns, found.ignore_case)


def find_approx(store, patterns, k, device, ignore_case: bool = False, max_hits: int = 1 << 24, verify: bool = True) -> ApproxFound:
    """One-off form of StoreFinder(store, device, verify).find_approx(patterns, k, ignore_case, max_hits)."""
    return StoreFinder(store, device, verify).find_approx(patterns, k, ignore_case, max_hits)


def grep_approx(store, patterns, k, device, ignore_case: bool = False, delim: bytes = b"\n", before: int = 0, after: int = 0,
                reach: int = 1 << 16, max_hits: int = 1 << 24, verify: bool = True) -> Lines:
    """One-off form of StoreFinder(store, device, verify).grep_approx(patterns, k, ignore_case, delim, before, after, reach, max_hits)."""
    _lines_args(delim, before, after, reach)
    return StoreFinder(store, device, verify).grep_approx(patterns, k, ignore_case, delim, before, after, reach, max_hits)


def find_regex(store, rx, device, max_hits: int = 1 << 24, verify: bool = True) -> RegexFound:
    """One-off form of StoreFinder(store, device, verify).find_regex(rx, max_hits)."""
    return StoreFinder(store, device, verify).find_regex(rx, max_hits)


def tally_regex(store, rx, device, ignore_case: bool = False, top=None, max_hits: int = 1 << 24, verify: bool = True) -> Tally:
    """One-off form of StoreFinder(store, device, verify).tally_regex(rx, ignore_case, top, max_hits)."""
    return StoreFinder(store, device, verify).tally_regex(rx, ignore_case, top, max_hits)


def sort_regex(store, rx, device, ignore_case: bool = False, unique: bool = False, max_hits: int = 1 << 24, verify: bool = True) -> Sorted:
    """One-off form of StoreFinder(store, device, verify).sort_regex(rx, ignore_case, unique, max_hits)."""
    return StoreFinder(store, device, verify).sort_regex(rx, ignore_case, unique, max_hits)


def substitute_regex(store, rx, repl, device, max_hits: int = 1 << 24, max_bytes: int = 1 << 34, verify: bool = True) -> Substituted:
    """One-off form of StoreFinder(store, device, verify).substitute_regex(rx, repl, max_hits, max_bytes)."""
    return StoreFinder(store, device, verify).substitute_regex(rx, repl, max_hits, max_bytes)


def redact_regex(store, rx, device, fill: bytes = b"*", max_hits: int = 1 << 24, max_bytes: int = 1 << 34, verify: bool = True) -> Substituted:
    """One-off form of StoreFinder(store, device, verify).redact_regex(rx, fill, max_hits, max_bytes)."""
    return StoreFinder(store, device, verify).redact_regex(rx, fill, max_hits, max_bytes)


def grep_regex(store, rx, device, delim: bytes = b"\n", before: int = 0, after: int = 0, reach: int = 1 << 16, max_hits: int = 1 << 24,
               verify: bool = True) -> Lines:
    """One-off form of StoreFinder(store, device, verify).grep_regex(rx, delim, before, after, reach, max_hits)."""
    _lines_args(delim, before, after, reach)
    return StoreFinder(store, device, verify).grep_regex(rx, delim, before, after, reach, max_hits)


def find_set(store, patterns, device, ignore_case: bool = False, max_hits: int = 1 << 24, verify: bool = True) -> Found:
    """One-off form of StoreFinder(store, device, verify).find_set(PatternSet(patterns, ignore_case, device), max_hits)."""
    return StoreFinder(store, device, verify).find_set(PatternSet(patterns, ignore_case, device), max_hits)


def find(store, patterns, device, ignore_case: bool = False, max_hits: int = 1 << 24, verify: bool = True) -> Found:
    """One-off form of StoreFinder(store, device, verify).find(patterns, ignore_case, max_hits)."""
    return StoreFinder(store, device, verify).find(patterns, ignore_case, max_hits)


def grep(store, patterns, device, ignore_case: bool = False, delim: bytes = b"\n", before: int = 0, after: int = 0, reach: int = 1 << 16,
         max_hits: int = 1 << 24, verify: bool = True) -> Lines:
    """One-off form of StoreFinder(store, device, verify).grep(patterns, ignore_case, delim, before, after, reach, max_hits)."""
    _lines_args(delim, before, after, reach)
    return StoreFinder(store, device, verify).grep(patterns, ignore_case, delim, before, after, reach, max_hits)
