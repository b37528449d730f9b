"""Host: the promises of tests/grid_caps.py, proved on the CPU, and an audit of the kernel sources for capped launches without a row.

Per builder: the input needs two full trips and a ragged last one at the cap read from the source; its planted items lie in the first
trip, the second and the ragged tail; the CPU reference the GPU test compares with agrees with an independent one where there is one
(hashlib / the oracle's SHA-256, zlib's inflate / the oracle's, zlib.crc32 / a table of tiny contents, bytes.find over the whole input /
over the planted places)."""
import zlib

import numpy as np
import pytest

import find_ref
import grid_caps as G
import similarity_ref


@pytest.fixture(scope="module")
def K():
    return G.kernel_constants()


def _three_trips(count, cap, unit=1):
    """Two full trips and a ragged third."""
    return G.trips(count, cap, unit) == 3 and count % (cap * unit) != 0 and count > 2 * cap * unit


def _in_every_trip(trip):
    return set(np.unique(trip).tolist()) == {0, 1, 2}


# ---- the table and the audit ------------------------------------------------------------------------------------------------------------
def test_every_row_names_its_test_and_the_must_have_rows_name_new_ones(K):
    import os
    rows = G.rows(K)
    here = os.path.dirname(os.path.abspath(__file__))
    for r in rows:
        path, name = r.test.split("::")
        with open(os.path.join(os.path.dirname(here), path)) as f:
            assert ("def %s(" % name) in f.read(), r
        assert r.cap >= 512 and r.unit >= 1 and G.crossing(r) == r.cap * r.unit + 1
        assert not r.must or r.test.startswith(G.NEW), r
    must = {kn for r in rows if r.must for kn in r.kernels}
    assert must == {"l3_sha256_kernel", "ord_hist_kernel", "l1_inflate_lanes_kernel", "l4_minhash_kernel", "qy_score_kernel", "crc32_kernel",
                    "find_scan_kernel", "findset_scan_kernel", "tables_validate_kernel"}
    assert not must & {kn for _, kn in G.EXEMPT}                                       # no must-have row among the exemptions
    # the crossings the sources imply
    by = {r.kernels[0]: G.crossing(r) for r in rows}
    assert by["l3_sha256_kernel"] == 262145 and by["l1_inflate_lanes_kernel"] == 131073 and by["l1_inflate_kernel"] == 8193
    assert by["l4_minhash_kernel"] == 16385 and by["qy_score_kernel"] == 8193 and by["crc32_kernel"] == 4097
    assert by["find_scan_kernel"] == (64 << 20) + 1 and by["findset_scan_kernel"] == (32 << 20) + 1 and by["tables_validate_kernel"] == 524289


def test_every_capped_launch_has_a_row_or_a_reason(K):
    """The capped-grid and stride sites of hmse_amd/csrc: each belongs to a kernel with a row, or to one with a written reason, or is
    listed as no grid at all.  A capped kernel added without a row fails here; so does an entry that no longer matches a site."""
    sites = G.capped_sites()
    assert len(sites) > 60
    covered = {(r.file, kn) for r in G.rows(K) for kn in r.kernels}
    seen = set()
    for file, line, kernel, text in sites:
        key = (file, kernel) if kernel else (file, text)
        seen.add(key)
        if kernel is None:
            assert key in G.NOT_A_GRID, "%s:%d: `%s` looks like a capped grid; give it a row in tests/grid_caps.py or list it" % (file, line, text)
        else:
            assert key in covered or key in G.EXEMPT, "%s:%d: %s has a capped or strided grid and no row in tests/grid_caps.py" % (file, line, kernel)
    assert not (covered & set(G.EXEMPT)), covered & set(G.EXEMPT)
    assert covered <= seen and set(G.EXEMPT) <= seen and G.NOT_A_GRID <= seen, (covered - seen, set(G.EXEMPT) - seen, G.NOT_A_GRID - seen)
    assert all(len(reason) > 20 for reason in G.EXEMPT.values())


SAMPLE = """\
__global__ __launch_bounds__(256) void stride_kernel(const uint32_t* p, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;      // one
  for (uint64_t i = blockIdx.x; i < n; i += stride) { }
}
template <int NT>
__global__ void loop_kernel(uint64_t n) {
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) { }
  // a comment that names gridDim.x and if (nb > 9) nb = 9; is not read
}
static uint32_t tail_blocks(uint64_t cap) { const uint64_t b = (cap + 255) / 256; return (uint32_t)(b > 1024 ? 1024 : b); }
int entry(uint64_t n, uint64_t lo, uint64_t hi, hipStream_t stream) {
  if (lo > hi) lo = hi;
  uint64_t nb = (n + 255) / 256;
  if (nb > 2048) nb = 2048;
  PROF_BEGIN(0, stream);
  stride_kernel<<<dim3((uint32_t)nb), dim3(256), 0, stream>>>(nullptr, n);
  uint64_t m = (n + 3) / 4;
  if (m > MY_MAX_BLOCKS) m = MY_MAX_BLOCKS;
  loop_kernel<256><<<dim3((uint32_t)m), dim3(256), 0, stream>>>(n);
  const dim3 grid((uint32_t)(n < MY_CAP ? n : MY_CAP));
  RX_KERNEL(scan_kernel)<<<grid, dim3(256), 0, stream>>>(n);
  loop_kernel<64><<<dim3((uint32_t)((n + 3) / 4 < 16384 ? (n + 3) / 4 : 16384)), dim3(64), 0, stream>>>(n);
  uint32_t w = left < MY_TRIP ? (uint32_t)left : MY_TRIP;
  return 0;
}









int late(uint64_t n, uint64_t limit) {
  if (n > limit) n = limit;
  x = y < z ? y : z;
  return 0;
}
"""


def test_the_audit_sees_each_form_of_a_capped_grid():
    """capped_sites() on a sample: the three forms, the kernel each belongs to (launched next, through a template or RX_KERNEL, or the one
    the line stands in), comments skipped, clamps to variables without a launch skipped, constant clamps without a launch reported."""
    got = [(line, kernel, text) for _, line, kernel, text in G.capped_sites({"sample.hip": SAMPLE})]
    assert got == [
        (2, "stride_kernel", "const uint64_t stride = (uint64_t)gridDim.x * 256;"),
        (7, "loop_kernel", "for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) { }"),
        (10, "stride_kernel", "b > 1024 ? 1024 : b"),                                  # (a helper: the launch found is merely the next one)
        (12, "stride_kernel", "if (lo > hi) lo = hi;"),                               # a clamp to a variable is kept when a launch follows
        (14, "stride_kernel", "if (nb > 2048) nb = 2048;"),
        (18, "loop_kernel", "if (m > MY_MAX_BLOCKS) m = MY_MAX_BLOCKS;"),
        (20, "scan_kernel", "n < MY_CAP ? n : MY_CAP"),
        (22, "loop_kernel", "(n + 3) / 4 < 16384 ? (n + 3) / 4 : 16384"),
        (23, None, "left < MY_TRIP ? (uint32_t)left : MY_TRIP"),
    ]


# ---- the builders -----------------------------------------------------------------------------------------------------------------------
def test_sha_chunks(K, orc):
    data, cuts, f = G.sha_chunks(K)
    assert f["count"] == len(cuts) - 1 == 2 * 262144 + 77 and _three_trips(f["count"], K["SHA_BLOCKS"], K["SHA_NT"])
    assert _three_trips(f["count"], K["ORD_BLOCKS"], K["ORD_NT"]) and f["count"] > 4096
    # ops.l3_sha256 asks for a workspace that holds the order table (the "longest-first" run is one), 256 bytes do not ("index-order")
    from hmse_amd import IngestConfig, ops
    assert ops.workspace_bytes(ops.STAGE_SHA, f["count"], IngestConfig()) >= G.sha_order_workspace(K, f["count"]) > 256
    lens = np.diff(cuts)
    assert cuts[-1] == data.size and 0 < lens[-1] < 64                                          # the last block is read byte by byte
    assert set(range(131)) <= set(lens.tolist()) and {4097, 32768} <= set(lens.tolist())
    assert _in_every_trip(G.trip_of(f["long_at"], f["lanes"])) and f["long_at"].size > 500
    # a long chunk directly in front of a short one and of an empty one
    nxt = lens[np.minimum(f["long_at"] + 1, lens.size - 1)]
    assert (nxt < 56).any() and ((nxt >= 56) & (nxt < 64)).any() and (nxt % 64 == 0).any()
    assert 30 << 20 < data.size < 48 << 20
    want = G.sha_reference(data, cuts)
    assert np.array_equal(want, orc.sha256_chunks(data, cuts.astype(np.uint64)))


def test_inflate_records(K, orc):
    recs, f = G.inflate_records(K)
    n, lanes = f["count"], f["lanes"]
    assert n == len(recs) == 2 * lanes + 64 * 37 + 5 and lanes == 131072 and _three_trips(n, K["IFL_BLOCKS"], K["IFL_LANES"])
    assert n >= K["IFL_WIDE_MIN"]                                                                # the automatic choice is this decoder
    base = f["base"]
    full, delta = np.flatnonzero(base < 0), np.flatnonzero(base >= 0)
    assert full.size > lanes                                                                     # some lane takes FULL after FULL
    assert 0.07 * n < delta.size < 0.12 * n and (base[delta] < delta).all()                      # every base has a smaller index
    assert (base[base[delta]] >= 0).sum() > 1000                                                 # chains
    assert 0.02 * n < f["damaged"].size < 0.04 * n
    for idx in (full, delta, f["damaged"]):
        assert _in_every_trip(G.trip_of(idx, lanes))
    assert max(r[1] for r in recs) == 600 and min(r[1] for r in recs) == 0
    # the oracle's decisions and bytes against zlib's, on every record zlib takes
    streams, off, kind, b, raw_len = G.pack_records(recs)
    raw, raw_off, ok = orc.inflate_chunks(streams, off, kind, b, raw_len)
    assert 0.95 * n < ok.sum() < n
    clean = np.ones(n, bool)                                                                     # undamaged, and so is its chain of bases
    clean[f["damaged"]] = False
    for i in delta.tolist():
        clean[i] &= clean[base[i]]
    assert ok[clean].all() and clean.sum() > 0.9 * n
    blob = raw.tobytes()
    got = lambda i: blob[int(raw_off[i]): int(raw_off[i + 1])]
    for i in np.flatnonzero(clean)[:: 7].tolist():
        assert got(i) == f["raws"][i], i
    for i in np.flatnonzero(~clean)[:: 3].tolist():                                              # zlib, asked the same question
        s, m, bi = recs[i]
        if bi >= 0 and not ok[bi]:
            assert not ok[i], i
            continue
        try:
            d = zlib.decompressobj(-15, zdict=got(bi)) if bi >= 0 else zlib.decompressobj(-15)
            out = d.decompress(s)
            good = d.eof and not d.unused_data and len(out) == m
        except zlib.error:
            good = False
        assert bool(ok[i]) == good and (not good or got(i) == out), i


def test_minhash_chunks(K):
    data, cuts, f = G.minhash_chunks(K)
    lens = np.diff(cuts)
    assert f["count"] == lens.size == 2 * K["MH_GRID"] + 9 and _three_trips(f["count"], K["MH_GRID"])
    assert lens.min() == 64 and lens.max() == 300 and cuts[-1] == data.size and data.size < 8 << 20
    assert np.unique(lens).size == 237


def test_query_signatures(K):
    S, Q, f = G.query_signatures(K)
    n = f["count"]
    assert n == len(Q) == 2 * K["QY_GRID"] + 45 and _three_trips(n, K["QY_GRID"])
    ids, sc, nh, nc = similarity_ref.search(S, Q, f["bands"], 8)
    kind = f["kind"]
    assert (nc[kind == "none"] == 0).all() and (nc[kind == "crowd"] >= f["crowd"].size).all() and f["crowd"].size > K["QY_CAP"]
    assert ((nc[kind == "near"] >= 1) & (nc[kind == "near"] <= 4)).all() and (nc[kind == "near"] == 4).any()
    # every resident workgroup starts on a crowd query; the later trips mix all three kinds
    assert (kind[: K["QY_GRID"]] == "crowd").all() and _in_every_trip(G.trip_of(np.flatnonzero(kind == "crowd"), K["QY_GRID"]))
    for name in ("none", "near"):
        assert set(G.trip_of(np.flatnonzero(kind == name), K["QY_GRID"]).tolist()) == {1, 2}
    # the threshold a crowd query leaves behind lies above every near query's hits: after the first QY_CAP candidates of the run (the
    # crowd in id order) the buffer is reduced to top_k and the threshold is the top_k-th best score of those; the largest top_k is 64
    crowd_q = np.flatnonzero(kind == "crowd")
    first = S[f["crowd"][: K["QY_CAP"]]]
    kth = np.array([np.sort((first == Q[q]).sum(1))[-64] for q in crowd_q[:: 16]])
    near_q = np.flatnonzero(kind == "near")
    near_best = sc[near_q].max(1)
    assert (nh[near_q] >= 1).all() and 32 <= near_best.min() and near_best.max() < 48 < kth.min()
    # a crowd query's candidates have many different scores, the best eight are not the first eight of the run
    q = int(np.flatnonzero(kind == "crowd")[3])
    scores = (S[f["crowd"]] == Q[q]).sum(1)
    assert np.unique(scores).size > 50 and sorted(ids[q].tolist()) != sorted(f["crowd"][:8].tolist())
    # neighbours in the hand-out are of different kinds
    later = kind[K["QY_GRID"]:]
    assert (later[:-1] != later[1:]).mean() > 0.8


def test_crc_ranges(K):
    data, cuts, f = G.crc_ranges(K)
    lens = np.diff(cuts)
    assert f["count"] == lens.size == 2 * K["EX_MAX_BLOCKS"] + 33 and _three_trips(f["count"], K["EX_MAX_BLOCKS"])
    assert set(range(201)) <= set(lens.tolist()) and cuts[-1] == data.size
    assert _in_every_trip(G.trip_of(f["long_at"], K["EX_MAX_BLOCKS"])) and (lens[f["long_at"]] > 4096).all()
    want = G.crc_reference(data, cuts)
    assert want[0] == 0 and want[1] == zlib.crc32(data[:1].tobytes())


def test_many_tiny_ranges(K):
    data, cuts, f = G.many_tiny_ranges(K)
    assert f["count"] == len(cuts) - 1 and _three_trips(f["count"], K["EX_MAX_BLOCKS"], K["EX_CNT"])
    assert G.trip_of(f["bad_at"], f["per_trip"]).tolist() == [1, 2]
    want = G.tiny_crc_reference(data, cuts)
    blob = data.tobytes()
    for i in list(range(0, f["count"], 997)) + f["bad_at"]:
        assert want[i] == zlib.crc32(blob[int(cuts[i]): int(cuts[i + 1])])


@pytest.mark.parametrize("which", ["find", "findset"])
def test_scan_inputs(K, which):
    tile, cap = (K["FIND_TILE"], K["FIND_MAX_BLOCKS"]) if which == "find" else (K["FSET_TILE"], K["FSET_MAX_BLOCKS"])
    pats = G.FIND_MANY_PATTERNS if which == "find" else G.FSET_PATTERNS
    raw, raw_off, f = G.scan_input(tile, cap, pats, seed=71 if which == "find" else 73)
    assert f["tiles"] == 2 * cap + 3 and _three_trips(f["tiles"], cap) and raw.size % tile == 123 and raw_off[-1] == raw.size
    assert len(G.FIND_FEW_PATTERNS) == K["FIND_FEW"] < len(G.FIND_MANY_PATTERNS) <= 32 and all(len(p) >= 4 for p in G.FSET_PATTERNS)
    assert _in_every_trip(f["trip_of_place"]) and len(f["places"]) > 1000
    places = sorted(f["places"])
    assert all(a + la <= b for (a, la), (b, _) in zip(places, places[1:]))                       # no two planted texts touch
    for B in (cap * tile, 2 * cap * tile):                                                      # across the seam of two trips
        assert any(o < B < o + ln for o, ln in places)
        assert any(B - tile < o and o + ln <= B for o, ln in places) and any(B <= o and o + ln < B + tile for o, ln in places)
    assert any((o + ln) % tile == 0 for o, ln in places) and any(o % tile == 0 for o, ln in places)
    assert any(o + ln == raw.size for o, ln in places)
    assert np.count_nonzero(raw != G.FILLER) == sum(ln for _, ln in places)
    # bytes.find over the whole input finds what the look at the planted places finds
    blob = raw.tobytes()
    for group, ic in ((G.FIND_FEW_PATTERNS, False), (pats, False)) if which == "find" else ((pats, False), (pats, True)):
        hits, counts = G.planted_hits(raw, raw_off, f["places"], group, ic)
        whole, whole_counts = find_ref.scan_hits(blob, raw_off, group, ic)
        assert hits == whole and counts == whole_counts and all(c > 0 for c in counts)
        assert _in_every_trip(G.trip_of(np.array([o for o, _ in hits]) // tile, cap))
        assert (raw.size - len(group[0]), 0) in hits
        if ic:
            assert len(hits) > len(G.planted_hits(raw, raw_off, f["places"], group, False)[0])
    cut = f["cut_place"]
    assert raw_off[1] == raw_off[2] == cut + 2                                                   # a record ends two bytes into a planted text
    assert not any(o == cut and len(pats[j]) > 2 for o, j in G.planted_hits(raw, raw_off, f["places"], pats)[0])


@pytest.mark.parametrize("which", ["find", "findset"])
def test_many_records(K, which):
    cap, nt = (K["FIND_MAX_BLOCKS"], K["FIND_NT"]) if which == "find" else (K["FSET_VALIDATE_BLOCKS"], K["FSET_NT"])
    raw, raw_off, f = G.many_records(cap * nt)
    per = f["per_trip"]
    assert f["count"] == len(raw_off) - 1 and per == (524288 if which == "find" else 1048576) and _three_trips(f["count"], cap, nt)
    assert G.trip_of(f["bad_at"], per).tolist() == [1, 2] and all(raw_off[i] < raw_off[i + 1] for i in f["bad_at"])
    assert _in_every_trip(f["trip_of_place"])
    hits, counts = G.planted_hits(raw, raw_off, f["places"], [f["pattern"]])
    whole, whole_counts = find_ref.occurrences(raw.tobytes(), f["pattern"]), None
    rec = np.searchsorted(raw_off, whole, side="right") - 1
    inside = [(o, 0) for o, r in zip(whole, rec.tolist()) if o + 4 <= raw_off[r + 1]]
    assert hits == inside and 100 < len(hits) < len(whole) == len(f["places"])                  # most cross a record's end


@pytest.mark.parametrize("which", ["find", "findset"])
def test_seam_corpora(K, which):
    per = K["FIND_MAX_BLOCKS"] * K["FIND_NT"] if which == "find" else K["FSET_SEAMS_BLOCKS"] * K["FSET_NT"]
    corpus, cuts, pats, f = G.seam_corpus(per, 255, seed=79 if which == "find" else 83)
    assert max(len(p) for p in pats) == 256 and min(len(p) for p in pats) >= 4
    assert f["count"] == (len(cuts) - 1) * 255 and _three_trips(f["count"], per) and cuts[-1] == len(corpus)
    assert _in_every_trip(f["trip_of_place"])
    inside, seam = find_ref.split(corpus, pats, cuts)
    assert len({j for _, j in seam}) == len(pats) and (len(corpus) - 256, 0) in seam
    assert sum(1 for _, j in seam if j == 0) >= f["planted_at"].size


def test_many_ranges(K):
    assert (K["LINES_MAX_BLOCKS"], K["LINES_NT"]) == (K["TALLY_MAX_BLOCKS"], K["TALLY_NT"])         # one input serves both
    per = K["LINES_MAX_BLOCKS"] * K["LINES_NT"]
    corpus, cuts, start, end, rep, f = G.many_ranges(per)
    n = f["count"]
    assert n == start.size == 2 * per + 77 and _three_trips(n, K["LINES_MAX_BLOCKS"], K["LINES_NT"]) and cuts[-1] == corpus.size
    assert (start <= end).all() and end.max() == corpus.size and (rep < n).all() and G.trip_of(f["bad_at"], per).tolist() == [1, 2]
    out, out_off = G.gathered(corpus, start, end)
    same = G.same_ranges(corpus, start, end, rep)
    blob = corpus.tobytes()
    assert out.tobytes()[: 4000] == b"".join(blob[a: b] for a, b in zip(start[:2000].tolist(), end[:2000].tolist()))[: 4000]
    for i in list(range(0, n, 1009)) + f["bad_at"] + [n - 1]:
        assert out[out_off[i]: out_off[i + 1]].tobytes() == blob[start[i]: end[i]]
        assert same[i] == (blob[start[i]: end[i]] == blob[start[rep[i]]: end[rep[i]]])
    assert 0.2 < same.mean() < 0.8


def test_tiny_chunks(K):
    data, cuts, f = G.tiny_chunks(K)
    assert f["per_trip"] == 65536 and f["count"] == len(cuts) - 1 and _three_trips(f["count"], K["GATHER_BLOCKS"], K["GATHER_WAVES"])
    assert cuts[-1] == data.size and np.diff(cuts).min() == 2 and np.diff(cuts).max() == 40
