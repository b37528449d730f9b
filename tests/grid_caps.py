"""Every launch whose grid stops growing at a fixed size, and an input that takes each one past that size twice.

A capped grid does the work beyond its cap in further trips: a grid-stride loop, or persistent lanes, wavefronts or workgroups that pull
the next item from a device counter.  State carried from one trip into the next (registers not set again, an LDS table reused, a
prefetch in flight, a tail mask computed for trip 0) can only go wrong there, and the generated-text tests stay below most caps.

Pure numpy and the standard library, seeded, no device.  ROWS is the table: one row per capped launch with its cap and unit read from
the kernel sources, the smallest input with a second trip, and the GPU test that crosses it.  Every builder returns its input together
with the facts it promises (the count, the number of trips, where its planted items lie); tests/test_grid_caps_host.py proves the
promises and audits the sources for capped launches that have no row, tests/test_gpu_grid_caps.py runs the inputs through the kernels."""
from __future__ import annotations

import os
import random
import re
import zlib
from collections import namedtuple

import numpy as np

from conftest import words_text

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc")
NEW = "tests/test_gpu_grid_caps.py::"


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, src, times=1):
    """The one value `pattern` captures in `src`, found exactly `times` times (a renamed or duplicated constant fails here)."""
    found = re.findall(pattern, src)
    assert len(found) == times and len(set(found)) == 1, (pattern, found)
    v = found[0]
    return int(v) if isinstance(v, str) else tuple(int(x) for x in v)


def _const(src, name):
    return _one(r"constexpr (?:int|uint32_t|uint64_t) %s = (\d+)u?;" % name, src)


def kernel_constants() -> dict:
    """Every cap and every per-block unit of ROWS, from where the kernels keep them."""
    sha, ifl, mh, qy, ex = _src("l3_sha256.hip"), _src("l1_inflate.hip"), _src("l4_minhash.hip"), _src("l4_query.hip"), _src("export.hip")
    fd, fs, cm, ln, ty = _src("find.hip"), _src("findset.hip"), _src("chunkmap.h"), _src("lines.hip"), _src("tally.hip")
    gz, bt, abi = _src("gunzip.hip"), _src("bandtable.hip"), _src("abi.hip")
    k = {}
    # SHA-256: both entry points cap the hash grid and the histogram grid alike; 256 lanes a workgroup, a chunk a lane
    k["SHA_BLOCKS"] = _one(r"if \(blocks > (\d+)\) blocks = \1;", sha, 2)
    k["ORD_BLOCKS"] = _one(r"if \(hb > (\d+)\) hb = \1;", sha, 2)
    k["SHA_NT"] = _one(r"l3_sha256_kernel<<<dim3\(\(uint32_t\)blocks\), dim3\((\d+)\)", sha, 2)
    k["ORD_NT"] = _one(r"ord_hist_kernel<<<dim3\(\(uint32_t\)hb\), dim3\((\d+)\)", sha, 2)
    assert re.search(r"ws_bytes >= hmse_l3_sha256_workspace_bytes_impl\(n_chunks\) && n_chunks > 4096", sha)      # else: index order
    assert re.search(r"hmse_l3_sha256_workspace_bytes_impl\(uint64_t n_chunks\) \{ return 256 \+ ORD_BINS \* 4 \+ hmse_align_up\(\(size_t\)n_chunks \* 4, 256\); \}", sha)
    k["ORD_BINS"] = _const(sha, "ORD_BINS")
    # inflate: the same cap for both decoders; a stream a lane (64 a workgroup), or a stream a wavefront (NT / 64 a workgroup)
    a, b = _one(r"if \(blocks > (\d+) \* (\d+)\) blocks = \1 \* \2;", ifl, 2)
    k["IFL_BLOCKS"] = a * b
    k["IFL_LANES"] = _one(r"l1_inflate_lanes_kernel<<<dim3\(\(uint32_t\)blocks\), dim3\((\d+)\)", ifl)
    k["IFL_WAVES"] = _one(r"constexpr int NT = (\d+);", ifl) // 64
    assert re.search(r"l1_inflate_kernel<<<dim3\(\(uint32_t\)blocks\), dim3\(NT\)", ifl)
    k["IFL_WIDE_MIN"] = _const(ifl, "HMSE_INFLATE_WIDE_MIN")
    k["MH_GRID"] = _const(mh, "MH_GRID")
    assert len(re.findall(r"\w+ < MH_GRID \? \w+ : MH_GRID", mh)) == 2
    k["QY_GRID"], k["QY_CAP"] = _const(qy, "QY_GRID"), _const(qy, "QY_CAP")
    assert re.search(r"grid = n_q < QY_GRID \? \(uint32_t\)n_q : QY_GRID;", qy)
    k["EX_MAX_BLOCKS"], k["EX_CNT"] = _const(ex, "EX_MAX_BLOCKS"), _const(ex, "EX_CNT")
    assert re.search(r"grid = \(uint32_t\)\(n_chunks < EX_MAX_BLOCKS \? n_chunks : EX_MAX_BLOCKS\);", ex)
    assert len(re.findall(r"if \(nb > EX_MAX_BLOCKS\) nb = EX_MAX_BLOCKS;", ex)) == 2
    k["FIND_MAX_BLOCKS"], k["FIND_NT"], k["FIND_FEW"] = _const(fd, "FIND_MAX_BLOCKS"), _const(fd, "FIND_NT"), _const(fd, "FIND_FEW")
    k["FIND_TILE"] = k["FIND_NT"] * _const(fd, "FIND_STRIP")
    assert re.search(r"n_tiles < FIND_MAX_BLOCKS \? n_tiles : FIND_MAX_BLOCKS", fd) and re.search(r"if \(nb > FIND_MAX_BLOCKS\) nb = FIND_MAX_BLOCKS;", fd)
    assert re.search(r"tables_validate<FIND_NT>\(.*FIND_MAX_BLOCKS, stream\)", fd) and re.search(r"if \(nb > max_blocks\) nb = max_blocks;", cm)
    k["FSET_MAX_BLOCKS"], k["FSET_NT"] = _const(fs, "FSET_MAX_BLOCKS"), _const(fs, "FSET_NT")
    k["FSET_TILE"] = k["FSET_NT"] * _const(fs, "FSET_STRIP")
    assert re.search(r"n_tiles < FSET_MAX_BLOCKS \? n_tiles : FSET_MAX_BLOCKS", fs)
    k["FSET_VALIDATE_BLOCKS"] = _one(r"if \(nb > (\d+)\) nb = \1;\s*\n\s*findset_validate_kernel<<<", fs)
    k["FSET_SEAMS_BLOCKS"] = _one(r"if \(nb > (\d+)\) nb = \1; +// \(no LDS table here", fs)
    k["LINES_MAX_BLOCKS"], k["LINES_NT"] = _const(ln, "LINES_MAX_BLOCKS"), _const(ln, "LINES_NT")
    k["TALLY_MAX_BLOCKS"], k["TALLY_NT"] = _const(ty, "TALLY_MAX_BLOCKS"), _const(ty, "TALLY_NT")
    assert re.search(r"if \(nb > LINES_MAX_BLOCKS\) nb = LINES_MAX_BLOCKS;", ln) and re.search(r"if \(nb > TALLY_MAX_BLOCKS\) nb = TALLY_MAX_BLOCKS;", ty)
    a, b = _one(r"if \(blocks > (\d+) \* (\d+)\) blocks = \1 \* \2;", gz)
    k["GZ_BLOCKS"], k["GZ_WAVES"] = a * b, _const(gz, "GZ_NT") // 64
    k["BT_SIGS_BLOCKS"], k["BT_NT"] = _one(r"if \(blocks > (\d+)\) blocks = \1;", bt), _const(bt, "BT_NT")
    assert re.search(r"uint64_t blocks = \(n_words / 4 \+ 255\) / 256;", abi)                      # 16 bytes a thread
    k["FILL_BLOCKS"] = _one(r"if \(blocks > (\d+)\) blocks = \1;\s*\n\s*hmse_fill_kernel<<<dim3\(\(uint32_t\)blocks\), dim3\(256\)", abi)
    dfl = _src("l1_deflate.hip")
    k["ENC_BLOCKS"] = max(int(v) for v in re.findall(r"l1_encode_kernel<\d+, \d+><<<dim3\(\(uint32_t\)\(max_jobs < (\d+) \? max_jobs : \1\)\)", dfl))
    assert len(re.findall(r"l1_encode_kernel<\d+, \d+><<<dim3\(\(uint32_t\)\(max_jobs < (\d+) \? max_jobs : \1\)\)", dfl)) == 2
    a, b = _one(r"gather_kernel<<<dim3\(\(uint32_t\)\(\(n_sel \+ 3\) / (\d+) < (\d+) \?", dfl)
    k["GATHER_WAVES"], k["GATHER_BLOCKS"] = a, b
    return k


# ---- the table ------------------------------------------------------------------------------------------------------------------------
# cap: workgroups; unit: items a workgroup takes per trip; crossing = cap * unit + 1: the smallest input with a second trip.  `test`
# names the GPU test that takes the launch through at least two full trips and a ragged last one; `must`: a row of the ingest and read
# hot path or of the search scans, whose test is this module's.
Row = namedtuple("Row", "file kernels cap unit item test must")


def rows(k: dict | None = None) -> list:
    k = k or kernel_constants()
    return [
        Row("l3_sha256.hip", ("l3_sha256_kernel", "ord_hist_kernel"), k["SHA_BLOCKS"], k["SHA_NT"], "chunks", NEW + "test_sha256_lanes_hash_a_second_and_a_third_chunk", True),
        Row("l1_inflate.hip", ("l1_inflate_lanes_kernel",), k["IFL_BLOCKS"], k["IFL_LANES"], "streams", NEW + "test_inflate_lanes_pull_a_second_and_a_third_stream", True),
        Row("l1_inflate.hip", ("l1_inflate_kernel",), k["IFL_BLOCKS"], k["IFL_WAVES"], "streams", "tests/test_gpu_read.py::test_inflate_many_small_records_auto_dispatch", False),
        Row("l4_minhash.hip", ("l4_minhash_kernel",), k["MH_GRID"], 1, "chunks", NEW + "test_minhash_workgroups_sign_a_second_and_a_third_chunk", True),
        Row("l4_query.hip", ("qy_score_kernel",), k["QY_GRID"], 1, "queries", NEW + "test_query_workgroups_score_a_second_and_a_third_query", True),
        Row("export.hip", ("crc32_kernel",), k["EX_MAX_BLOCKS"], 1, "ranges", NEW + "test_crc32_workgroups_take_a_second_and_a_third_range", True),
        Row("find.hip", ("find_scan_kernel",), k["FIND_MAX_BLOCKS"], k["FIND_TILE"], "bytes of records", NEW + "test_find_scan_strides_over_more_tiles_than_the_grid", True),
        Row("findset.hip", ("findset_scan_kernel",), k["FSET_MAX_BLOCKS"], k["FSET_TILE"], "bytes of records", NEW + "test_findset_scan_strides_over_more_tiles_than_the_grid", True),
        Row("chunkmap.h", ("tables_validate_kernel",), k["FIND_MAX_BLOCKS"], k["FIND_NT"], "records or chunks", NEW + "test_tables_are_validated_beyond_the_first_trip", True),
        Row("find.hip", ("find_seams_kernel",), k["FIND_MAX_BLOCKS"], k["FIND_NT"], "(chunk, distance) pairs", NEW + "test_seams_stride_over_more_pairs_than_the_grid", False),
        Row("findset.hip", ("findset_seams_kernel",), k["FSET_SEAMS_BLOCKS"], k["FSET_NT"], "(chunk, distance) pairs", NEW + "test_seams_stride_over_more_pairs_than_the_grid", False),
        Row("l1_deflate.hip", ("l1_encode_kernel",), k["ENC_BLOCKS"], 1, "jobs of one list", "tests/test_gpu_scale.py::test_whole_pipeline_bit_exact_vs_oracle_at_scale", False),
        Row("l1_deflate.hip", ("gather_kernel",), k["GATHER_BLOCKS"], k["GATHER_WAVES"], "selected chunks", NEW + "test_deflate_gathers_more_records_than_its_grid_has_wavefronts", False),
        Row("findset.hip", ("findset_validate_kernel",), k["FSET_VALIDATE_BLOCKS"], k["FSET_NT"], "records, chunks or set entries", NEW + "test_tables_are_validated_beyond_the_first_trip", False),
        Row("lines.hip", ("lines_ranges_kernel",), k["LINES_MAX_BLOCKS"], k["LINES_NT"], "ranges", NEW + "test_ranges_are_checked_beyond_the_first_trip", False),
        Row("tally.hip", ("tally_ranges_kernel",), k["TALLY_MAX_BLOCKS"], k["TALLY_NT"], "ranges", NEW + "test_ranges_are_checked_beyond_the_first_trip", False),
        Row("gunzip.hip", ("measure_kernel",), k["GZ_BLOCKS"], k["GZ_WAVES"], "candidates", "tests/test_gpu_gunzip.py::test_enough_tiny_members_for_the_lane_per_stream_decoder", False),
        Row("bandtable.hip", ("bt_sigs_kernel",), k["BT_SIGS_BLOCKS"], k["BT_NT"], "words of keys and signatures", "tests/test_gpu_edges.py::test_band_tables_and_index_sort_around_tiles_and_2_16", False),
        Row("abi.hip", ("hmse_fill_kernel",), k["FILL_BLOCKS"], 256 * 16, "bytes filled", "tests/test_gpu_edges.py::test_l4_lsh_equal_keys_over_different_bands", False),
        Row("export.hip", ("crc32_validate_kernel",), k["EX_MAX_BLOCKS"], k["EX_CNT"], "ranges", NEW + "test_crc32_cuts_are_validated_beyond_the_first_trip", False),
    ]


def crossing(row: Row) -> int:
    return row.cap * row.unit + 1


def trips(count: int, cap: int, unit: int = 1) -> int:
    return -(-count // (cap * unit))


def trip_of(index, cap: int, unit: int = 1):
    """The trip in which a grid of `cap` workgroups reaches item `index` (grid stride; a dynamic hand-out reaches it no earlier)."""
    return np.asarray(index) // (cap * unit)


# Capped launches and grid-stride loops that have no row, each with its reason.  Keyed by (file, kernel).  No must-have kernel may be here.
OTHER_TESTS = "the regex / approximate family keeps its own second-trip tests: "
EXEMPT = {
    ("approx.hip", "approx_scan_kernel"): OTHER_TESTS + "tests/test_gpu_approx.py::test_more_tiles_than_the_grid",
    ("approx.hip", "approx_seams_kernel"): "not part of this table: the approximate search is checked by tests/test_gpu_approx.py alone",
    ("approx.hip", "approx_spans_kernel"): "not part of this table: the approximate search is checked by tests/test_gpu_approx.py alone",
    ("regex_core.h", "validate_kernel"): OTHER_TESTS + "GRID in tests/test_gpu_regex.py and tests/test_gpu_regexa.py",
    ("regex_core.h", "scan_kernel"): OTHER_TESTS + "GRID in tests/test_gpu_regex.py and tests/test_gpu_regexa.py",
    ("regex_core.h", "seams_kernel"): OTHER_TESTS + "GRID in tests/test_gpu_regex.py and tests/test_gpu_regexa.py",
    ("stream_batch.hip", "append_cuts_kernel"): "grid sized by the batch's capacity in the captured chain, capped at 262 144 chunks of ONE batch: gigabytes at the stream tests' geometries; one element per thread, no state between trips",
    ("stream_batch.hip", "commit_kernel"): "grid sized by the batch's capacity in the captured chain, capped at 262 144 chunks of ONE batch: gigabytes at the stream tests' geometries; one element per thread, no state between trips",
    ("stream_batch.hip", "sig_row_kernel"): "NOT crossed, and cheap to cross: a fixed grid of 1024 x 256 threads in the global-L4 captured chain; two trips and a tail need more than 16 384 NEW stored chunks in one piece, about 35 MiB of dense cut points (tests/edge_inputs.py: 2112-byte chunks) per piece, some 110 MiB of stream and its one-shot ingest as the reference; it needs a scenario of its own in tests/test_gpu_stream_gl4.py, which is left to that module; a 16-byte copy per thread, no state between trips",
    ("stream_batch.hip", "ingest_sig_rows_kernel"): "NOT crossed, and cheap to cross: a fixed grid of 2048 x 256 threads in the global-L4 captured chain; two trips and a tail need more than 32 768 NEW stored chunks in one batch, about 70 MiB of dense cut points per batch; the scenario is sig_row_kernel's at twice the size and is left to tests/test_gpu_stream_gl4.py; a copy per thread, no state between trips",
    ("export.hip", "gzip_validate_kernel"): "a crossing needs a store of 2 million records exported in one call, each a gzip member of its own: beyond a few seconds; one bounds check per member and thread, no state between trips",
}

# Lines the audit's expressions match that size no grid: a clamp of a length, a bit count or a reach.  (file, the statement)
NOT_A_GRID = {
    ("abi.hip", "if (bs > 32) bs = 32;"), ("manifest_pack.hip", "if (rc > 65535u) rc = 65535u;"), ("manifest_pack.hip", "if (raw > 65535u) raw = 65535u;"),
    ("l1_deflate.hip", "if (Dl > WMAX) Dl = WMAX;"), ("tally.hip", "if (w > TALLY_TRIP) w = TALLY_TRIP;"),
    ("tally.hip", "left < TALLY_TRIP ? (uint32_t)left : TALLY_TRIP"), ("bandtable.hip", "left < BT_PIECE ? left : BT_PIECE"),
    ("lines.hip", "before < HMSE_LINES_MAX_REACH ? before : HMSE_LINES_MAX_REACH"), ("lines.hip", "after < HMSE_LINES_MAX_REACH ? after : HMSE_LINES_MAX_REACH"),
    ("l1_deflate.hip", "if (nx > L) nx = L;"), ("l1_inflate.hip", "nb < D ? nb : D"), ("l1_deflate.hip", "km < 63u ? km : 63u"),
    ("l1_inflate.hip", "rem < 14 ? rem : 14"),
}

_CLAMP = re.compile(r"if \((\w+) > ([\w \*]+?)\) \1 = \2;")
_TERN = re.compile(r"(\w+|\([^()]*\) / \d+) < ([A-Z0-9]\w*) \? (?:\(\w+\))?\1 : \2")
_TERN_GT = re.compile(r"(\w+) > ([A-Z0-9]\w*) \? \2 : \1")
_STRIDE = re.compile(r"gridDim\.x")
_LAUNCH = re.compile(r"(?:RX_KERNEL\((\w+)\)|(\w+)(?:<[^<>;]*>)?)<<<")
_GLOBAL = re.compile(r"__global__[^;{]*?void (?:RX_KERNEL\((\w+)\)|(\w+))\(")
_CONSTANT = re.compile(r"[A-Z0-9_ \*u]+")


def capped_sites(sources: dict | None = None) -> list:
    """Every place in csrc (or in `sources`, {file name: text}) where a grid is capped or a kernel strides by its grid: (file, line, kernel
    or None, statement).  Three forms: `if (x > N) x = N;` with a launch within the next eight lines (or a constant N), `n < CAP ? n : CAP`
    (or `n > CAP ? CAP : n`) likewise, and any use of gridDim.x in a kernel.  The kernel is the one launched next (the first two) or the
    one the line stands in (the third).  What stands behind `//` is not read.
    NOT seen: a cap written with min() / std::min, and a grid clamped to a VARIABLE whose launch stands more than eight lines further on
    (a helper that returns the grid).  csrc holds neither form today (the one helper, sb_tail_blocks, clamps to a constant)."""
    if sources is None:
        sources = {name: _src(name) for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h"))}
    out = []
    for name, text in sources.items():
        lines = text.split("\n")
        for i, full in enumerate(lines):
            code = full.split("//")[0]
            m = _CLAMP.search(code) or _TERN.search(code) or _TERN_GT.search(code)
            if m:
                launched = next((g for j in range(i, min(i + 9, len(lines))) for g in _LAUNCH.findall(lines[j])), None)
                if launched is None and not _CONSTANT.fullmatch(m.group(2)):
                    continue                                    # a clamp to a variable with no launch behind it
                out.append((name, i + 1, (launched[0] or launched[1]) if launched else None, m.group(0)))
            elif _STRIDE.search(code):
                inside = next((g for j in range(i, -1, -1) for g in _GLOBAL.findall(lines[j])), None)
                assert inside, (name, i + 1)
                out.append((name, i + 1, inside[0] or inside[1], code.strip()))
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _cuts(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def sha_chunks(k: dict, seed: int = 41):
    """2 x lanes + 77 chunks.  Lengths cycle through 0..130 (every padding branch: rem < 56, 56..63, multiples of 64); every 1009th is
    4097 and every 4999th 32768 bytes, so that lanes of a wavefront finish at different times and a lane goes from a long chunk with a
    prefetch in flight to a short one.  The last chunk ends with the buffer, inside its last 64 bytes.  -> (data, cuts, facts)"""
    lanes = k["SHA_BLOCKS"] * k["SHA_NT"]
    n = 2 * lanes + 77
    lens = np.arange(n, dtype=np.int64) % 131
    lens[5::1009] = 4097
    lens[11::4999] = 32768
    lens[[n - 70, n - 33]] = (32768, 4097)                                  # ... also among the 77 of the ragged third trip
    lens[-1] = 61
    cuts = _cuts(lens)
    data = np.random.default_rng(seed).integers(0, 256, int(cuts[-1]), dtype=np.uint8)
    return data, cuts, {"count": n, "lanes": lanes, "trips": trips(n, lanes), "long_at": np.flatnonzero(lens > 4096)}


def sha_order_workspace(k: dict, n_chunks: int) -> int:
    """The workspace from which hmse_l3_sha256 builds its order table and hands chunks out longest first (below it: index order)."""
    return 256 + k["ORD_BINS"] * 4 + -(-n_chunks * 4 // 256) * 256


def sha_reference(data: np.ndarray, cuts: np.ndarray) -> np.ndarray:
    import hashlib
    blob, c = data.tobytes(), cuts.tolist()
    return np.frombuffer(b"".join(hashlib.sha256(blob[c[i]: c[i + 1]]).digest() for i in range(len(c) - 1)), np.uint8).reshape(-1, 32)


def inflate_records(k: dict, seed: int = 43):
    """2 x lanes + 64 x 37 + 5 records of 0..600 bytes: nine in ten FULL — more than there are lanes, so some lane takes a FULL record
    after a FULL record and a third record, whichever way the hand-out falls —, one in ten DELTA with an EARLIER record as its
    dictionary (chains included), 3 % corrupted.  -> ([(stream, raw length, base or -1)], facts)"""
    lanes = k["IFL_BLOCKS"] * k["IFL_LANES"]
    n = 2 * lanes + 64 * 37 + 5
    rnd = random.Random(seed)
    text = words_text(1 << 20, seed=seed).tobytes()
    strategies = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)
    recs, raws, damaged = [], [], []
    for i in range(n):
        m = rnd.choice((0, 1, 5, 40, 300, 600)) if rnd.random() < 0.2 else rnd.randrange(601)
        o = rnd.randrange(len(text) - 600)
        t = text[o: o + m]
        b = -1
        if i > 10 and rnd.random() < 0.1:
            b = rnd.randrange(max(0, i - 200), i)
            while not raws[b] and b > 0:
                b -= 1
            if not raws[b]:
                b = -1
        lvl, strat = rnd.choice((0, 1, 6, 9)), rnd.choice(strategies)
        c = zlib.compressobj(lvl, zlib.DEFLATED, -15, 9, strat, zdict=raws[b]) if b >= 0 else zlib.compressobj(lvl, zlib.DEFLATED, -15, 9, strat)
        s = c.compress(t) + c.flush()
        if rnd.random() < 0.03:
            s = mutate(s, rnd)
            damaged.append(i)
        recs.append((s, len(t), b))
        raws.append(t)
    base = np.array([r[2] for r in recs], np.int64)
    return recs, {"count": n, "lanes": lanes, "trips": trips(n, lanes), "base": base, "damaged": np.array(damaged), "raws": raws}


def mutate(stream: bytes, rnd) -> bytes:
    """A damaged copy of a DEFLATE stream: a bit flipped up front (headers and code-length sets live there) or anywhere, a truncation, or a
    trailing byte."""
    m = bytearray(stream)
    k = rnd.random()
    if k < 0.5 and m:
        m[rnd.randrange(min(len(m), 40))] ^= 1 << rnd.randrange(8)
    elif k < 0.7 and m:
        m[rnd.randrange(len(m))] ^= 1 << rnd.randrange(8)
    elif k < 0.85:
        m = m[:rnd.randrange(len(m) + 1)]
    else:
        m += b"\0"
    return bytes(m)


def pack_records(recs):
    """-> (streams, stream_off, kind, base, raw_len): the dense arrays of an hmse_l1_inflate call."""
    streams = np.frombuffer(b"".join(r[0] for r in recs) + b"\0", np.uint8)[:-1].copy()
    off = _cuts([len(r[0]) for r in recs])
    raw_len = np.array([r[1] for r in recs], np.int64)
    base = np.array([r[2] for r in recs], np.int64)
    return streams, off, np.where(base >= 0, 2, 0).astype(np.uint8), base, raw_len


def minhash_chunks(k: dict, seed: int = 47):
    """2 x MH_GRID + 9 chunks of 64..300 bytes of words (shingles recur: the memo table answers some and computes others), the last
    one ending with the buffer.  -> (data, cuts, facts)"""
    n = 2 * k["MH_GRID"] + 9
    lens = 64 + (np.arange(n, dtype=np.int64) * 89) % 237
    cuts = _cuts(lens)
    return words_text(int(cuts[-1]), seed=seed), cuts, {"count": n, "trips": trips(n, k["MH_GRID"])}


def query_signatures(k: dict, seed: int = 53, bands: int = 4):
    """A store of 3000 signatures and 2 x QY_GRID + 45 queries of three kinds.  `crowd` queries share band 0 with 300 stored signatures of
    differing scores (more candidates than the QY_CAP entries of a workgroup's hit buffer: it is reduced and its admission threshold
    raised to a score far above 32), `none` queries have no candidate, `near` queries one or four, each with a score of about 32 (one
    band of a stored signature).  The first QY_GRID queries are ALL crowd queries: every resident workgroup starts on one and is as busy
    as every other, so the workgroups that take the later queries — none, near and a few crowd ones, mixed — come from a query that raised
    their threshold.  A threshold (or count) that reached the next query would drop its hits.
    -> (S u32[3000, 128], Q u32[n, 128], facts)"""
    rng = np.random.default_rng(seed)
    R = 128 // bands
    rnd = lambda m: rng.integers(0, 2**32, (m, 128), dtype=np.uint64).astype(np.uint32)
    n_s, n = 3000, 2 * k["QY_GRID"] + 45
    S = rnd(n_s)
    crowd = np.arange(100, 400)
    proto = rnd(1)[0]
    S[crowd] = proto
    flip = rng.random((crowd.size, 128)) < rng.uniform(0.0, 0.9, (crowd.size, 1))
    flip[:, :R] = False                                                     # band 0 stays: every crowd member is a candidate
    S[crowd] = np.where(flip, rnd(crowd.size), S[crowd])
    S[1000:1003, R: 2 * R] = S[2000, R: 2 * R]                              # a family of four in band 1
    Q = rnd(n)
    kind = np.array(["none", "near", "none", "near", "crowd", "none", "near", "none"])[np.arange(n) % 8]
    kind[: k["QY_GRID"]] = "crowd"
    is_crowd, is_near = kind == "crowd", kind == "near"
    Q[is_crowd] = proto
    noise = rng.random((int(is_crowd.sum()), 128)) < 0.2
    noise[:, :R] = False
    Q[is_crowd] = np.where(noise, rnd(int(is_crowd.sum())), Q[is_crowd])
    near = np.flatnonzero(is_near)
    src = np.where(np.arange(near.size) % 5 == 0, 2000, 600 + np.arange(near.size) % 2300)
    b = np.arange(near.size) % bands
    for j, (q, s) in enumerate(zip(near, src)):
        bb = 1 if s == 2000 else int(b[j])
        Q[q, bb * R: (bb + 1) * R] = S[s, bb * R: (bb + 1) * R]
    return S, Q, {"count": n, "trips": trips(n, k["QY_GRID"]), "kind": kind, "crowd": crowd, "bands": bands}


def crc_ranges(k: dict, seed: int = 59):
    """2 x EX_MAX_BLOCKS + 33 ranges with lengths 0..200 and a few long ones (one and several 8 KiB tiles), the last ending with the
    buffer.  -> (data, cuts, facts)"""
    n = 2 * k["EX_MAX_BLOCKS"] + 33
    lens = np.arange(n, dtype=np.int64) % 201
    long_at = np.array([7, k["EX_MAX_BLOCKS"] - 1, k["EX_MAX_BLOCKS"], k["EX_MAX_BLOCKS"] + 1234, 2 * k["EX_MAX_BLOCKS"], n - 2])
    lens[long_at] = (8192, 70001, 8193, 20000, 16384, 4097)
    cuts = _cuts(lens)
    data = np.random.default_rng(seed).integers(0, 256, int(cuts[-1]), dtype=np.uint8)
    return data, cuts, {"count": n, "trips": trips(n, k["EX_MAX_BLOCKS"]), "long_at": long_at}


def crc_reference(data: np.ndarray, cuts: np.ndarray) -> np.ndarray:
    blob, c = data.tobytes(), cuts.tolist()
    return np.array([zlib.crc32(blob[c[i]: c[i + 1]]) for i in range(len(c) - 1)], np.uint32)


def many_tiny_ranges(k: dict, seed: int = 61):
    """2 x EX_MAX_BLOCKS x EX_CNT + 77 ranges of 0..3 bytes for the kernel that checks the cuts, and the two places where a test puts a
    descending pair: in the second trip and in the ragged third.  -> (data, cuts, facts)"""
    per = k["EX_MAX_BLOCKS"] * k["EX_CNT"]
    n = 2 * per + 77
    lens = (np.arange(n, dtype=np.int64) * 7) % 4
    cuts = _cuts(lens)
    data = np.random.default_rng(seed).integers(0, 256, int(cuts[-1]), dtype=np.uint8)
    bad_at = [per + 12345, 2 * per + 70]
    assert all(lens[i] > 0 for i in bad_at)                                   # swapping cuts[i], cuts[i + 1] makes them descend
    return data, cuts, {"count": n, "trips": trips(n, per), "bad_at": bad_at, "per_trip": per}


def tiny_crc_reference(data: np.ndarray, cuts: np.ndarray) -> np.ndarray:
    """zlib.crc32 of ranges of at most 3 bytes, through a table of the distinct contents."""
    lens = np.diff(cuts)
    assert lens.max() <= 3
    pad = np.concatenate([data, np.zeros(4, np.uint8)])
    code = np.zeros(lens.size, np.int64)
    for j in range(3):
        code |= np.where(lens > j, pad[cuts[:-1] + j].astype(np.int64), 0) << (8 * j)
    code |= lens << 24
    u, inv = np.unique(code, return_inverse=True)
    table = np.array([zlib.crc32(int(c & 0xFFFFFF).to_bytes(3, "little")[: int(c >> 24)]) for c in u], np.uint32)
    return table[inv.ravel()]


# ---- the scans: filler that no pattern holds, occurrences planted where the trips meet ---------------------------------------------------
FILLER = ord(".")
FIND_FEW_PATTERNS = [b"Qz7xW", b"needle in a haystack", b"7x", b"Q"]                             # FIND_FEW of them; "7x" and "Q" also lie inside "Qz7xW"
FIND_MANY_PATTERNS = FIND_FEW_PATTERNS + [b"W!", b"zebra", b"Zebra crossing", b"0123456789" * 25 + b"012345", b"xW", b"haystack",
                                          b"a hay", b"k" * 17]
FSET_PATTERNS = [p for p in FIND_MANY_PATTERNS if len(p) >= 4] + [b"Qz7x", b"needle", b"needle in", b"0123456789" * 3, b"stack#", b"rossing"]
SLOT = 512            # a planted text starts in the first 200 bytes of a 512-byte slot and has at most 256 bytes: no two touch


def _variants(pats):
    """What is planted: every pattern, the same in the other case, and with its last byte changed (a near miss)."""
    return list(pats) + [p.swapcase() for p in pats] + [p[:-1] + b"#" for p in pats]


def scan_input(tile: int, cap: int, pats, seed: int):
    """(2 cap + 3) tiles of filler, the last of 123 bytes, with `pats` and their variants planted: in about 1500 slots all over the input,
    across the two seams where the last tile of a trip meets the first of the next (and a few other tile seams), and ending on the last
    byte.  Five records, one empty, one boundary cutting a planted occurrence in two.  -> (raw, raw_off, facts)"""
    assert tile % SLOT == 0 and all(FILLER not in p and 1 <= len(p) <= 256 for p in pats)
    rng = np.random.default_rng(seed)
    n = (2 * cap + 2) * tile + 123
    raw = np.full(n, FILLER, np.uint8)
    var = _variants(pats)
    places = []

    def put(o, v):
        assert 0 <= o and o + len(v) <= n
        raw[o: o + len(v)] = np.frombuffer(v, np.uint8)
        places.append((o, len(v)))

    longest = max(pats, key=len)
    seams = [cap * tile, 2 * cap * tile, 3 * tile, (cap + 7) * tile, (2 * cap + 1) * tile]
    for j, B in enumerate(seams):
        put(B - len(longest) // 2, longest)                                     # across the seam
        put(B + SLOT - 1 - j % 2, pats[0])                                      # wholly behind it, in the first tile of the next trip
        put(B - SLOT - len(pats[0]) + j % 3, pats[0])                           # wholly in front, in the last tile of the trip
        side = 1 if B + 7 * tile < n else -1
        put(B + side * 5 * tile - len(pats[0]), pats[0])                        # another seam: the pattern ends with the tile
        put(B + side * 6 * tile, pats[0])                                       # ... and starts with one
    put(n - len(pats[0]), pats[0])                                              # ends on the last byte of the input
    taken = {(o + d) // SLOT for o, ln in places for d in (-SLOT, 0, ln, SLOT)}
    slots = np.sort(rng.choice(n // SLOT - 2, 1500, replace=False) + 1)
    for i, s in enumerate(slots.tolist()):
        if s in taken or s - 1 in taken or s + 1 in taken:
            continue
        put(s * SLOT + int(rng.integers(0, 200)), var[i % len(var)])
    cut_place = next(o for o, ln in places if ln >= 5 and tile < o < cap * tile - 4 * SLOT)
    mid = sorted(o for o, _ in places)[len(places) // 2]
    raw_off = np.array([0, cut_place + 2, cut_place + 2, mid + SLOT, (2 * cap + 1) * tile + 77, n], np.int64)
    starts = np.array([o for o, _ in places])
    return raw, raw_off, {"count": n, "tiles": -(-n // tile), "trips": trips(-(-n // tile), cap), "places": places, "seams": seams,
                          "trip_of_place": trip_of(starts // tile, cap), "cut_place": cut_place}


def planted_hits(raw: np.ndarray, raw_off, places, pats, ignore_case: bool = False):
    """What a scan finds, looking at the planted places only (the filler holds no byte of a pattern, so every occurrence overlaps one):
    -> (sorted [(position, pattern)] of the occurrences lying wholly inside one record, counts [P])."""
    off = np.asarray(raw_off, np.int64)
    hits = set()
    for o, ln in places:
        a = max(0, o - 256)
        w = raw[a: o + ln + 256].tobytes()
        if ignore_case:
            w = w.lower()
        for j, p in enumerate(pats):
            p = p.lower() if ignore_case else p
            s = w.find(p)
            while s >= 0:
                pos = a + s
                r = int(np.searchsorted(off, pos, side="right")) - 1
                if pos + len(p) <= off[r + 1]:
                    hits.add((pos, j))
                s = w.find(p, s + 1)
    hits = sorted(hits)
    return hits, [sum(1 for _, j in hits if j == q) for q in range(len(pats))]


def many_records(per: int, seed: int = 67):
    """2 x per + 77 records (per: the threads of a full grid of the kernel that checks the tables) of 0..7 bytes of filler with a 4-byte pattern planted at 3000 places (where it crosses
    a record's end it is no hit), and the two records whose bounds a test swaps to break the table: in the second trip and in the ragged
    third.  -> (raw, raw_off, facts)"""
    n_rec = 2 * per + 77
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 8, n_rec)
    tail = 2 * per + np.array([3, 30, 76])                                   # three records of the ragged third trip that hold the pattern
    lens[tail] = (4, 7, 5)
    raw_off = _cuts(lens)
    raw = np.full(int(raw_off[-1]), FILLER, np.uint8)
    pat = b"Qz7x"
    at = np.sort(rng.choice(raw.size // 16 - 1, 3000, replace=False)) * 16 + rng.integers(0, 8, 3000)
    at = np.sort(np.concatenate([at[at + 4 <= raw_off[2 * per]], raw_off[tail]]))
    places = []
    for o in at.tolist():
        raw[o: o + 4] = np.frombuffer(pat, np.uint8)
        places.append((o, 4))
    bad_at = [next(j for j in range(i, n_rec) if lens[j] > 0) for i in (per + 4321, 2 * per + 50)]   # swapping raw_off[j], raw_off[j + 1] makes them descend
    rec = np.searchsorted(raw_off, at, side="right") - 1
    return raw, raw_off, {"count": n_rec, "trips": trips(n_rec, per), "per_trip": per, "places": places, "pattern": pat, "bad_at": bad_at,
                          "trip_of_place": trip_of(rec, per)}


def seam_corpus(threads_per_trip: int, span: int, seed: int):
    """Chunks for the seams kernels, which give one thread to every (chunk, distance 1..span from its end): 2 x threads_per_trip / span
    chunks and a few more, of 1..40 bytes over the letters a..d, with a 256-byte pattern (span = 255) that occurs across chunk ends all
    over the corpus and runs to its last byte.  The chunks are their own records.  -> (corpus bytes, cuts list, patterns, facts)"""
    rng = np.random.default_rng(seed)
    n_chunks = -(-2 * threads_per_trip // span) + 40
    lens = rng.integers(1, 41, n_chunks)
    cuts = _cuts(lens)
    corpus = rng.integers(97, 101, int(cuts[-1]), dtype=np.uint8)
    long = bytes(rng.integers(97, 101, span + 1, dtype=np.uint8))
    m = (corpus.size // 1024 - 1) // 2
    at = np.sort(rng.choice(corpus.size // 1024 - 1, m, replace=False)) * 1024 + rng.integers(0, 500, m)
    for o in at.tolist():
        corpus[o: o + len(long)] = np.frombuffer(long, np.uint8)
    corpus[-len(long):] = np.frombuffer(long, np.uint8)
    pats = [long, long[:5], b"abca", long[100:117]]
    at = np.append(at, corpus.size - len(long))
    chunk = np.searchsorted(cuts, at, side="right") - 1
    return corpus.tobytes(), cuts.tolist(), pats, {"count": n_chunks * span, "chunks": n_chunks, "trips": trips(n_chunks * span, threads_per_trip),
                                                   "planted_at": at, "trip_of_place": trip_of(chunk * span, threads_per_trip)}


def many_ranges(per: int, seed: int = 89):
    """2 x per + 77 ranges of 0..6 bytes over a corpus of 60 000 bytes (letters a..c: equal ranges are common) in chunks of 1..30 bytes,
    each chunk its own record; rep[i]: another range to compare range i with; bad_at: a range of the second trip and one of the ragged
    third, for a test to spoil.  -> (corpus, cuts, start, end, rep, facts)"""
    rng = np.random.default_rng(seed)
    n = 2 * per + 77
    cuts = _cuts(rng.integers(1, 31, 4000))
    corpus = rng.integers(97, 100, int(cuts[-1]), dtype=np.uint8)
    lens = rng.integers(0, 7, n)
    start = rng.integers(0, corpus.size - 6, n)
    start[-1], lens[-1] = corpus.size - 5, 5                                   # the last range ends with the corpus
    rep = rng.integers(0, n, n)
    rep[::5] = np.arange(n)[::5]                                              # itself
    return corpus, cuts, start.astype(np.int64), (start + lens).astype(np.int64), rep.astype(np.int64), \
        {"count": n, "trips": trips(n, per), "per_trip": per, "bad_at": [per + 999, 2 * per + 60]}


def gathered(corpus: np.ndarray, start: np.ndarray, end: np.ndarray):
    """-> (the bytes of every range back to back, out_off)."""
    lens = end - start
    out_off = _cuts(lens)
    idx = np.repeat(start - out_off[:-1], lens) + np.arange(int(out_off[-1]))
    return corpus[idx], out_off


def same_ranges(corpus: np.ndarray, start: np.ndarray, end: np.ndarray, rep: np.ndarray) -> np.ndarray:
    """u8[n]: range i and range rep[i] have the same length and bytes (ranges of at most 7 bytes: compared as packed words)."""
    lens = end - start
    assert lens.max() <= 7
    pad = np.concatenate([corpus, np.zeros(8, np.uint8)])
    code = lens.astype(np.int64) << 56
    for j in range(7):
        code |= np.where(lens > j, pad[start + j].astype(np.int64), 0) << (8 * j)
    return (code == code[rep]).astype(np.uint8)


def tiny_chunks(k: dict, seed: int = 97):
    """2 x (GATHER_BLOCKS x GATHER_WAVES) + 37 chunks of 2..40 bytes of words for hmse_l1_deflate, whose last kernel copies one record per
    wavefront out of the workspace.  -> (data, cuts, facts)"""
    per = k["GATHER_BLOCKS"] * k["GATHER_WAVES"]
    n = 2 * per + 37
    lens = 2 + (np.arange(n, dtype=np.int64) * 7) % 39
    cuts = _cuts(lens)
    return words_text(int(cuts[-1]), seed=seed), cuts, {"count": n, "trips": trips(n, per), "per_trip": per}
