"""Inputs that reach the branches, buffers and compile-time thresholds the generated-text tests never touch.

Pure numpy, seeded, no device.  Every builder returns its input together with the facts it promises about it (candidates per
segment, window size T, shingle count, bucket populations); tests/test_edge_inputs_host.py proves each promise from the CPU
reference and the constants in the kernel sources, tests/test_gpu_edges.py runs the inputs through the kernels."""
from __future__ import annotations

import os
import re

import numpy as np

from conftest import words_text

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmse_amd", "csrc")


# ---- thresholds, read from where the kernels keep them ----------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(src, name):
    return int(re.search(r"constexpr (?:int|uint32_t) %s = (\d+)u?;" % name, src).group(1))


def kernel_constants() -> dict:
    """RS_MAX_TILES / RS_MAX_CAND / the L2 tile, MH_TBITS -> MH_SUB, BT_NT / BT_PIECE, and the `n / per * 8 + 65536` of l2_cand_cap."""
    l2, mh, bt, dfl = _src("l2_cdc.hip"), _src("l4_minhash.hip"), _src("bandtable.hip"), _src("l1_deflate.hip")
    k = {"RS_MAX_TILES": _const(l2, "RS_MAX_TILES"), "RS_MAX_CAND": _const(l2, "RS_MAX_CAND"),
         "L2_TILE": _const(l2, "L2_NT") * int(re.search(r"#define HMSE_L2_STRIP (\d+)", l2).group(1)),
         "MH_TBITS": _const(mh, "MH_TBITS"), "BT_NT": _const(bt, "BT_NT"), "BT_PIECE": _const(bt, "BT_PIECE")}
    assert re.search(r"constexpr int MH_SLOTS = 1 << MH_TBITS;", mh) and re.search(r"constexpr int MH_SUB = MH_SLOTS \* 3 / 4;", mh)
    k["MH_SUB"] = (1 << k["MH_TBITS"]) * 3 // 4
    m = re.search(r"return n / per \* (\d+) \+ (\d+);", l2)
    k["CAND_FACTOR"], k["CAND_SLACK"] = int(m.group(1)), int(m.group(2))
    assert re.search(r"uint64_t per = \(uint64_t\)cfg->avg_size >> cfg->norm_level;", l2)
    # profile slot of every match-kernel size class, keyed by its window cap (plain jobs; dictionary jobs report 10 higher)
    caps = {n: int(v) for n, v in re.findall(r"#define HMSE_(TCAP_\w+) (\d+)", dfl)}
    caps["TCAP_SG3"] = int(re.search(r"TCAP_SG3 = (\d+)", dfl).group(1))
    caps["TCAP_B"] = int(re.search(r"TCAP_B = (\d+)", dfl).group(1))
    k["CLASS_SLOT"] = {caps[name]: 8 + int(s) for s, name in re.findall(r"HMSE_DFL_LAUNCH\(false, \d+, 8 \+ (\d), \w+, \w+, (TCAP_\w+),", dfl)}
    k["ENC_SPLIT"] = int(re.search(r"l1_encode_kernel<0, (\d+)>", dfl).group(1))
    return k


def l2_cand_capacity(n: int, cfg, k: dict) -> int:
    """Entries of the candidate list hmse_workspace_bytes(HMSE_STAGE_L2, ...) provisions (l2_cand_cap)."""
    per = max(1, cfg.avg_size >> cfg.norm_level)
    return n // per * k["CAND_FACTOR"] + k["CAND_SLACK"]


# ---- L2: Gear hash in window form ---------------------------------------------------------------------------------------------
def gear_candidates(data: np.ndarray, G: np.ndarray, mask_l: int, block: int = 1 << 22) -> np.ndarray:
    """bool[n]: byte i is a cut candidate, i.e. the window hash sum_{k<64} G[data[i-k]] << k (mod 2^64, bytes in front of the input
    absent) has no bit of the easy mask.  64 shifted adds per block; the rolling state is never reset, so this is a pure function
    of the 64 bytes ending at i."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    out = np.zeros(n, dtype=bool)
    m = np.uint64(mask_l)
    for a in range(0, n, block):
        lo = max(0, a - 63)
        g = G[data[lo: min(n, a + block)]]
        h = np.zeros(g.size, dtype=np.uint64)
        for s in range(64):
            h[s:] += g[: g.size - s] << np.uint64(s)
        out[a: a + block] = ((h & m) == 0)[a - lo:]
    return out


def dense_pairs(G: np.ndarray, mask_l: int) -> list:
    """Byte pairs (x, y), x != y, for which a window filled with x y x y ... y has no bit of the easy mask: in a run of the pair every
    second position (those holding y) is a candidate.  Found by search over all 65 280 ordered pairs; ascending."""
    k = np.arange(64, dtype=np.uint64)
    even = np.array([(G << s) for s in k[0::2]]).sum(axis=0, dtype=np.uint64)      # the byte under the window's end and every second before it
    odd = np.array([(G << s) for s in k[1::2]]).sum(axis=0, dtype=np.uint64)
    h = odd[:, None] + even[None, :]                                               # h[x, y]
    hit = (h & np.uint64(mask_l)) == 0
    np.fill_diagonal(hit, False)
    return [(int(x), int(y)) for x, y in zip(*np.nonzero(hit))]


def pair_run(n: int, pair) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    out[0::2], out[1::2] = pair[0], pair[1]
    return out


def l2_dense_segment(pair, n: int = 110_000):
    """One segment of the pair: about n / 2 candidates.  -> (data, facts)"""
    return pair_run(n, pair), {"segments": [(0, n)], "candidates_about": n // 2}


def l2_mixed_segment(pair, text: np.ndarray, tile: int):
    """Text with a dense stretch at the very start, in the middle and at the very end of one segment: the walk meets tiles with no
    candidate (a constant stretch), with a few (text) and with tile / 2 (the pair).  -> (data, facts)"""
    parts = [pair_run(2 * tile, pair), text[: 3 * tile + 17], np.zeros(2 * tile, np.uint8), text[3 * tile: 5 * tile + 5],
             pair_run(20000, pair), text[5 * tile: 7 * tile + 1], pair_run(9234, pair)]
    data = np.concatenate(parts)
    return data, {"segments": [(0, data.size)], "candidates_about": (2 * tile + 20000 + 9234) // 2}


def l2_sparse_tiles(tile: int, max_tiles: int, seed: int = 5):
    """Bytes with so few candidates (a 16 KiB island of text per MiB of zeros) that only the TILE count decides between the staged walk
    and the walk from global memory, and segmentations around max_tiles: exactly max_tiles aligned tiles (staged), max_tiles + 1
    (global), max_tiles tiles' worth of bytes from an unaligned start (spans max_tiles + 1: global), and the rest.
    -> (data, {name: seg_off}, facts)"""
    n = (max_tiles + 1) * tile + (5 << 20) + 321
    data = np.zeros(n, np.uint8)
    text = words_text(16384 * (n // (1 << 20) + 1), seed=seed)
    for i, a in enumerate(range(777, n - 16384, 1 << 20)):
        data[a: a + 16384] = text[i * 16384: (i + 1) * 16384]
    segs = {"exactly": [0, max_tiles * tile, n], "one_more": [0, (max_tiles + 1) * tile, n],
            "unaligned": [0, 100, 100 + max_tiles * tile, n], "unaligned_short": [0, tile - 1, tile - 1 + (max_tiles - 1) * tile + 2, n]}
    spans = {"exactly": [max_tiles, None], "one_more": [max_tiles + 1, None], "unaligned": [1, max_tiles + 1, None],
             "unaligned_short": [1, max_tiles + 1, None]}
    return data, {k: np.array(v, dtype=np.uint64) for k, v in segs.items()}, {"tiles_spanned": spans}


def tiles_spanned(a: int, b: int, tile: int) -> int:
    return (b - 1) // tile - a // tile + 1 if b > a else 0


def l2_overflow(pair, n: int):
    """n bytes of the pair: n / 2 candidates, more than the provisioned list holds."""
    return pair_run(n, pair), {"candidates_about": n // 2}


def l2_corpus_with_dense_stretch(pair, text: np.ndarray):
    """A corpus for the whole pipeline: text, 600 000 bytes of the pair (overflows the list on its own), text again (the same text:
    duplicates and near-duplicates for L3 / L4 / L1)."""
    t = text[: 1_500_000]
    v = t[: 700_000].copy()
    v[::1700] ^= 0x20
    return np.concatenate([t, pair_run(600_000, pair), v, t[200_000: 500_000]]), {"dense_bytes": 600_000}


# ---- a piece of dense CUT POINTS (not dense candidates): the stream chain's per-chunk rows -----------------------------------------
DENSE_CUT_FILL, DENSE_CUT_RUN = 2040, 72


def dense_cut_piece(pair, n: int, seed: int, text: bool = False) -> np.ndarray:
    """n bytes whose chunks are about as small as chunks get: DENSE_CUT_FILL bytes of filler (random bytes, or words with `text`: every
    period different, so all digests differ), then DENSE_CUT_RUN bytes of `pair` — a pair of dense_pairs(G, mask_s), the HARD mask, so the
    first position of the run that is min_size (2048) behind the last cut is a cut: one chunk per period of 2112 bytes, a quarter of
    avg_size.  The runs are short: the candidate count stays far below the list's capacity (unlike l2_overflow)."""
    period = DENSE_CUT_FILL + DENSE_CUT_RUN
    k = -(-n // period)
    fill = (words_text(k * DENSE_CUT_FILL, seed=seed) if text else np.random.default_rng(seed).integers(0, 256, k * DENSE_CUT_FILL, dtype=np.uint8))
    out = np.empty((k, period), np.uint8)
    out[:, :DENSE_CUT_FILL] = np.asarray(fill[: k * DENSE_CUT_FILL]).reshape(k, DENSE_CUT_FILL)
    out[:, DENSE_CUT_FILL:] = pair_run(DENSE_CUT_RUN, pair)
    return out.reshape(-1)[:n].copy()


def dense_cut_near_duplicate(piece: np.ndarray, every: int = 1) -> np.ndarray:
    """A dense-cut piece for ANOTHER piece of the stream: the same bytes with one letter's case flipped in the middle of every `every`-th
    period's filler (far from the 64-byte windows that decide the cuts): the same cut points, chunks that are near-duplicates of
    `piece`'s — dictionaries for L4 to find on whichever rank got `piece`."""
    out = piece.copy()
    out[DENSE_CUT_FILL // 2:: (DENSE_CUT_FILL + DENSE_CUT_RUN) * every] ^= 0x20
    return out


# ---- L1 DEFLATE: windows on the class caps --------------------------------------------------------------------------------------
CONTENTS = ("text", "neardup", "run", "period", "random")


def _content(kind: str, L: int, D: int, text: np.ndarray, rng, salt: int):
    """(chunk[L], dictionary[D] or None)."""
    o = 1000 + 37 * salt
    if kind == "text":
        return text[o: o + L].copy(), (text[o + 40000: o + 40000 + D].copy() if D else None)
    if kind == "neardup":                       # the dictionary's own bytes (continued past its end), edited in the first and last 16
        src = text[o: o + max(L, D)]
        c = src[:L].copy()
        c[: min(16, L): 5] ^= 0x01
        c[max(0, L - 16):: 7] ^= 0x02
        return c, (src[:D].copy() if D else None)
    if kind == "run":
        return np.full(L, 0x61, np.uint8), (np.full(D, 0x61, np.uint8) if D else None)
    if kind == "period":
        p = np.tile(np.frombuffer(b"abcd", np.uint8), (max(L, D) + 8) // 4 + 1)
        return p[:L].copy(), (p[2: 2 + D].copy() if D else None)
    if kind == "random":
        return rng.integers(0, 256, L, dtype=np.uint8), (text[o: o + D].copy() if D else None)
    raise ValueError(kind)


def deflate_boundary_jobs(caps, dict_jobs: bool, seed: int = 11, contents=CONTENTS, only_cap: int | None = None):
    """Jobs whose window T = L + min(D, 32768) sits on a class cap c or one byte either side (c + 1 left out at 65536, and wherever the
    chunk would pass 32768 bytes).  Plain jobs: T = L.  Dictionary jobs at three splits: D in {1, 2, 3}; D = L (+- 1); D >= 32768 with
    a dictionary LONGER than the window (only its last 32768 bytes count).

    -> dict(data, cuts, ids, base, T, cap, parts): `data` / `cuts` hold dictionaries and chunks, `ids` the chunks to encode (a
    dictionary above 32768 bytes is no job itself), `base` the dictionary's CHUNK index or -1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    text = words_text(140_000, seed=seed)
    parts, ids, base, Ts, cap_of = [], [], [], [], []
    salt = 0
    for c in caps:
        if only_cap is not None and c != only_cap:
            continue
        for T in (c - 1, c, c + 1):
            if T > 65536:
                continue
            splits = []
            if not dict_jobs:
                if T <= 32768:
                    splits.append((T, 0, 0))
            else:
                d = 1 + salt % 3
                if T - d <= 32768:
                    splits.append((T - d, d, d))                       # a dictionary of 1..3 bytes
                if T - T // 2 <= 32768:
                    splits.append((T - T // 2, T // 2, T // 2))        # D = L or L - 1
                if 32768 < T:
                    splits.append((T - 32768, 32768 + 1234, 32768))    # longer than the window
            for L, D, Deff in splits:
                assert 1 <= L <= 32768 and L + Deff == T
                for kind in contents:
                    salt += 1
                    chunk, dct = _content(kind, L, D, text, rng, salt)
                    if dct is not None:
                        parts.append(dct); base.append(len(parts) - 1)
                    else:
                        base.append(-1)
                    parts.append(chunk); ids.append(len(parts) - 1); Ts.append(T); cap_of.append(c)
    lens = np.array([p.size for p in parts], dtype=np.uint64)
    return {"data": np.concatenate(parts), "cuts": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), "ids": np.array(ids, np.uint64),
            "base": np.array(base, np.int64), "T": np.array(Ts), "cap": np.array(cap_of), "parts": parts}


def window_class(T: int, caps) -> int:
    """The cap of the class a window of T bytes belongs to (size_class: the first cap with T <= cap)."""
    return next(c for c in caps if T <= c)


def oracle_view(job: dict):
    """The same jobs for the CPU oracle, whose `base` is an index into the selection: every chunk is selected, and a dictionary longer
    than 32768 bytes is replaced by its last 32768 (all a DEFLATE window can reach, include/hmse.h).  -> (data, cuts, base, rows):
    rows[j] = index of job j in the oracle's output."""
    parts = [p[-32768:] if p.size > 32768 else p for p in job["parts"]]
    lens = np.array([p.size for p in parts], dtype=np.uint64)
    base = np.full(len(parts), -1, np.int64)
    base[job["ids"].astype(np.int64)] = job["base"]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), base, job["ids"].astype(np.int64)


def encode_list_jobs(split: int, delta: bool, seed: int = 13):
    """Chunks of split - 1, split, split + 1, 32767 and 32768 bytes for the encode kernel's two lists; with `delta` each has a
    near-identical dictionary of its own length (quick-accepted DELTA records)."""
    text = words_text(80_000, seed=seed)
    parts, ids, base = [], [], []
    for j, L in enumerate((split - 1, split, split + 1, 32767, 32768)):
        c = text[100 * j: 100 * j + L].copy()
        if delta:
            d = c.copy(); d[L // 2] ^= 0x04
            parts.append(d); base.append(len(parts) - 1)
        else:
            base.append(-1)
        parts.append(c); ids.append(len(parts) - 1)
    lens = np.array([p.size for p in parts], dtype=np.uint64)
    return {"data": np.concatenate(parts), "cuts": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), "ids": np.array(ids, np.uint64),
            "base": np.array(base, np.int64), "parts": parts, "L": np.array([parts[i].size for i in ids])}


# ---- L4 MinHash: shingle counts on the pass boundary ----------------------------------------------------------------------------
def distinct_bytes(n: int) -> np.ndarray:
    """A byte sequence whose 4-byte shingles are all different: a three-digit base-250 counter (digits 1..250) and a zero byte.  The zero's
    place tells a shingle's alignment, the digits around it the counter."""
    i = np.arange((n + 3) // 4, dtype=np.int64) + 1
    assert i[-1] < 250 ** 3
    w = np.stack([i // 62500 % 250 + 1, i // 250 % 250 + 1, i % 250 + 1, np.zeros_like(i)], axis=1).astype(np.uint8)
    return w.reshape(-1)[:n].copy()


def minhash_lengths(sub: int):
    """Chunk lengths with L - 3 shingles on and around one and two passes, and the longest chunk."""
    return [s + 3 for s in (sub - 1, sub, sub + 1, 2 * sub - 1, 2 * sub, 2 * sub + 1)] + [32768]


def minhash_boundary_chunks(sub: int, seed: int = 17):
    """-> (data, cuts, facts): per content (distinct / abcd / text) one chunk per length of minhash_lengths(); then the sentinel chunks:
    32768 bytes of 'a' with ONE 'b', placed so that shingle sub - 1, then shingle sub (and the same at 2 * sub) is in turn the last and
    the first of the four shingles that contain it; then the plain run without a 'b'.  facts: rows of each group, shingle counts."""
    lens = minhash_lengths(sub)
    text = words_text(sum(lens) + 64, seed=seed)
    parts, group = [], {"distinct": [], "abcd": [], "text": [], "sentinel": [], "plain": []}
    o = 0
    for L in lens:
        group["distinct"].append(len(parts)); parts.append(distinct_bytes(L))
        group["abcd"].append(len(parts)); parts.append(np.tile(np.frombuffer(b"abcd", np.uint8), L // 4 + 1)[:L].copy())
        group["text"].append(len(parts)); parts.append(text[o: o + L].copy()); o += L
    odd_at = []
    for edge in (sub, 2 * sub):
        for sh in (edge - 1, edge):
            for p in (sh, sh + 3):          # shingle sh is the LAST one holding byte sh, and the FIRST one holding byte sh + 3
                c = np.full(32768, 0x61, np.uint8); c[p] = 0x62
                group["sentinel"].append(len(parts)); parts.append(c); odd_at.append(p)
    group["plain"].append(len(parts)); parts.append(np.full(32768, 0x61, np.uint8))
    ln = np.array([p.size for p in parts], dtype=np.uint64)
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64), {"rows": group, "shingles": ln.astype(np.int64) - 3,
                                                                                        "odd_at": odd_at, "parts": parts}


# ---- L3 / L4 open-addressing tables --------------------------------------------------------------------------------------------
def table_slots(n: int) -> int:
    """The tables' size rule (hmse_l3_index_slots / hmse_l4_lsh_slots below their caps): the power of two >= 2 n, at least 1024."""
    m = 1024
    while m < 2 * n:
        m <<= 1
    return m


def planted_digests(n_random: int, seed: int = 23):
    """-> (digests u8[n][32], facts).  4096 different digests with the SAME first four bytes (one home slot, a probe run of 4096), each
    occurring 1 to 5 times; 4096 different digests starting FF FF FF FF (home slot = the table's last slot whatever its size: every
    probe wraps to slot 0); n_random random ones; all shuffled."""
    rng = np.random.default_rng(seed)
    same = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    same[:, :4] = (0x12, 0x34, 0x56, 0x78)
    same[:, 4:8] = np.arange(4096, dtype=">u4").view(np.uint8).reshape(-1, 4)      # distinct tails, whatever the generator gave
    same = np.repeat(same, rng.integers(1, 6, 4096), axis=0)
    last = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    last[:, :4] = 0xFF
    last[:, 4:8] = np.arange(4096, dtype=">u4").view(np.uint8).reshape(-1, 4)
    rnd = rng.integers(0, 256, (n_random, 32), dtype=np.uint8)
    dg = np.concatenate([same, last, rnd, rnd[: n_random // 7]])
    dg = dg[rng.permutation(dg.shape[0])]
    return np.ascontiguousarray(dg), {"same_prefix": (0x12, 0x34, 0x56, 0x78), "n": dg.shape[0]}


def lsh_population(n: int, bands: int, rows: int, seed: int = 29, planted: int = 20000):
    """n random signatures (enough for pairs of DIFFERENT band rows with EQUAL 32-bit keys, by the birthday bound n^2 / 2^33 per band),
    with whole bands copied from earlier signatures across the population."""
    rng = np.random.default_rng(seed)
    sig = rng.integers(0, 1 << 32, (n, bands * rows), dtype=np.uint64).astype(np.uint32)
    dst = rng.integers(n // 50, n, planted)
    src = (rng.random(planted) * dst).astype(np.int64)
    b = rng.integers(0, bands, planted)
    for i, j, bb in zip(dst, src, b):
        sig[i, rows * bb: rows * bb + rows] = sig[j, rows * bb: rows * bb + rows]
    return sig


def equal_key_different_rows(sig: np.ndarray, keys: np.ndarray, rows: int) -> list:
    """Per band: the number of adjacent pairs, in key order, of equal keys over different band rows."""
    out = []
    for b in range(keys.shape[1]):
        o = np.argsort(keys[:, b], kind="stable")
        eq = np.flatnonzero(keys[o[1:], b] == keys[o[:-1], b])
        band = sig[:, rows * b: rows * b + rows]
        out.append(int(sum(1 for e in eq if not np.array_equal(band[o[e]], band[o[e + 1]]))))
    return out


# ---- band tables and index sort ----------------------------------------------------------------------------------------------------
def hot_bucket_keys(n: int, hot: int, spread: bool, bands: int = 2, seed: int = 31):
    """u32 keys [n, bands]: band 1 has one 16-bit bucket (0x1234) of exactly `hot` ids — contiguous ids from 1000 on, or spread evenly
    over the whole id range — and no other id in it; the rest random."""
    rng = np.random.default_rng(seed + hot)
    keys = rng.integers(0, 1 << 32, (n, bands), dtype=np.uint64).astype(np.uint32)
    low = keys[:, 1] & np.uint32(0xFFFF)
    keys[low == 0x1234, 1] ^= np.uint32(1)
    ids = (np.arange(hot) * n // hot) if spread else (1000 + np.arange(hot))
    assert ids[-1] < n and np.unique(ids).size == hot
    keys[ids, 1] = (keys[ids, 1] & np.uint32(0xFFFF0000)) | np.uint32(0x1234)
    return keys, {"hot_ids": ids, "bucket": 0x1234}


LSH_N = 300_000                                                     # about n^2 / 2^33 = 10 equal-key pairs per band
BT_N = [255, 256, 257, 511, 512, 513, 65535, 65536, 65537]          # around a BT_NT tile and around 2^16
BT_HOT = [65534, 65535, 65536, 131070, 131071]                      # around one and two BT_PIECE pieces
