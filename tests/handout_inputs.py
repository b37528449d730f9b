"""Inputs of tests/test_gpu_handout_in_sort.py and tests/handout_check.py: PLAIN DEFLATE jobs whose hand-out list is written by the ordered
sort (classes S and S2: windows up to 10048 / 13952 bytes), at the lengths where that code changes its path, with contents that fill the
list's four classes in different ways.  Jobs have the form of edge_inputs.deflate_boundary_jobs (no dictionaries)."""
from __future__ import annotations

import numpy as np

from conftest import words_text

# nh = L - 3 hashed positions; the scatter takes 1024 of them per step
LENGTHS = (3, 4, 7,                 # nh = 0, 1, 4
           1026, 1027, 1028,        # nh on and around one scatter step
           2051,                    # two steps
           10047, 10048, 10049,     # the cap of class S (10049: class S2)
           13951, 13952, 13953)     # the cap of class S2 (13953: class SG, whose list is still written by the two passes: the control)
DEPTH_LENGTHS = (1027, 10048)
CONTENTS = ("byte", "random", "period5", "period7", "words")


def content(kind: str, L: int, salt: int) -> np.ndarray:
    if kind == "byte":        # ONE bucket: in-bucket indices 0 .. nh - 1, every class of the list non-empty
        return np.full(L, 0x61, np.uint8)
    if kind == "random":      # ~2.5 positions per bucket: the classes of 4 candidates and more stay (nearly) empty
        return np.random.Generator(np.random.PCG64(1000 + salt)).integers(0, 256, L, dtype=np.uint8)
    if kind in ("period5", "period7"):   # 5 / 7 buckets of hundreds of members, inside one scatter step and across steps
        p = int(kind[-1])
        return np.tile(np.frombuffer(b"qwertyu"[:p], np.uint8), L // p + 1)[:L].copy()
    if kind == "words":
        return words_text(16000, seed=7)[100 + 13 * salt: 100 + 13 * salt + L].copy()
    raise ValueError(kind)


def plain_jobs(lengths, contents=CONTENTS) -> dict:
    parts = [content(k, L, i) for k in contents for i, L in enumerate(lengths)]
    assert all(p.size == L for p, L in zip(parts, list(lengths) * len(contents)))
    lens = np.array([p.size for p in parts], dtype=np.uint64)
    n = len(parts)
    return {"data": np.concatenate(parts), "cuts": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), "ids": np.arange(n, dtype=np.uint64),
            "base": np.full(n, -1, np.int64), "T": lens.astype(np.int64), "parts": parts}


def depth_cfgs(max_depth: int):
    """level 1 (depth 2: every listed rank in the last class); depths on and beside the class thresholds 4, 12, 24; the default (32);
    the largest depth the configuration accepts (above 62: the entry's count saturates and the matcher's pull recomputes it)."""
    from hmse_amd import IngestConfig
    return [("level1", IngestConfig(level=1))] + [("depth%d" % d, IngestConfig(chain_depth=d)) for d in (3, 4, 12, 24)] + \
           [("default", IngestConfig()), ("depth%d" % max_depth, IngestConfig(chain_depth=max_depth))]
