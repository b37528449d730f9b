"""STUDY (test infrastructure: loads oracle/): the long compares of a dictionary job's unhinted positions, and how many of them the
anchors of the next two blocks already know.  CPU only; the walks are the oracle's, the cost is the trip model
of tools/study/lz_study.c.
    python tools/dict_known_runs.py [MiB of wiki-synth, seed 42] [output file]"""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import oracle as O
import lz_study as S

if __name__ == "__main__":
    mib = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    from hmse_amd import corpus
    S.build(); L = C.CDLL(S.SO)
    L.study_dict_known.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    d = corpus.wiki_synth(mib << 20, seed=42); cfg = O.default_cfg()
    cuts = O.cdc(d, cfg); fo, _ = O.dedup(O.sha256_chunks(d, cuts))
    uniq = np.nonzero(fo == np.arange(len(fo)))[0].astype(np.uint64)
    _, base = O.lsh(O.minhash_chunks(d, cuts, cfg, uniq), cfg)
    out = np.zeros(16, np.uint64); jobs = 0
    for k in np.nonzero(base >= 0)[0]:
        c, b = int(uniq[k]), int(uniq[base[k]])
        ch, di = d[int(cuts[c]):int(cuts[c + 1])], d[int(cuts[b]):int(cuts[b + 1])]
        L.study_dict_known(ch.ctypes.data, ch.size, di.ctypes.data, di.size, 32, out.ctypes.data); jobs += 1
    o = [int(v) for v in out]
    assert o[12] == 0, f"{o[12]} known lengths differ from the compared ones"
    left = o[3] - o[5] - o[7]
    lines = [
        f"wiki-synth {mib} MiB, seed 42: {len(uniq)} unique chunks, {jobs} dictionary jobs, {o[0]} chunk positions",
        f"positions walked (no hint of 16 bytes)         {o[1]:9d}  {100 * o[1] / max(1, o[0]):5.1f} % of the positions",
        f"  of them with a fact from anchor a0+1 / a0+2  {o[11]:9d}  {100 * o[11] / max(1, o[1]):5.1f} % of the walked",
        f"probe trips of the walked positions            {o[10]:9d}  {o[10] / max(1, o[1]):5.2f} per walked position",
        f"candidates that enter EXTEND (16 bytes agree)  {o[2]:9d}  {o[2] / max(1, o[1]):5.2f} per walked position",
        f"EXTEND lane-trips (32 bytes each)              {o[3]:9d}  {o[3] / max(1, o[1]):5.2f} per walked position",
        f"  on the diagonal of anchor a0+1, in its backward stretch   {o[5]:9d}  {100 * o[5] / max(1, o[3]):5.1f} %  ({o[4]} candidates)",
        f"  anchor a0+2 only                                          {o[7]:9d}  {100 * o[7] / max(1, o[3]):5.1f} %  ({o[6]} candidates)",
        f"  left by fact (a)                                          {left:9d}  {100 * left / max(1, o[3]):5.1f} %",
        f"  of those: resumed diagonal of anchor a0 / a0-1 (fact b)   {o[9]:9d}  {100 * o[9] / max(1, left):5.1f} % of what (a) leaves  ({o[8]} candidates)",
    ]
    print("\n".join(lines))
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write("\n".join(lines) + "\n")
