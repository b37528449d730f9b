"""The regex-search kernels (hmse_amd/csrc/regex_core.h, the plain form of regex.hip) on the CPU against a brute-force search: no GPU needed.
    python tools/regex_emu.py [--iters 20] [--seed 12345] [--sanitize]
Compiles tools/regex_emu.cpp with -DRX_ASSERTING=0 — it includes regex_core.h as it is; the place kernel comes with chunkmap.h — (g++
-std=c++20: one std::thread per lane, std::barrier for __syncthreads, a plain prefix sum for block_exclusive_scan) and runs random cases
through validate, scan, place and seams (and a damaged automaton the validate kernel must refuse).  The automata come from
hmse_amd/regex.py (numpy only) and are handed to the program in a file.  --sanitize builds that program with
-fsanitize=address,undefined (host code only).  Prints how many cases ran; exit status 0 = all equal.  tools/regexa_emu.py is the same
for the form with assertions."""
import os
import sys

from emu_common import ROOT, run

sys.path.insert(0, ROOT)
PATTERNS = [(rb"q", 0), (rb"ab", 0), (rb"ab", 1), (rb"a+", 0), (rb"[ab]+c", 0), (rb"(a|aa)*b", 0), (rb"a{2,4}[^a]", 0), (rb"[^\n]*c", 0),
            (rb"a.{0,7}b", 2), (rb"(ab|b)c?", 1), (rb"b{255}a", 0), (rb"[ab]{16}", 0), (rb"\w+\s", 0)]


def automata(td, patterns, asserting):
    """per automaton: n_states n_classes reach (asserting: and the four starts), 256 classes, the table"""
    from hmse_amd.regex import Regex
    path = os.path.join(td, "automata.txt")
    with open(path, "w") as f:
        f.write(f"{len(patterns)}\n")
        for pat, fl in patterns:
            r = Regex(pat, bool(fl & 1), bool(fl & 2), assertions=asserting)
            head = [r.n_states, r.n_classes, r.reach] + (list(r.start) if asserting else [])
            f.write("\n".join(" ".join(map(str, line)) for line in (head, r.classmap.tolist(), r.table.tolist())) + "\n")
    return [path]


if __name__ == "__main__":
    sys.exit(run(__doc__, "regex", None, None, 20, lambda td: automata(td, PATTERNS, False), defines=["RX_ASSERTING=0"]))
