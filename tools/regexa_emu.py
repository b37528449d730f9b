"""The kernels of the regex search with assertions (hmse_amd/csrc/regex_core.h, the asserting form of regexa.hip) on the CPU against a
brute-force walk: no GPU needed.
    python tools/regexa_emu.py [--iters 20] [--seed 12345] [--sanitize]
Compiles tools/regex_emu.cpp with -DRX_ASSERTING=1 — it includes regex_core.h as it is; the place kernel comes with chunkmap.h — (g++
-std=c++20: one std::thread per lane, std::barrier for __syncthreads, a plain prefix sum for block_exclusive_scan) and runs random cases
through validate, scan, place and seams — random chunk maps with empty chunks and duplicates, every assertion evaluated against the real
bytes around the match — and one damaged automaton per cause the validate kernel must refuse (the first five cases take the five causes
in turn).  The automata come from hmse_amd/regex.py (numpy only) and are handed to the program in a file.  --sanitize builds that program
with -fsanitize=address,undefined (host code only).  Prints how many cases ran; exit status 0 = all equal."""
import sys

from emu_common import run
from regex_emu import automata

PATTERNS = [(rb"^a", 0), (rb"a$", 0), (rb"\bab\b", 1), (rb"\Ba+", 0), (rb"^[ab]+c", 0), (rb"(^|-)a*b", 0), (rb"a{2,4}\b", 0), (rb"^[^\n]*c$", 0),
            (rb"\ba.{0,7}b\b", 2), (rb"(ab|b)c?$", 1), (rb"b{255}a\b", 0), (rb"\b[ab]{16}", 0), (rb"\w+$", 0), (rb"\A\w+|\w+\Z", 0),
            (rb"a{256}$", 0), (rb"ab", 0), (rb"q+\b", 0), (rb"^$\n|-\B-", 0)]


if __name__ == "__main__":
    sys.exit(run(__doc__, "regexa", None, None, 20, lambda td: automata(td, PATTERNS, True), source="regex_emu.cpp", defines=["RX_ASSERTING=1"]))
