"""The dictionary-search kernels (hmse_amd/csrc/findset.hip) on the CPU against a brute-force search: no GPU needed.
    python tools/findset_emu.py [--iters 20] [--seed 12345] [--sanitize]
Cuts the kernels out of findset.hip (everything between its geometry constants and its entry points), compiles them with tools/findset_emu.cpp
(g++ -std=c++20: one std::thread per lane, std::barrier for __syncthreads, a plain prefix sum for block_exclusive_scan) and runs random
cases through validate, scan, seams and place (and a damaged set the validate kernel must refuse).  --sanitize builds with
-fsanitize=address,undefined (host code only).  Prints how many cases ran; exit status 0 = all equal."""
import sys

from emu_common import run

if __name__ == "__main__":
    sys.exit(run(__doc__, "findset", "constexpr int FSET_NT", "// ---- entry points", 20))
