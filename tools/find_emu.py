"""The find kernels (hmse_amd/csrc/find.hip) on the CPU against a brute-force search: no GPU needed.
    python tools/find_emu.py [--iters 30] [--seed 12345] [--sanitize]
Cuts the kernels out of find.hip (everything between its geometry constants and its entry points), compiles them with tools/find_emu.cpp
(g++ -std=c++20: one std::thread per lane, std::barrier for __syncthreads, a plain prefix sum for block_exclusive_scan) and runs random
cases through scan, seams and place.  --sanitize builds with -fsanitize=address,undefined (host code only).  Exit status 0 = all equal."""
import sys

from emu_common import run

if __name__ == "__main__":
    sys.exit(run(__doc__, "find", "constexpr int FIND_NT", "// ---- entry points", 30))
