"""The approximate-search kernels (hmse_amd/csrc/approx.hip) on the CPU against Sellers' dynamic programme: no GPU needed.
    python tools/approx_emu.py [--iters 20] [--seed 12345] [--sanitize]
Cuts the kernels out of approx.hip (everything between its geometry constants and its entry points; the validate and place kernels come
with chunkmap.h), compiles them with tools/approx_emu.cpp (g++ -std=c++20: one std::thread per lane, std::barrier for __syncthreads, a
plain prefix sum for block_exclusive_scan) and runs random cases — chunk maps with tiny and empty chunks, noisy copies of the patterns
planted — through validate, scan, place, seams and spans.  --sanitize builds that program with -fsanitize=address,undefined (host code
only).  Prints how many cases ran; exit status 0 = all equal."""
import sys

from emu_common import run

if __name__ == "__main__":
    sys.exit(run(__doc__, "approx", "constexpr int AX_NT", "// ---- entry points", 20))
