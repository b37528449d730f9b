"""The kernels of hmse_amd/csrc/subst.hip on the CPU against the definition of include/hmse_subst.h (the naive splice): no GPU needed.
    python tools/subst_emu.py [--iters 200] [--seed 12345] [--sanitize]
Cuts the kernels out of subst.hip (everything between the geometry constants and the entry points), compiles them with
tools/subst_emu.cpp (g++ -std=c++20: one std::thread per lane of the writing kernel, a std::barrier under __syncthreads and one per
wavefront under __ballot, so a loop that is not wave-uniform hangs it) into a STAND-ALONE program and runs it: every single edit of a
corpus of five strips + 7 bytes with replacement lengths 0, 1, 15, 16, 17 and two strips + 1 and in fill mode (--iters below 100: every
41st of them), then per iteration a random chunk map (chunks of 0, 1 and 2 bytes, a single chunk, junk around the records), a random edit
list (ties, insertions, deletions, runs of one-byte deletions) in either mode, and the same call with one thing wrong at a time, which
must be refused with out untouched.  Heap blocks have exactly the declared size and out is poisoned, at every alignment.  --sanitize
builds that program with -fsanitize=address,undefined (host code only: a read or write one byte outside is reported).  Exit status 0 =
every output equals the splice and every refusal left out as it was."""
import sys

from emu_common import run

if __name__ == "__main__":
    sys.exit(run(__doc__, "subst", "constexpr int SUBST_NT", "// ---- entry points", 200))
