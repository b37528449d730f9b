"""The kernels of hmse_amd/csrc/tally.hip on the CPU against the definition of a range's key and of two ranges' equality: no GPU needed.
    python tools/tally_emu.py [--iters 200] [--seed 12345] [--sanitize]
Cuts the kernels out of tally.hip (everything between the geometry constants and the entry points), compiles them with
tools/tally_emu.cpp (g++ -std=c++20: one std::thread per lane, a std::barrier per wavefront under __ballot and the lane reads, so a loop
that is not wave-uniform hangs it) into a STAND-ALONE program and runs random chunk maps through it: chunks of 0, 1 and 2 bytes, a single
chunk, junk around the records in raw, heap blocks of exactly the declared size, poisoned outputs, bad ranges, bad rep, inconsistent
tables.  --sanitize builds that program with -fsanitize=address,undefined (host code only: a read one byte outside a table or raw is
reported).  Exit status 0 = every key and every answer equals the definition; the "KEY start end fold seed bits key" lines at the end
are the keys of fixed ranges of the corpus C[q] = (37 q + 11) & 0xFF, for tests/test_tally_host.py."""
import sys

from emu_common import run

if __name__ == "__main__":
    sys.exit(run(__doc__, "tally", "constexpr int TALLY_NT", "// ---- entry points", 200))
