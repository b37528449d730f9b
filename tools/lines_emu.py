"""The kernels of hmse_amd/csrc/lines.hip on the CPU against the brute-force definition of a line's extent: no GPU needed.
    python tools/lines_emu.py [--iters 200] [--seed 12345] [--sanitize]
Cuts the kernels out of lines.hip (everything between the geometry constants and the entry points), compiles them with
tools/lines_emu.cpp (g++ -std=c++20: one std::thread per lane, a std::barrier per wavefront under __ballot, so a loop that is not
wave-uniform hangs it) into a STAND-ALONE program and runs random chunk maps through it: chunks of 0, 1 and 2 bytes, junk around the
records in raw, heap blocks of exactly the declared size.  --sanitize builds that program with -fsanitize=address,undefined (host code
only: a read one byte outside a table or raw is reported).  Exit status 0 = every extent and every gathered byte equals the definition."""
import sys

from emu_common import run

if __name__ == "__main__":
    sys.exit(run(__doc__, "lines", "constexpr int LINES_NT", "// ---- entry points", 200))
