"""The kernels of hmse_amd/csrc/order.hip on the CPU against the definition of a range's key at a depth and of two ranges' common prefix:
no GPU needed.
    python tools/order_emu.py [--iters 200] [--seed 12345] [--sanitize]
Cuts the kernels out of order.hip (everything between the geometry constants and the entry points), compiles them with
tools/order_emu.cpp (g++ -std=c++20: one std::thread per lane, a std::barrier per wavefront under __ballot, so a loop that is not
wave-uniform hangs it) into a STAND-ALONE program and runs random chunk maps through it: chunks of 0, 1 and 2 bytes, a single chunk, mixes
with empty chunks, junk around the records in raw, heap blocks of exactly the declared size, poisoned outputs with a guard behind them,
and every refusal (bad ranges, a depth beyond the text, a bad rep, a from beyond the shorter text, inconsistent tables).  --sanitize
builds that program with -fsanitize=address,undefined (host code only: a read one byte outside a table or raw is reported).  Exit
status 0 = every key and every common prefix equals the definition; the "KEY start end depth fold key" lines at the end are the keys of
fixed ranges of the corpus C[q] = (37 q + 11) & 0xFF with 0x00 and 0xFF planted where windows end, for tests/test_order_host.py."""
import sys

from emu_common import run

if __name__ == "__main__":
    sys.exit(run(__doc__, "order", "constexpr int ORDER_NT", "// ---- entry points", 200))
