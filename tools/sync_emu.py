"""The match kernel of replication (hmse_amd/csrc/sync.hip) on the CPU against memcmp: no GPU needed.
    python tools/sync_emu.py [--iters 100] [--seed 12345] [--sanitize]
Cuts the kernel out of sync.hip (everything between its geometry constants and its entry point), compiles it with tools/sync_emu.cpp
(g++ -std=c++20: one std::thread per lane, a std::barrier per wavefront under __ballot) into a stand-alone program and runs random record
tables through it.  --sanitize builds with -fsanitize=address,undefined (host code only; the blobs are heap blocks of exactly the declared
size, so a read outside one is reported).  Exit status 0 = every answer equals memcmp's."""
import sys

from emu_common import run

if __name__ == "__main__":
    sys.exit(run(__doc__, "sync", "constexpr int SYNC_NT", "// ---- entry point", 100))
