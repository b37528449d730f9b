"""The export kernels (hmse_amd/csrc/export.hip) on the CPU against the definitions of include/hmse.h: no GPU needed.
    python tools/export_emu.py [--iters 12] [--seed 12345] [--sanitize]
Cuts the kernels out of export.hip (everything between its geometry constants and its entry points; wave_copy comes with blockops.h),
compiles them with tools/export_emu.cpp (g++ -std=c++20: one std::thread per lane, std::barrier for __syncthreads, a plain prefix sum
for block_exclusive_scan) and runs random cases — ranges of every length around the strip and tile sizes, empty ones, odd starts, junk
around the data, refused tables — through the CRC-32, the combination and the member layout.  The program's bit-by-bit CRC-32 is first
held against known answers that this script takes from zlib.  --sanitize builds that program with -fsanitize=address,undefined (host
code only).  Prints how many cases ran; exit status 0 = all equal."""
import os
import random
import struct
import sys
import zlib

from emu_common import run


def known_answers(td):
    rnd = random.Random(2024)
    path = os.path.join(td, "crc32_known.bin")
    with open(path, "wb") as f:
        for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 1000, 32768):
            for fill in (None, 0x00, 0xFF):
                b = bytes(rnd.randrange(256) for _ in range(n)) if fill is None else bytes([fill]) * n
                f.write(struct.pack("<I", n) + b + struct.pack("<I", zlib.crc32(b)))
    return [path]


if __name__ == "__main__":
    sys.exit(run(__doc__, "export", "constexpr int EX_NT", "// ---- entry points", 12, extra=known_answers))
