"""The match kernel of replication (hmse_amd/csrc/sync.hip) on the CPU against memcmp: no GPU needed.
    python tools/sync_emu.py [--iters 100] [--seed 12345] [--sanitize]
Cuts the kernel out of sync.hip (everything between its geometry constants and its entry point), compiles it with tools/sync_emu.cpp
(g++ -std=c++20: one std::thread per lane, a std::barrier per wavefront under __ballot) into a stand-alone program and runs random record
tables through it.  --sanitize builds with -fsanitize=address,undefined (host code only; the blobs are heap blocks of exactly the declared
size, so a read outside one is reported).  Exit status 0 = every answer equals memcmp's."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--sanitize", action="store_true")
    a = ap.parse_args()
    src = open(os.path.join(ROOT, "hmse_amd", "csrc", "sync.hip")).read()
    kernels = src[src.index("constexpr int SYNC_NT"): src.index("// ---- entry point")]
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "sync_kernels.inc"), "w").write(kernels)
        exe = os.path.join(td, "sync_emu")
        cmd = ["g++", "-std=c++20", "-O1", "-g", "-pthread", "-Wno-attributes", "-I", td, "-I", os.path.join(ROOT, "include"),
               os.path.join(ROOT, "tools", "sync_emu.cpp"), "-o", exe]
        if a.sanitize:
            cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        subprocess.check_call(cmd)
        return subprocess.call([exe, str(a.iters), str(a.seed)])


if __name__ == "__main__":
    sys.exit(main())
