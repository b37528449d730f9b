"""The dictionary-search kernels (hmse_amd/csrc/findset.hip) on the CPU against a brute-force search: no GPU needed.
    python tools/findset_emu.py [--iters 20] [--seed 12345] [--sanitize]
Cuts the kernels out of findset.hip (everything between its geometry constants and its entry points), compiles them with tools/findset_emu.cpp
(g++ -std=c++20: one std::thread per lane, std::barrier for __syncthreads, a plain prefix sum for block_exclusive_scan) and runs random
cases through validate, scan, seams and place (and a damaged set the validate kernel must refuse).  --sanitize builds with
-fsanitize=address,undefined (host code only).  Prints how many cases ran; exit status 0 = all equal."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--sanitize", action="store_true")
    a = ap.parse_args()
    src = open(os.path.join(ROOT, "hmse_amd", "csrc", "findset.hip")).read()
    kernels = src[src.index("constexpr int FSET_NT"): src.index("// ---- entry points")]
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "findset_kernels.inc"), "w").write(kernels)
        exe = os.path.join(td, "findset_emu")
        cmd = ["g++", "-std=c++20", "-O1", "-g", "-pthread", "-Wno-attributes", "-I", td, "-I", os.path.join(ROOT, "include"),
               "-I", os.path.join(ROOT, "hmse_amd", "csrc"),
               os.path.join(ROOT, "tools", "findset_emu.cpp"), "-o", exe]
        if a.sanitize:
            cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        subprocess.check_call(cmd)
        return subprocess.call([exe, str(a.iters), str(a.seed)])


if __name__ == "__main__":
    sys.exit(main())
