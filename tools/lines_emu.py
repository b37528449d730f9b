"""The kernels of hmse_amd/csrc/lines.hip on the CPU against the brute-force definition of a line's extent: no GPU needed.
    python tools/lines_emu.py [--iters 200] [--seed 12345] [--sanitize]
Cuts the kernels out of lines.hip (everything between the geometry constants and the entry points), compiles them with
tools/lines_emu.cpp (g++ -std=c++20: one std::thread per lane, a std::barrier per wavefront under __ballot, so a loop that is not
wave-uniform hangs it) into a STAND-ALONE program and runs random chunk maps through it: chunks of 0, 1 and 2 bytes, junk around the
records in raw, heap blocks of exactly the declared size.  --sanitize builds that program with -fsanitize=address,undefined (host code
only: a read one byte outside a table or raw is reported).  Exit status 0 = every extent and every gathered byte equals the definition."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--sanitize", action="store_true")
    a = ap.parse_args()
    src = open(os.path.join(ROOT, "hmse_amd", "csrc", "lines.hip")).read()
    kernels = src[src.index("constexpr int LINES_NT"): src.index("// ---- entry points")]
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "lines_kernels.inc"), "w").write(kernels)
        exe = os.path.join(td, "lines_emu")
        cmd = ["g++", "-std=c++20", "-O1", "-g", "-pthread", "-Wno-attributes", "-I", td, "-I", os.path.join(ROOT, "include"),
               "-I", os.path.join(ROOT, "hmse_amd", "csrc"),
               os.path.join(ROOT, "tools", "lines_emu.cpp"), "-o", exe]
        if a.sanitize:
            cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        subprocess.check_call(cmd)
        return subprocess.call([exe, str(a.iters), str(a.seed)])


if __name__ == "__main__":
    sys.exit(main())
