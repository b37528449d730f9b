"""What the ten tools/*_emu.py share: cut the kernels out of a .hip file (everything between two markers) into <name>_kernels.inc, compile
tools/<name>_emu.cpp with it into a stand-alone program (g++ -std=c++20, tools/hip_on_cpu.h under the kernels), run it."""
import argparse
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(doc, name, first, last, iters, extra=None, hip=None):
    """--iters / --seed / --sanitize; extra(td) -> further arguments of the program (files it wrote into td; it may also rewrite the cut
    there); hip = the .hip file's name where it is not `name`; returns the exit status"""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--sanitize", action="store_true")
    a = ap.parse_args()
    csrc = os.path.join(ROOT, "hmse_amd", "csrc")
    src = open(os.path.join(csrc, (hip or name) + ".hip")).read()
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, (hip or name) + "_kernels.inc"), "w").write(src[src.index(first): src.index(last)])
        more = extra(td) if extra else []
        exe = os.path.join(td, name + "_emu")
        cmd = ["g++", "-std=c++20", "-O1", "-g", "-pthread", "-Wno-attributes", "-I", td, "-I", os.path.join(ROOT, "include"), "-I", csrc,
               os.path.join(ROOT, "tools", name + "_emu.cpp"), "-o", exe]
        if a.sanitize:
            cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        subprocess.check_call(cmd)
        return subprocess.call([exe, str(a.iters), str(a.seed)] + more)
