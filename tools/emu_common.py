"""What the thirteen tools/*_emu.py share: cut the kernels out of a .hip file (everything between two markers) into <name>_kernels.inc, compile
tools/<name>_emu.cpp with it into a stand-alone program (g++ -std=c++20, tools/hip_on_cpu.h under the kernels), run it.  The two regex
emulators cut nothing: tools/regex_emu.cpp includes hmse_amd/csrc/regex_core.h as it is and is compiled once per form."""
import argparse
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(doc, name, first, last, iters, extra=None, hip=None, source=None, defines=()):
    """--iters / --seed / --sanitize; extra(td) -> further arguments of the program (files it wrote into td; it may also rewrite the cut
    there); hip = the .hip file's name where it is not `name`; first = None: nothing is cut out (the program includes a header of csrc
    itself); source = the program's source where it is not <name>_emu.cpp, defines = its -D switches; returns the exit status"""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--sanitize", action="store_true")
    a = ap.parse_args()
    csrc = os.path.join(ROOT, "hmse_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        if first is not None:
            src = open(os.path.join(csrc, (hip or name) + ".hip")).read()
            open(os.path.join(td, (hip or name) + "_kernels.inc"), "w").write(src[src.index(first): src.index(last)])
        more = extra(td) if extra else []
        exe = os.path.join(td, name + "_emu")
        cmd = ["g++", "-std=c++20", "-O1", "-g", "-pthread", "-Wno-attributes", "-I", td, "-I", os.path.join(ROOT, "include"), "-I", csrc,
               *("-D" + d for d in defines), os.path.join(ROOT, "tools", source or name + "_emu.cpp"), "-o", exe]
        if a.sanitize:
            cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        subprocess.check_call(cmd)
        return subprocess.call([exe, str(a.iters), str(a.seed)] + more)
