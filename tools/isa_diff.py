"""Per-kernel comparison of the gfx950 code of two trees: python tools/isa_diff.py PARENT_TREE CHANGE_TREE [old_kernel=new_kernel ...] [--only a.hip,b.hip]
Compiles the device side of every hmse_amd/csrc/*.hip of both trees to assembly (no GPU needed), splits it per kernel, numbers the local
labels in order of appearance and replaces mangled names, then prints per kernel `identical` or both instruction counts.  A kernel that
was renamed is paired by an old=new argument (demangled names without their argument lists, as this script prints them)."""
import concurrent.futures, glob, os, re, subprocess, sys, tempfile


def kernels(tree, hip):
    """{demangled name: [normalised instruction, ...]} of one .hip file"""
    src = os.path.join(tree, "hmse_amd", "csrc", hip)
    out = os.path.join(tempfile.mkdtemp(), "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", out, src],
                   check=True, stderr=subprocess.DEVNULL, cwd=os.path.dirname(src))
    txt = open(out).read()
    res = {}
    for sym in re.findall(r"^\t\.amdhsa_kernel (\S+)$", txt, re.M):
        body = txt[txt.index("\n%s:" % sym):]
        body = body[:body.index(".Lfunc_end")]
        labels, ins = {}, []
        for line in body.split("\n")[2:]:
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") and not line.endswith(":"):
                continue
            line = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), line)
            line = re.sub(r"\b_Z\w+", "SYM", line)
            ins.append(line)              # (a label keeps its place: the same branches must reach the same instructions)
        name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        res[re.sub(r"^void ", "", re.sub(r"\((?!anonymous).*", "", name))] = ins
    return res


def main():
    args = sys.argv[1:]
    only = None
    if "--only" in args:
        i = args.index("--only")
        only = args[i + 1].split(",")
        del args[i:i + 2]
    parent, change = args[0], args[1]
    renamed = dict(a.split("=", 1) for a in args[2:])
    files = sorted({os.path.basename(p) for t in (parent, change) for p in glob.glob(os.path.join(t, "hmse_amd", "csrc", "*.hip"))})
    if only:
        files = [f for f in files if f in only]
    jobs = [(t, f) for f in files for t in (parent, change) if os.path.exists(os.path.join(t, "hmse_amd", "csrc", f))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        asm = dict(zip(jobs, ex.map(lambda j: kernels(*j), jobs)))
    n_ins = lambda k: sum(1 for x in k if not x.endswith(":"))
    differ = 0
    for f in files:
        a, b = asm.get((parent, f), {}), dict(asm.get((change, f), {}))
        for name, ka in a.items():
            new = renamed.get(name, name)
            kb = b.pop(new, None)
            label = name if new == name else "%s -> %s" % (name, new)
            if kb is None:
                print("%-14s %-96s gone (%d instructions)" % (f, label, n_ins(ka)))
            elif ka == kb:
                print("%-14s %-96s identical (%d instructions)" % (f, label, n_ins(ka)))
            else:
                differ += 1
                print("%-14s %-96s DIFFERS: %d instructions in the parent, %d in the change" % (f, label, n_ins(ka), n_ins(kb)))
        for name, kb in b.items():
            print("%-14s %-96s new (%d instructions)" % (f, name, n_ins(kb)))
    print("%d kernels differ" % differ)


if __name__ == "__main__":
    main()
