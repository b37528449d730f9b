"""Spill and instruction audit of the DEFLATE kernels, per natural loop.

    python tools/spill_audit.py [path/to/libhmse_hip.so]           # the shipped code objects, loops named by offset
    python tools/spill_audit.py --source [-DFLAG ...]              # a -gline-tables-only build of l1_deflate.hip: loops named by source phase

CPU only.  A wavefront of these kernels holds more wave-uniform state than it has SGPRs; the compiler parks the overflow in lanes of
VGPRs (`v_writelane_b32` to park, `v_readlane_b32` to reload).  Both are VECTOR instructions in kernels whose time follows the number
of vector instructions they issue, and the VGPRs they occupy come out of the 64 that eight wavefronts per SIMD allow.  Per kernel and
natural loop (the control-flow graph and the loops are tools/isa_audit.py's) this prints: vector instructions, spill reloads / spill
writes — a lane move whose VGPR the kernel only ever writes with `v_writelane_b32` is spill traffic, any other `v_readlane_b32` is a
genuine cross-lane read —, scratch loads / stores, and the code object's metadata (SGPR / VGPR spill counts, scratch bytes, VGPRs).
Counts of a loop include its inner loops; `own` excludes them.  tests/test_spill_audit_host.py asserts the conditions."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_audit  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "hmse_amd", "csrc", "l1_deflate.hip")
LIB = os.path.join(ROOT, "hmse_amd", "csrc", "libhmse_hip.so")
META_KEYS = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
VREG_RE = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
SRC_LINE_RE = re.compile(r"^; (\S+):(\d+)\s*$")
PHASE_RE = re.compile(r"^\s*// -{4} (.+?) -{3,}\s*$")


def metadata(elf_bytes):
    """{mangled kernel name: {key: int}} from the code object's NT_AMDGPU_METADATA note."""
    with tempfile.NamedTemporaryFile(suffix=".elf") as f:
        f.write(elf_bytes); f.flush()
        txt = subprocess.run([f"{isa_audit.LLVM}/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
    out = {}
    for blk in txt.split("  - .agpr_count:")[1:]:
        blk = blk.split("amdhsa.target:")[0]
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        out[name] = {k: int(re.search(r"^\s+\.%s:\s+(\d+)" % k, blk, re.M).group(1)) for k in META_KEYS}
    return out


def disassemble_lines(elf_bytes):
    """isa_audit.disassemble plus, per kernel, the source line of every instruction (needs a -gline-tables-only code object)."""
    with tempfile.NamedTemporaryFile(suffix=".elf") as f:
        f.write(elf_bytes); f.flush()
        txt = subprocess.run([f"{isa_audit.LLVM}/llvm-objdump", "-d", "-l", "--mcpu=gfx950", f.name], capture_output=True, text=True, check=True).stdout
    lines, cur, here = {}, None, None
    for ln in txt.splitlines():
        m = isa_audit.FUNC_RE.match(ln)
        if m:
            cur = lines.setdefault(m.group(2), [])
            here = None
            continue
        m = SRC_LINE_RE.match(ln)
        if m:
            here = (os.path.basename(m.group(1)), int(m.group(2)))
            continue
        if cur is not None and isa_audit.LINE_RE.match(ln):
            cur.append(here)
    return isa_audit.disassemble(elf_bytes), lines


def spill_vgprs(ins):
    """VGPRs the kernel only ever writes with v_writelane_b32: SGPR spill space."""
    lane_written, written = set(), set()
    for _, mn, ops, _ in ins:
        first = ops.split(",")[0]
        regs = set()
        for m in VREG_RE.finditer(first):
            regs |= {int(m.group(1))} if m.group(1) else set(range(int(m.group(2)), int(m.group(3)) + 1))
        if mn == "v_writelane_b32":
            lane_written |= regs
        elif not mn.startswith(("v_readlane", "v_readfirstlane", "v_cmp", "global_store", "flat_store", "ds_write", "scratch_store", "buffer_store")):
            written |= regs
    return {"v%d" % r for r in lane_written - written}


def count(ins, idxs, spill):
    c = dict(instructions=0, valu=0, reload=0, spill_write=0, cross_lane=0, scratch_ld=0, scratch_st=0)
    for i in idxs:
        _, mn, ops, _ = ins[i]
        c["instructions"] += 1
        if mn.startswith("v_"):
            c["valu"] += 1
        o = [x.strip() for x in ops.split(",")]
        if mn == "v_readlane_b32":
            c["reload" if len(o) > 1 and o[1] in spill else "cross_lane"] += 1
        elif mn == "v_writelane_b32":
            c["spill_write" if o[0] in spill else "cross_lane"] += 1
        elif mn.startswith("scratch_load"):
            c["scratch_ld"] += 1
        elif mn.startswith("scratch_store"):
            c["scratch_st"] += 1
    return c


def phases_of_source(path):
    """[(line, name)] of the `// ---- <name> ----` markers of the kernels' source."""
    out = []
    for n, ln in enumerate(open(path), 1):
        m = PHASE_RE.match(ln)
        if m:
            out.append((n, m.group(1).strip()))
    return out


def audit_function(ins, src_lines=None, phases=None, src_name=None):
    """-> {"total": counts, "loops": [...]}: one entry per loop header (back edges to the same header merged), outermost first.  `depth` 0 is
    a loop that lies in no other — in the persistent kernels the per-job loop."""
    spill = spill_vgprs(ins)
    blocks, blk_of, succ, loops = isa_audit.natural_loops(ins)
    by_head = {}
    for h, u, body in loops:
        e = by_head.setdefault(h, [set(), set()])
        e[0] |= body; e[1].add(u)
    items = sorted(by_head.items(), key=lambda kv: -len(kv[1][0]))
    out = []
    for h, (body, latches) in items:
        inner = set()
        for h2, (b2, _) in items:
            if h2 != h and b2 < body:
                inner |= b2
        depth = sum(1 for h2, (b2, _) in items if h2 != h and body < b2)
        idx = lambda bs: [i for b in sorted(bs) for i in range(*blocks[b])]
        ent = {"header": ins[blocks[h][0]][0], "depth": depth, "all": count(ins, idx(body), spill), "own": count(ins, idx(body - inner), spill)}
        if src_lines is not None:
            own = [src_lines[i] for i in idx(body - inner) if src_lines[i] and src_lines[i][0] == src_name]
            at = [src_lines[blocks[u][1] - 1] for u in latches]
            at = [a for a in at if a and a[0] == src_name] or own
            if at:
                line = min(a[1] for a in at)
                ph = [name for n, name in phases if n <= line]
                ent["phase"] = "per-job loop" if depth == 0 and len(body) > len(blocks) // 2 else ph[-1] if ph else "prologue"
                ent["lines"] = [min(a[1] for a in own), max(a[1] for a in own)] if own else [line, line]
        out.append(ent)
    out.sort(key=lambda e: e["header"])
    return {"total": count(ins, range(len(ins)), spill), "spill_vgprs": sorted(spill), "loops": out}


def audit_objects(objs, with_lines=False, only=("l1_deflate_kernel", "l1_encode_kernel")):
    """{demangled kernel: {"meta": ..., "total": ..., "loops": [...]}} over the code objects given as ELF images."""
    rep, names = {}, []
    phases = phases_of_source(SRC) if with_lines else None
    for co in objs:
        md = metadata(co)
        funcs, lines = disassemble_lines(co) if with_lines else (isa_audit.disassemble(co), {})
        for fn, ins in funcs.items():
            if not ins or fn not in md or not any(o in fn for o in only):
                continue
            rep[fn] = dict(audit_function(ins, lines.get(fn), phases, os.path.basename(SRC)), meta=md[fn])
            names.append(fn)
    dm = isa_audit.demangle(names) if names else {}
    return {dm[k].replace("dfl::", ""): v for k, v in rep.items()}


def audit(lib_path=LIB):
    return audit_objects(isa_audit.code_objects(lib_path))


def audit_source(flags=()):
    """Audit of a diagnostic device-only build of l1_deflate.hip with line tables: the same code as the product build, loops named by phase."""
    with tempfile.TemporaryDirectory() as td:
        co = os.path.join(td, "dfl.co")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output",
                        "-gline-tables-only", "-c", "-o", co, SRC] + list(flags), check=True, stderr=subprocess.DEVNULL, cwd=os.path.dirname(SRC))
        return audit_objects([open(co, "rb").read()], with_lines=True)


def two_per_cu(kernel):
    """Is this an l1_deflate_kernel instantiation of the classes S .. SG2 (1024 threads, two workgroups per CU, 64 VGPRs at most)?"""
    m = re.match(r"l1_deflate_kernel<(\d+), (\d+), (\d+), (true|false)", kernel)
    if not m:
        return False
    caps = [int(x) for x in re.findall(r"#define HMSE_TCAP_SG2 (\d+)", open(SRC).read())]
    return m.group(4) == "true" and int(m.group(1)) == 1024 and int(m.group(2)) <= caps[0]


def render(rep):
    out = []
    for k in sorted(rep):
        v = rep[k]; m = v["meta"]; t = v["total"]
        out.append("%s\n   vgpr %d  sgpr %d  sgpr spills %d  vgpr spills %d  scratch %d B  lds %d B  spill vgprs: %s" % (
            k, m["vgpr_count"], m["sgpr_count"], m["sgpr_spill_count"], m["vgpr_spill_count"], m["private_segment_fixed_size"],
            m["group_segment_fixed_size"], " ".join(v["spill_vgprs"]) or "-"))
        out.append("   %-64s %6s %6s %7s %7s %6s %8s   (own: valu reload write)" % ("loop", "instr", "valu", "reload", "sp.wr", "xlane", "scr l/s"))
        row = lambda name, c, o: "   %-64s %6d %6d %7d %7d %6d %4d/%-3d" % (name[:64], c["instructions"], c["valu"], c["reload"], c["spill_write"], c["cross_lane"], c["scratch_ld"], c["scratch_st"]) + (
            "   %5d %4d %3d" % (o["valu"], o["reload"], o["spill_write"]) if o else "")
        out.append(row("whole kernel", t, None))
        for l in v["loops"]:
            name = "%s%#x" % ("  " * l["depth"], l["header"])
            if "phase" in l:
                name += " %s [%d-%d]" % (l["phase"], l["lines"][0], l["lines"][1])
            out.append(row(name, l["all"], l["own"]))
        out.append("")
    return "\n".join(out)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--source" in args:
        print(render(audit_source([a for a in args if a.startswith("-D")])))
    else:
        print(render(audit(args[0] if args else LIB)))
