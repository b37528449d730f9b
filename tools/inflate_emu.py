"""The two decoders of hmse_l1_inflate (hmse_amd/csrc/l1_inflate.hip) on the CPU against zlib: no GPU needed.
    python tools/inflate_emu.py [--sanitize]
Cuts ifl::l1_inflate_kernel (one stream per wavefront) and ifl::l1_inflate_lanes_kernel (one stream per lane) out of l1_inflate.hip —
everything between the geometry constant and the assemble kernel; the bit reader, the code tables, the symbol decode and the walk over a
stream (ifl::walk_stream, which the first shares with gz::measure_kernel; its storing sink is in the cut)
come with hmse_amd/csrc/inflate_core.h as they are — compiles them with tools/inflate_emu.cpp (g++ -std=c++20: one std::thread per lane,
a barrier per wavefront under __ballot, readlane and readfirstlane) and runs both over the catalogue of tests/deflate_vectors.py: streams
zlib's decoder accepts and its encoder never writes, and the rejections beside them (those that would decode to some bytes once more, told that length), with zlib's decision and bytes as
the answer.  Left
out as too slow for a thread per lane: the 65 535-byte stored block and the 300-block stream (deflate_vectors.SLOW).  What g++ does not
take is replaced in the cut, the kernels stay as they are: the s_waitcnt asm becomes a meeting of the wavefront, the register-pinning asm
a fence, the ext_vector_type typedef a struct of four words; the scoped atomics and s_sleep have stand-ins in tools/hip_on_cpu.h.
--sanitize builds that program with -fsanitize=address,undefined (host code only).  Exit status 0 = all equal."""
import os
import re
import struct
import sys

from emu_common import ROOT, run

sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_vectors as dv  # noqa: E402


def for_gxx(td):
    path = os.path.join(td, "l1_inflate_kernels.inc")
    src = open(path).read()
    # s_waitcnt vmcnt(0): "the wavefront's own stores have landed".  Lanes in lockstep have all issued theirs by then; free-running
    # threads have not, so the wait becomes a meeting of the wavefront (it stands in wave-uniform code only).
    src, n_wait = re.subn(r'asm volatile\("s_waitcnt vmcnt\(0\)" ::: "memory"\);', "__builtin_amdgcn_wave_barrier();", src)
    src, n_asm = re.subn(r'asm volatile\("" : [^;]*\);', "__atomic_thread_fence(__ATOMIC_SEQ_CST);", src)
    src, n_vec = re.subn(r"typedef uint32_t u32x4 __attribute__\(\(ext_vector_type\(4\)\)\);", "struct u32x4 { uint32_t x, y, z, w; };", src)
    assert (n_wait, n_asm, n_vec) == (3, 1, 1), (n_wait, n_asm, n_vec)
    open(path, "w").write(src)


def records(td):
    for_gxx(td)
    keep = [(e, r) for e, r in zip(dv.catalogue(), dv.catalogue_raws()) if e[0] not in dv.SLOW]
    recs, first = dv.records([e for e, _ in keep], [r for _, r in keep], dv.WOULD_DECODE)
    raws = [dv.verdict(s) for s, _, _ in recs[:first]] + [r for _, r in keep]
    raws += [None] * (len(recs) - len(raws))                                           # refused as well when told the length they would decode to
    path = os.path.join(td, "inflate_records.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)))
        for (s, raw_len, base), raw in zip(recs, raws):
            assert raw is None or raw_len == len(raw)
            f.write(struct.pack("<I", len(s)) + s + struct.pack("<IiB", raw_len, base, raw is not None) + (raw or bytes(raw_len)))
    return [path]


if __name__ == "__main__":
    sys.exit(run(__doc__, "inflate", "constexpr int NT = 256;", "// chunk i of the original data", 1, extra=records, hip="l1_inflate"))
