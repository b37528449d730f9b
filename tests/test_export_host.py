"""CPU: the arithmetic of the export (tests/export_ref.py: the product and the powers of x modulo the CRC-32 polynomial, the combination,
the right-aligned 64-strip tree of the CRC kernel) against zlib, the entry points' own refusals (HMSE_EINVAL in front of every HIP call),
the symbols and prototypes, the wrappers' refusal of host tensors and their pointers, the member layout against Python's gzip, and the
kernels on the CPU (tools/export_emu.py)."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import export_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("hmse_crc32", "hmse_crc32_combine", "hmse_gzip_members")


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_the_register_is_zlib_s():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 1000):
        for data in (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), bytes(n), b"\xff" * n):
            assert ref.crc_from_reg(ref.reg(data), n) == zlib.crc32(data)
            assert ref.reg(data, 0xFFFFFFFF) ^ 0xFFFFFFFF == zlib.crc32(data)
            assert ref.reg(bytes(7) + data) == ref.reg(data)                           # leading zeros leave a register of 0 at 0
    assert ref.mulmod(ref.ONE, 0x12345678) == 0x12345678 and ref.xpow8(0) == ref.ONE and ref.xpow8(1) == ref.ONE >> 8
    assert ref.xpow8((1 << 32) - 1) == ref.ONE                                         # the order of x divides 2^32 - 1
    a, b, c = (int(v) for v in rng.integers(0, 1 << 32, 3))
    assert ref.mulmod(a, b) == ref.mulmod(b, a) and ref.mulmod(ref.mulmod(a, b), c) == ref.mulmod(a, ref.mulmod(b, c))
    assert ref.mulmod(a ^ b, c) == ref.mulmod(a, c) ^ ref.mulmod(b, c)
    assert ref.mulmod(ref.xpow8(1000), ref.xpow8(23456)) == ref.xpow8(24456)


def test_two_parts_and_random_splits_with_empty_parts():
    rng = np.random.default_rng(2)
    empties = 0
    for trial in range(60):
        n = int(rng.integers(0, 3000))
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        k = int(rng.integers(0, n + 1))
        A, B = data[:k], data[k:]
        assert zlib.crc32(A + B) == ref.mulmod(zlib.crc32(A), ref.xpow8(len(B))) ^ zlib.crc32(B)
        cuts = np.sort(rng.integers(0, n + 1, int(rng.integers(0, 12))))
        cuts = [0] + [int(c) for c in np.repeat(cuts, rng.integers(1, 3, cuts.size))] + [n]       # repeated cuts: empty parts
        parts = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        empties += sum(1 for p in parts if not p)
        assert ref.combine([zlib.crc32(p) for p in parts], [len(p) for p in parts]) == zlib.crc32(data)
    assert empties > 50
    assert ref.combine([], []) == 0 and ref.combine([0, 0], [0, 0]) == 0


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 63, 64, 65, 1000, 32768])
def test_the_right_aligned_strip_tree(n):
    """what hmse_crc32 computes per range: 64 strips, zeros in front, registers from 0, six levels, the init folded in at the end"""
    rng = np.random.default_rng(n)
    for data in (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), bytes(n), b"\xff" * n):
        assert ref.strip_tree(data) == zlib.crc32(data)
    if n:
        tiles, s, ss = ref.geometry(n)
        assert s % 16 == 0 and 16 <= s <= 128 and 64 * ss >= n and 64 * (ss - 16 * tiles) < n      # the smallest strip of whole pieces
    if n:                                                                              # and with the smallest strip of whole dwords
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert ref.strip_tree(data, strip=((n + 63) // 64 + 3) & ~3) == zlib.crc32(data)


def test_geometry_is_the_kernel_s():
    src = open(os.path.join(ROOT, "hmse_amd", "csrc", "export.hip")).read()
    smax = int(re.search(r"constexpr int EX_SMAX = (\d+);", src).group(1))
    assert smax == 128 and "constexpr int EX_TILE = 64 * EX_SMAX;" in src
    assert ref.geometry(8192) == (1, 128, 128) and ref.geometry(8193) == (2, 80, 160) and ref.geometry(1) == (1, 16, 16)


def test_members_are_gzip_and_bgzf():
    raw = b"hello, hello, hello\n" * 7
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    stream = co.compress(raw) + co.flush()
    for bgzf in (False, True):
        m = ref.member(stream, raw, bgzf)
        assert gzip.decompress(m) == raw and zlib.decompress(m, wbits=31) == raw
        assert gzip.decompress(m + ref.member(stream[:0] + b"\x03\x00", b"", bgzf) + m) == raw + raw      # an empty member between two
        assert ref.parse_members(m + m) == [(0, len(m)), (len(m), len(m))]
    z = ref.member(stream, raw, True)
    assert len(ref.BGZF_HEADER) == 16 and int.from_bytes(z[16:18], "little") == len(z) - 1
    assert len(ref.BGZF_EOF) == 28 and gzip.decompress(ref.BGZF_EOF) == b"" and gzip.decompress(z + ref.BGZF_EOF) == raw
    from hmse_amd import export
    assert export.BGZF_EOF == ref.BGZF_EOF and (export.GZIP_HEADER, export.BGZF_HEADER, export.TRAILER) == (10, 18, 8)


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_prototypes():
    from hmse_amd import _lib, ops
    lib = _lib.hip_lib()
    header = open(os.path.join(ROOT, "include", "hmse.h")).read()
    for name in CALLS:
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        proto = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M).group(1).split(",")
        assert fn.restype is C.c_int and len(proto) == len(fn.argtypes), name
        assert proto[-1].split()[-1] == "stream"
    assert [len(getattr(lib, n).argtypes) for n in CALLS] == [7, 6, 18]
    assert int(re.search(r"#define HMSE_GZIP_BGZF (\d+)u", header).group(1)) == ops.GZIP_BGZF == 1
    assert lib.hmse_abi_version() == 3
    stages = dict(re.findall(r"HMSE_STAGE_(EXPORT_\w+)\s*= (\d+)", header))
    assert (int(stages["EXPORT_CRC"]), int(stages["EXPORT_MEMBERS"])) == (ops.STAGE_EXPORT_CRC, ops.STAGE_EXPORT_MEMBERS) == (0, 1)


def test_entry_points_refuse_null_arrays_and_bad_flags_with_no_gpu_present():
    """HMSE_EINVAL (-1), never HMSE_EHIP (-3): refused in front of every clear and launch.  (The pointers are host addresses; nothing may
    touch them.)"""
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr()
    crc = lambda **kw: lib.hmse_crc32(*[{**dict(data=b, n=100, cuts=b, n_chunks=2, out=b, status=b), **kw}[k] for k in ("data", "n", "cuts", "n_chunks", "out", "status")], None)
    for kw in (dict(status=None), dict(cuts=None), dict(out=None), dict(data=None), dict(n_chunks=(1 << 40) + 1)):
        assert crc(**kw) == -1, kw
    comb = lambda **kw: lib.hmse_crc32_combine(*[{**dict(crc=b, len=b, n=3, out=b, status=b), **kw}[k] for k in ("crc", "len", "n", "out", "status")], None)
    for kw in (dict(status=None), dict(out=None), dict(crc=None), dict(len=None), dict(n=(1 << 32) + 1), dict(out=None, n=0)):
        assert comb(**kw) == -1, kw
    names = ("src0", "src0_bytes", "src1", "src1_bytes", "src_off", "stream_len", "src_sel", "crc", "raw_off", "n_rec", "slot", "n_chunks", "member_off",
             "flags", "dst", "dst_bytes", "status")
    dflt = dict(src0=b, src0_bytes=10, src1=b, src1_bytes=10, src_off=b, stream_len=b, src_sel=b, crc=b, raw_off=b, n_rec=1, slot=b, n_chunks=1,
                member_off=b, flags=0, dst=b, dst_bytes=100, status=b)
    mem_ = lambda **kw: lib.hmse_gzip_members(*[{**dflt, **kw}[k] for k in names], None)
    for kw in [dict(status=None), dict(flags=2), dict(flags=3), dict(flags=0x80000000), dict(src0=None), dict(src1=None), dict(n_chunks=1 << 33),
               dict(flags=2, n_chunks=0)] + [{k: None} for k in ("src_off", "stream_len", "src_sel", "crc", "raw_off", "slot", "member_off", "dst")]:
        assert mem_(**kw) == -1, kw
    assert mem.sum().item() == 0


def test_wrappers_refuse_host_tensors():
    from hmse_amd import export, ops
    data, cuts = torch.zeros(16, dtype=torch.uint8), torch.tensor([0, 16])
    i32, i64 = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.crc32(data, cuts)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.crc32_combine(i32, i64)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.gzip_members(data, None, i64, i64, torch.zeros(1, dtype=torch.uint8), i32, cuts, i64, torch.tensor([0, 20]))
    with pytest.raises(IndexError):
        export.read_member(export.GzipExport(data, torch.tensor([0, 5, 16]), cuts, 0, 1, 0), 2)
    assert export.read_member(export.GzipExport(data, torch.tensor([0, 5, 16]), cuts, 0, 1, 0), 1) == (5, 11)


def test_every_pointer_the_export_wrappers_hand_to_the_library_comes_from_the_arena(monkeypatch):
    """The three entry points replaced by recorders of their arguments (tests/arena.py: RecordingLib)."""
    import arena as A
    from hmse_amd import ops
    lib = A.record(monkeypatch, CALLS)
    ar = A.Arena(torch.device("cpu"), "zero", seed=5).install(monkeypatch)             # (zero: the recorders leave the status words as they are)
    p = ar.place
    i64 = lambda *v: p(np.array(v, np.int64))
    i32 = lambda *v: p(np.array(v, np.int32))
    data = p(np.arange(100, dtype=np.uint8), misalign=3)
    calls = {"crc32": lambda: ops.crc32(data, i64(0, 40, 100)),
             "crc32_combine": lambda: ops.crc32_combine(i32(1, 2), i64(40, 60)),
             "gzip_members": lambda: ops.gzip_members(data, None, i64(0, 40), i64(40, 60), p(np.zeros(2, np.uint8)), i32(1, 2), i64(0, 400, 1000), i64(1, 0, 1),
                                                      i64(0, 78, 136, 214), bgzf=True)}
    for name, fn in calls.items():
        n_call = len(lib.calls)
        fn()
        made = lib.calls[n_call:]
        assert len(made) == 1 and made[0][0] == "hmse_" + name, name
        ptrs = made[0][1]
        assert ptrs and all(ar.contains(q) for q in ptrs), (name, [hex(q) for q in ptrs if not ar.contains(q)])
    assert lib.calls[-1][2][13] == 1 and lib.calls[-1][2][15] == 214                    # flags = BGZF, dst_bytes = member_off[-1]
    assert not [k for k, _ in ar.requests if k != "buf"]                               # no workspace anywhere
    ar.check()


def test_to_gzip_refuses_a_result_above_max_bytes_before_any_device_work(monkeypatch):
    """the copied streams alone already exceed max_bytes: ValueError with both numbers, nothing decoded, nothing allocated"""
    from hmse_amd import export, ops

    class Reader:
        def __init__(self, store, device):
            self.kind = np.array([0, 2, 0], np.uint8)
            self.stream_off, self.stream_len = np.array([0, 108, 200], np.int64), np.array([100, 50, 30], np.int64)
            self.slot = np.array([0, 1, 0, 2], np.int64)
    monkeypatch.setattr(export, "StoreReader", Reader)
    for name in ("crc32", "l1_deflate", "gzip_members", "_buf"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("device work"))
    with pytest.raises(ValueError, match=r"at least 302 bytes, max_bytes is 301"):     # 100 + 0 + 100 + 30 and 4 x 18
        export.to_gzip(None, torch.device("cpu"), max_bytes=301)
    with pytest.raises(ValueError, match=r"at least 362 bytes, max_bytes is 100"):     # BGZF: 4 x 26 and the EOF block
        export.to_gzip(None, torch.device("cpu"), bgzf=True, max_bytes=100)


# ---- the kernels on the CPU --------------------------------------------------------------------------------------------------------------
def test_the_emulator_builds_and_its_cases_pass():
    """tools/export_emu.py: the kernels cut out of export.hip, one std::thread per lane, against the bit-by-bit CRC-32 (itself held against
    zlib's answers first), an independent modular product and the member layout byte by byte (no sanitizer here)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "export_emu.py"), "--iters", "6", "--seed", "4242"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "known answers (zlib): 33, 0 wrong" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
