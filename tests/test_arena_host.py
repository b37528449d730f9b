"""CPU: the test allocator of tests/test_gpu_arguments_only.py (tests/arena.py) checked on CPU tensors — placement, the three patterns,
the guard-band check — and, with the library's device entry points replaced by recorders, that hmse_amd.ops takes EVERY buffer it hands
to the library from ops._ws / ops._buf (so Arena.install sees them all), and that every entry point refuses a workspace off its 256-byte
alignment before it does anything else."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import arena as A

CPU = torch.device("cpu")


# ---- the arena itself ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", A.PATTERNS)
def test_place_delivers_the_misalignment_and_the_bytes(pattern):
    ar = A.Arena(CPU, pattern, seed=3)
    src = np.arange(1000, dtype=np.uint8)
    for m in range(16):
        t = ar.place(src, misalign=m)
        assert t.data_ptr() % 16 == m and t.data_ptr() % A.ALIGN == m
        assert t.is_contiguous() and t.dtype == torch.uint8 and np.array_equal(t.numpy(), src)
    d2 = ar.place(np.arange(64, dtype=np.uint8).reshape(2, 32), misalign=5)      # digest rows: a 2-D byte argument
    assert d2.shape == (2, 32) and d2.data_ptr() % 16 == 5 and d2.is_contiguous()
    typed = ar.place(np.arange(10, dtype=np.int64))
    assert typed.dtype == torch.int64 and typed.data_ptr() % A.ALIGN == 0 and typed.tolist() == list(range(10))
    with pytest.raises(ValueError):
        ar.place(np.arange(10, dtype=np.int64), misalign=4)                       # typed pointers keep their natural alignment
    a, both = ar.place_with_tail(src, np.full(300, 7, np.uint8), misalign=3)
    assert a.numel() == 1000 and both.numel() == 1300 and a.data_ptr() == both.data_ptr() and a.data_ptr() % 16 == 3
    assert np.array_equal(both.numpy()[1000:], np.full(300, 7, np.uint8))
    ar.check()


def test_empty_is_256_aligned_and_holds_the_pattern():
    seen = {}
    for pattern in A.PATTERNS:
        ar = A.Arena(CPU, pattern, seed=1)
        for shape, dt in ((5000, torch.uint8), ((7, 3), torch.int32), (0, torch.int64), ((0, 32), torch.uint8), (1, torch.int64)):
            t = ar.empty(shape, dt)
            assert t.data_ptr() % A.ALIGN == 0 and t.dtype == dt and t.is_contiguous()
            assert tuple(t.shape) == (shape if isinstance(shape, tuple) else (shape,))
        seen[pattern] = ar.empty(4096, torch.uint8).numpy().copy()
        ar.check()
    assert (seen["zero"] == 0).all() and (seen["ones"] == 0xFF).all()
    assert len(np.unique(seen["random"])) > 200                                  # a byte stream, not a constant
    assert np.array_equal(A.Arena(CPU, "random", seed=1).empty(4096).numpy(), A.Arena(CPU, "random", seed=1).empty(4096).numpy())   # seeded
    assert not np.array_equal(A.Arena(CPU, "random", seed=1).empty(4096).numpy(), A.Arena(CPU, "random", seed=2).empty(4096).numpy())
    with pytest.raises(ValueError):
        A.Arena(CPU, "stale")


def test_guard_bands_are_at_least_4096_bytes_of_pattern():
    ar = A.Arena(CPU, "ones")
    ar.place(np.zeros(100, np.uint8), misalign=13, name="x")
    b = ar.buffers[0]
    assert b["lo"] >= 4096 and b["raw"].numel() - b["lo"] - b["nbytes"] >= 4096
    assert (b["raw"][: b["lo"]] == 0xFF).all() and (b["raw"][b["lo"] + 100:] == 0xFF).all() and (b["raw"][b["lo"]: b["lo"] + 100] == 0).all()


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("where", ["-1", "-4096", "size", "size+4095"])
def test_check_names_the_buffer_and_the_first_changed_offset(pattern, where):
    ar = A.Arena(CPU, pattern, seed=9)
    ar.empty(100, torch.int32, name="innocent")
    t = ar.place(np.zeros(777, np.uint8), misalign=2, name="victim")
    ar.empty(50, torch.uint8, name="bystander")
    ar.check()
    t.fill_(0x5A)                                                                 # writing the buffer itself is no offence
    ar.check()
    off = {"-1": -1, "-4096": -4096, "size": 777, "size+4095": 777 + 4095}[where]
    b = ar.buffers[1]
    raw = b["raw"]
    raw[b["lo"] + off] ^= 0x01                                                    # a planted one-byte write in a guard band
    with pytest.raises(AssertionError) as ei:
        ar.check()
    msg = str(ei.value)
    assert "'victim'" in msg and f"offset {off} " in msg and ("in front of" if off < 0 else "behind") in msg
    raw[b["lo"] + off] ^= 0x01
    ar.check()


# ---- hmse_amd.ops allocates through _ws / _buf only -----------------------------------------------------------------------------------
DEVICE_CALLS = ("hmse_l2_cdc", "hmse_l3_sha256", "hmse_l3_dedup", "hmse_l3_index_update", "hmse_l4_lsh_update", "hmse_l4_minhash", "hmse_l4_lsh",
                "hmse_l1_deflate", "hmse_l1_deflate_ex", "hmse_l1_inflate", "hmse_read_assemble", "hmse_manifest_pack", "hmse_manifest_pack_ex",
                "hmse_gc_plan", "hmse_record_gather", "hmse_band_tables_write", "hmse_l4_index_build", "hmse_l4_query", "hmse_scrub_records",
                "hmse_scrub_attribute", "hmse_stream_workspace_init", "hmse_stream_batch", "hmse_stream_piece_hash", "hmse_stream_piece_encode",
                "hmse_stream_piece_sign", "hmse_stream_piece_bases", "hmse_stream_piece_encode_g")


@pytest.fixture()
def recorded(monkeypatch):
    """The library with its device entry points replaced by recorders (tests/arena.py: RecordingLib), and `torch` as hmse_amd.ops sees it
    without its uninitialised and zeroed allocators."""
    lib = A.record(monkeypatch, DEVICE_CALLS, banned=("empty", "zeros", "empty_like", "empty_strided"))
    ar = A.Arena(CPU, "random", seed=5)
    ar.install(monkeypatch)
    return ar, lib


def _wrapper_calls(ar):
    """name -> (callable, least number of buffers the wrapper creates itself (outputs, status words, workspace), number of pointers to inputs
    the wrapper COMPUTES (segment offsets, ids of a piece, a default base): values, not allocations)."""
    from hmse_amd import IngestConfig, ops
    cfg = IngestConfig()
    p = ar.place
    i64 = lambda *v: p(np.array(v, np.int64))
    data = p(np.arange(20000, dtype=np.uint8) // 3, misalign=3)
    cuts = i64(0, 5000, 12000, 20000)
    dg = p(np.arange(96, dtype=np.uint8).reshape(3, 32), misalign=1)
    sig = p(np.arange(3 * 128, dtype=np.int32).reshape(3, 128))
    keys = p(np.arange(12, dtype=np.int32).reshape(3, 4))
    t_i32 = lambda n: ar.empty(n, torch.int32)
    t_i64 = lambda n: ar.empty(n, torch.int64)
    res = SimpleNamespace(cuts=cuts, uniq_ids=i64(0, 1, 2), streams=data, stream_off=i64(0, 10, 20, 30), kind=p(np.zeros(3, np.uint8)), base=None,
                          base_global=None, digests=dg, refcount=t_i32(3), first_occ=i64(0, 1, 2), chunk_base=0)
    u8 = lambda n: ar.empty(n, torch.uint8)
    return {
        "l2_cdc": (lambda: ops.l2_cdc(data, cfg), 3, 1),
        "l2_cdc seg_off": (lambda: ops.l2_cdc(data, cfg, i64(0, 9000, 20000)), 3),
        "l3_sha256": (lambda: ops.l3_sha256(data, cuts), 2),
        "l3_dedup": (lambda: ops.l3_dedup(dg), 3),
        "l4_minhash": (lambda: ops.l4_minhash(data, cuts, cfg), 2),
        "l4_minhash no memo": (lambda: ops.l4_minhash(data, cuts, cfg, i64(2, 0), memo=False), 2),
        "l4_lsh": (lambda: ops.l4_lsh(sig, cfg), 3),
        "l1_deflate": (lambda: ops.l1_deflate(data, cuts, cfg, None, i64(-1, 0, -1), ws_limit=1 << 30), 5),
        "l1_deflate pieces": (lambda: ops.l1_deflate(data, cuts, cfg, None, None, ws_limit=40000), 4 + 3 + 1, 3),
        "l1_inflate": (lambda: ops.l1_inflate(data, i64(0, 10, 20, 30), p(np.zeros(3, np.uint8)), None, i64(5, 6, 7), check=False), 5),
        "l1_inflate empty chunks": (lambda: ops.l1_inflate(data, i64(0, 2), p(np.zeros(1, np.uint8)), None, i64(0), check=False), 6),
        "read_assemble": (lambda: ops.read_assemble(cuts, i64(0, 1, 2), cuts, data), 2),
        "manifest_pack": (lambda: ops.manifest_pack(res, 0, 1, None, i64(0, 10, 20, 30), 1, i64(0, 0, 0), u8(30), u8(3 * 40), u8(3 * 8), u8(0).reshape(0, 8)), 2, 1),
        "gc_plan": (lambda: ops.gc_plan(cuts, t_i32(3), 3, i64(0, 20000), p(np.zeros(1, np.uint8)), dg), 10),
        "record_gather": (lambda: ops.record_gather(data, None, i64(0, 100), p(np.zeros(2, np.uint8)), i64(0, 50, 90)), 2),
        "band_tables_write": (lambda: ops.band_tables_write(keys, sig, 16), 3),
        "l4_index_build": (lambda: ops.l4_index_build(keys), 4),
        "l4_query": (lambda: ops.l4_query(sig, keys, sig, ar.empty((4, 3), torch.int32), ar.empty((4, 3), torch.int32), cfg), 6),
        "scrub_records": (lambda: ops.scrub_records(data, t_i32(2), i64(0, 20000), i64(0, 2), t_i32(1), t_i32(2), t_i32(2), u8(2), t_i64(2), t_i32(2),
                                                    t_i32(2), 2, u8(2)), 3),
        "scrub_attribute": (lambda: ops.scrub_attribute(u8(2), t_i64(2), u8(2), ar.empty((2, 32)), ar.empty((2, 32)), True, t_i64(3), cuts, 16), 9),
        "stream_workspace": (lambda: ops.stream_workspace(1 << 20, cfg, CPU), 1),
    }


def test_every_pointer_ops_hands_to_the_library_comes_from_the_arena(recorded):
    """Inputs are placed through the arena by the test, everything else by ops._ws / ops._buf: a pointer outside the arena is a buffer that
    a wrapper allocated past the two helpers (a bare torch.empty added later), which Arena.install could not poison or guard."""
    ar, lib = recorded
    calls = _wrapper_calls(ar)
    assert len(calls) >= 20
    for name, (fn, least, *computed) in calls.items():
        n_buf, n_req, n_call = len(ar.buffers), len(ar.requests), len(lib.calls)
        fn()
        made = lib.calls[n_call:]
        assert made, name
        ptrs = [p for _, ps, _ in made for p in ps]
        outside = {p for p in ptrs if not ar.contains(p)}
        assert ptrs and len(outside) <= (computed[0] if computed else 0), (name, [hex(p) for p in outside])
        # at least as many requests as the wrapper has outputs, status words and workspaces of its own
        requested = len(ar.requests) - n_req
        assert requested >= least, (name, requested, least)
        assert all((b["raw"].data_ptr() + b["lo"]) % A.ALIGN == 0 for b in ar.buffers[n_buf:] if b["name"].startswith(("workspace", "ops buffer")))
    ar.check()


def test_install_poisons_what_the_wrapper_asks_to_be_zero_only_when_told_to(monkeypatch):
    from hmse_amd import ops
    ar = A.Arena(CPU, "ones").install(monkeypatch)
    assert ops._buf(8, torch.int64, CPU, fill=0).tolist() == [0] * 8 and ops._buf((2, 2), torch.int32, CPU, fill=-1).tolist() == [[-1, -1], [-1, -1]]
    assert ops._buf(4, torch.uint8, CPU).tolist() == [255] * 4 and ops._ws(10, CPU).numel() == 256 and ops._ws(10, CPU).data_ptr() % 256 == 0
    ar2 = A.Arena(CPU, "ones").install(monkeypatch, distrust_zeros=True)
    assert ops._buf(8, torch.int64, CPU, fill=0).tolist() == [-1] * 8 and ops._buf(3, torch.uint8, CPU, fill=0).tolist() == [255] * 3
    # reuse_ws: the second, smaller request gets the first one's memory as it was left
    ar3 = A.Arena(CPU, "zero").install(monkeypatch, reuse_ws=True)
    w1 = ops._ws(1000, CPU)
    w1.fill_(9)
    w2 = ops._ws(600, CPU)
    assert w2.data_ptr() == w1.data_ptr() and w2.numel() == 600 and (w2 == 9).all()
    w3 = ops._ws(5000, CPU)
    assert w3.data_ptr() != w1.data_ptr() and (w3 == 0).all()
    assert [k for k, _ in ar3.requests] == ["ws", "ws-reused", "ws"]
    for a in (ar, ar2, ar3):
        a.check()


def test_the_plain_helpers_are_what_they_replaced():
    from hmse_amd import ops
    assert ops._buf(5, torch.int64, CPU, fill=0).tolist() == [0] * 5 and ops._buf((2, 3), torch.int32, CPU, fill=-1).tolist() == [[-1] * 3] * 2
    e = ops._buf((3, 32), torch.uint8, CPU)
    assert e.shape == (3, 32) and e.dtype == torch.uint8
    assert ops._ws(1, CPU).numel() == 256 and ops._ws(1000, CPU).numel() == 1000


# ---- a workspace off its alignment is refused before anything else happens ---------------------------------------------------------------
def test_every_entry_point_refuses_a_misaligned_workspace_first():
    """HMSE_EINVAL from every entry point that takes a workspace, with no GPU in the machine: the check is the first statement, in front of
    every HIP call (include/hmse.h: "a workspace is 256-byte aligned").
    What this cannot show: the other arguments are dummies (every integer 1, every pointer one host address) and there is no aligned
    control call — that one would launch — so an entry point whose own validation refuses the dummies returns the same -1 without its
    alignment check.  What it does show is that no entry point gets as far as a HIP call (that returns HMSE_EHIP here) and that none is
    missing from the list.  The aligned call going through and the refused one leaving its outputs alone are checked on the GPU, for six
    wrappers (tests/test_gpu_arguments_only.py)."""
    from hmse_amd import IngestConfig, _lib
    real = _lib.hip_lib()
    cfg = IngestConfig().to_c()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hmse.h")) as f:
        header = f.read()
    mem = torch.zeros(1 << 16, dtype=torch.uint8)
    base = mem.data_ptr() + (-mem.data_ptr()) % 256
    seen = []
    for name in DEVICE_CALLS:
        fn = getattr(real, name)
        at = fn.argtypes
        proto = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M).group(1).split(",")      # the prototype in include/hmse.h names the arguments
        assert len(proto) == len(at), name
        ws_i = [i for i, arg in enumerate(proto) if arg.split()[-1] == "ws"]
        if not ws_i:
            assert name in ("hmse_l3_index_update", "hmse_l4_lsh_update", "hmse_read_assemble", "hmse_record_gather", "hmse_scrub_records"), name
            continue
        assert len(ws_i) == 1
        for off in (1, 4, 16, 128, 255):
            args = []
            for i, t in enumerate(at):
                if i == ws_i[0]:
                    args.append(base + 4096 + off)
                elif t is C.c_void_p:
                    args.append(base if i < len(at) - 1 else None)
                elif isinstance(t, type) and issubclass(t, C._Pointer):
                    args.append(C.byref(cfg) if t._type_ is _lib.HmseCfg else None)
                else:
                    args.append(1)
            assert fn(*args) == -1, (name, off)
        seen.append(name)
    assert len(seen) == 22, seen
