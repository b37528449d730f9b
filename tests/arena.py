"""A test allocator: the test decides what a call finds in its memory, where its byte pointers point and what lies around them.

Every buffer is carved out of the middle of a larger one that is filled with the arena's pattern: at least GUARD bytes of pattern lie in
front of it and behind it, and check() proves that a call left them alone.  Works on any torch device (tests/test_arena_host.py runs it
on the CPU; tests/test_gpu_arguments_only.py on the GPU).

  Arena(device, pattern, seed)     pattern: "zero" (0x00), "ones" (0xFF), "random" (a seeded byte stream; the one that catches "the stale
                                   value happened to be valid")
  place(array, misalign=0)         a copy of a numpy array / tensor; data_ptr() % 256 == misalign (uint8 only when misalign != 0)
  empty(shape, dtype)              the same placement, 256-byte aligned (uint8: misalign= as in place), contents = the pattern
  check()                          every guard band still holds its pattern, else AssertionError naming the buffer and the first changed offset
  install(monkeypatch, ...)        hmse_amd.ops allocates its outputs, status words and workspaces here
  record(monkeypatch, faked)       hmse_amd.ops runs without a GPU: the entry points `faked` record their arguments (RecordingLib)
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

GUARD = 4096
ALIGN = 256           # what the workspace carver of the library assumes (hmse_amd/csrc/common.h: WsCarver)
PATTERNS = ("zero", "ones", "random")


class Arena:
    def __init__(self, device, pattern: str = "random", seed: int = 0):
        if pattern not in PATTERNS:
            raise ValueError(f"pattern must be one of {PATTERNS}")
        self.device = torch.device(device)
        self.pattern = pattern
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))
        self.buffers = []          # dicts: name, raw, lo (offset of the view in raw), nbytes, before / after (copies of the guard bands)
        self.requests = []         # (kind, bytes) per buffer handed out through install(): kind in "ws", "buf", "ws-reused"
        self._ws_cache = None

    # ---- the pattern ------------------------------------------------------------------------------------------------------------
    def _filled(self, nbytes: int) -> torch.Tensor:
        if self.pattern == "random":
            return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=self.device, generator=self._gen)
        return torch.full((nbytes,), 0 if self.pattern == "zero" else 0xFF, dtype=torch.uint8, device=self.device)

    def _carve(self, nbytes: int, misalign: int, name: str | None) -> torch.Tensor:
        """uint8 view of `nbytes` bytes with data_ptr() % ALIGN == misalign, GUARD..GUARD + ALIGN + misalign pattern bytes in front of it and
        GUARD..GUARD + ALIGN behind it."""
        if not 0 <= misalign < 16:
            raise ValueError("misalign must lie in [0, 16)")
        raw = torch.empty(nbytes + 2 * GUARD + 2 * ALIGN, dtype=torch.uint8, device=self.device)
        lo = GUARD + (-(raw.data_ptr() + GUARD)) % ALIGN + misalign
        # (body first, then the bands from fixed-size draws: what a buffer holds depends on the seed and the order of requests, not on where
        # the allocator happened to put it)
        raw[lo: lo + nbytes] = self._filled(nbytes)
        raw[:lo] = self._filled(GUARD + 2 * ALIGN)[-lo:]
        raw[lo + nbytes:] = self._filled(GUARD + 2 * ALIGN)[: raw.numel() - lo - nbytes]
        view = raw[lo: lo + nbytes]
        assert view.data_ptr() % ALIGN == misalign and lo >= GUARD and raw.numel() - (lo + nbytes) >= GUARD
        self.buffers.append({"name": name or f"buffer{len(self.buffers)}", "raw": raw, "lo": lo, "nbytes": nbytes,
                             "before": raw[:lo].clone(), "after": raw[lo + nbytes:].clone()})
        return view

    # ---- buffers ------------------------------------------------------------------------------------------------------------------
    def empty(self, shape, dtype=torch.uint8, name: str | None = None, misalign: int = 0) -> torch.Tensor:
        shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (int(shape),)
        if misalign and dtype != torch.uint8:
            raise ValueError("only uint8 arguments may be misaligned: typed pointers need their natural alignment")
        item = torch.empty(0, dtype=dtype).element_size()
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        return self._carve(n * item, misalign, name).view(dtype).reshape(shape)

    def place(self, array, misalign: int = 0, name: str | None = None) -> torch.Tensor:
        t = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        t = t.contiguous()
        if misalign and t.dtype != torch.uint8:
            raise ValueError("only uint8 arguments may be misaligned: typed pointers need their natural alignment")
        view = self._carve(t.numel() * t.element_size(), misalign, name)
        out = view.view(t.dtype).reshape(t.shape)
        out.copy_(t)
        assert out.is_contiguous()
        return out

    def place_with_tail(self, array, tail, misalign: int = 0, name: str | None = None):
        """`array` (uint8) followed directly by the bytes `tail`, then the guard band: -> (view of array alone, view of both).  For a call
        whose declared size ends inside the buffer it was given: what lies behind the declared end is the test's choice."""
        a = np.ascontiguousarray(array, dtype=np.uint8).reshape(-1)
        both = self.place(np.concatenate([a, np.ascontiguousarray(tail, dtype=np.uint8).reshape(-1)]), misalign, name)
        return both[: a.size], both

    # ---- the check ------------------------------------------------------------------------------------------------------------------
    def check(self) -> None:
        """Offsets in the message count from the buffer's first byte: negative in the band in front of it, >= its size behind it."""
        for b in self.buffers:
            raw, lo, nb = b["raw"], b["lo"], b["nbytes"]
            for side, now, was, origin in (("in front of", raw[:lo], b["before"], -lo), ("behind", raw[lo + nb:], b["after"], nb)):
                if not torch.equal(now, was):
                    first = int(torch.nonzero(now != was)[0].item())
                    raise AssertionError(f"arena: the guard band {side} '{b['name']}' ({nb} bytes) was written: first changed byte at offset "
                                         f"{origin + first} ({int(was[first])} -> {int(now[first])})")

    def contains(self, ptr: int) -> bool:
        """`ptr` points into (or one past the end of) a buffer of this arena."""
        return any(b["raw"].data_ptr() + b["lo"] <= ptr <= b["raw"].data_ptr() + b["lo"] + b["nbytes"] for b in self.buffers)

    # ---- hmse_amd.ops ---------------------------------------------------------------------------------------------------------------
    def install(self, monkeypatch, distrust_zeros: bool = False, reuse_ws: bool = False, byte_misalign: int = 0) -> "Arena":
        """Route ops._ws and ops._buf through the arena.  distrust_zeros: a buffer the wrapper asks to be filled (zeros, -1) comes back
        poisoned like the others — include/hmse.h asks no caller to clear anything.  reuse_ws: a later call gets the workspace of the
        earlier one, as it was left, whenever it is large enough.  byte_misalign: the uint8 outputs the wrapper allocates (streams, raw
        bytes, digests, kinds, flags: byte pointers of the C-ABI) start that many bytes off a 256-byte boundary; workspaces never do."""
        from hmse_amd import ops

        def ws(nbytes, device):
            assert torch.device(device) == self.device or torch.device(device).type == self.device.type
            nbytes = max(int(nbytes), 256)
            if reuse_ws and self._ws_cache is not None and self._ws_cache.numel() >= nbytes:
                self.requests.append(("ws-reused", nbytes))
                return self._ws_cache[:nbytes]
            out = self.empty(nbytes, torch.uint8, name=f"workspace{len(self.buffers)}")
            self._ws_cache = out
            self.requests.append(("ws", nbytes))
            return out

        def buf(shape, dtype, device, fill=None):
            out = self.empty(shape, dtype, name=f"ops buffer{len(self.buffers)} {tuple(shape) if isinstance(shape, (tuple, list)) else shape} {dtype}",
                             misalign=byte_misalign if dtype == torch.uint8 else 0)
            if fill is not None and not distrust_zeros:
                out.fill_(fill)
            self.requests.append(("buf", out.numel() * out.element_size()))
            return out

        monkeypatch.setattr(ops, "_ws", ws)
        monkeypatch.setattr(ops, "_buf", buf)
        return self


# ---- hmse_amd.ops without a GPU: the library's device entry points replaced by recorders ------------------------------------------------
class RecordingLib:
    """The real library with the entry points `faked` replaced by recorders of their arguments (they return HMSE_OK and touch nothing);
    every other function (sizes, bounds, error strings) stays real.  calls: (name, the device pointers that are not NULL, all arguments)."""

    def __init__(self, real, faked):
        self._real, self._faked, self.calls = real, tuple(faked), []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._faked:
            return fn

        def fake(*args):
            assert len(args) == len(fn.argtypes), name
            ptrs = [a for a, t in zip(args[:-1], fn.argtypes[:-1]) if t is C.c_void_p and a is not None]   # (the last argument is the stream)
            assert all(isinstance(p, int) for p in ptrs), (name, ptrs)
            ints = [a for a, t in zip(args, fn.argtypes) if t in (C.c_uint64, C.c_uint32)]
            assert all(isinstance(v, int) and v >= 0 for v in ints), (name, ints)
            self.calls.append((name, ptrs, args))
            return 0
        return fake


class NoBareAllocation:
    """`torch` as hmse_amd.ops sees it: an uninitialised or filled allocation past _ws / _buf is an error."""

    def __init__(self, banned):
        self._banned = tuple(banned)

    def __getattr__(self, name):
        if name in self._banned:
            raise AssertionError(f"hmse_amd.ops calls torch.{name} directly: device buffers come from ops._ws / ops._buf")
        return getattr(torch, name)


def record(monkeypatch, faked, banned=()) -> RecordingLib:
    """Let hmse_amd.ops run on CPU tensors: the entry points `faked` record their calls, the device check and the stream are stubbed, and
    (with `banned`) ops sees a torch without those allocators.  -> the recording library."""
    from hmse_amd import _lib, ops
    lib = RecordingLib(_lib.hip_lib(), faked)
    monkeypatch.setattr(_lib, "hip_lib", lambda: lib)
    monkeypatch.setattr(ops, "_require_gpu", lambda t, name: None)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    if banned:
        monkeypatch.setattr(ops, "torch", NoBareAllocation(banned))
    return lib
