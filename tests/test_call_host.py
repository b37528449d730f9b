"""CPU: the one call path of hmse_amd.ops (ops._call over _lib.SIGNATURES), with the library's device entry points replaced by recorders
(tests/arena.py) — what it does with every kind of parameter, and that a tensor whose elements are not as wide as the header declares
is refused before the library is reached."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import arena as A

CPU = torch.device("cpu")


@pytest.fixture()
def recorded(monkeypatch):
    from hmse_amd import _lib
    lib = A.record(monkeypatch, [n for n, (_, params) in _lib.PARSED.items() if params and params[-1].kind == _lib.STREAM])
    return A.Arena(CPU, "random", seed=5).install(monkeypatch), lib


def _refused(lib, call, text):
    from hmse_amd import ops
    with pytest.raises(ops.HmseError, match=text) as ei:
        call()
    assert ei.value.code == -1 and lib.calls == []


def test_wrappers_refuse_a_tensor_of_another_element_width(recorded):
    """A kernel that reads 8 bytes per element never sees an int32 array (and the other way round): HmseError(-1) that names the
    parameter, and no call reaches the library."""
    from hmse_amd import ops
    ar, lib = recorded
    p = ar.place
    i64, i32 = (lambda *v: p(np.array(v, np.int64))), (lambda *v: p(np.array(v, np.int32)))
    raw, pat = p(np.arange(100, dtype=np.uint8)), p(np.frombuffer(b"abcd", np.uint8).copy())
    _refused(lib, lambda: ops.find_scan(raw, i32(0, 40, 100), None, pat, [0, 4]), "hmse_find_scan: raw_off must have 8-byte elements")
    cuts, dg = i64(0, 5000, 12000, 20000), p(np.zeros((3, 32), np.uint8))
    _refused(lib, lambda: ops.gc_plan(cuts, i64(0, 1, 2), 3, i64(0, 20000), p(np.zeros(1, np.uint8)), dg), "hmse_gc_plan: slot must have 4-byte elements")
    data = p(np.zeros(20000, np.uint8))
    _refused(lib, lambda: ops.l3_sha256(data, i32(0, 5000, 12000, 20000)), "hmse_l3_sha256: cuts must have 8-byte elements")
    ops.find_scan(raw, i64(0, 40, 100), i32(2, 1), pat, [0, 4], hits_cap=0)              # the declared widths go through
    ops.gc_plan(cuts, i32(0, 1, 2), 3, i64(0, 20000), p(np.zeros(1, np.uint8)), dg)
    ops.l3_sha256(data, cuts)
    assert [c[0] for c in lib.calls] == ["hmse_find_scan", "hmse_gc_plan", "hmse_l3_sha256"]


def test_call_handles_every_kind_of_parameter(recorded, monkeypatch):
    from hmse_amd import IngestConfig, _lib, ops
    ar, lib = recorded
    monkeypatch.setattr(ops, "_stream", lambda: 77)
    p = ar.place
    raw, off, mult = p(np.arange(100, dtype=np.uint8)), p(np.array([0, 40, 100], np.int64)), p(np.array([2, 1], np.int32))
    pat, hits, counts = p(np.frombuffer(b"abcd", np.uint8).copy()), ar.empty(4, torch.int64), ar.empty(1, torch.int64)
    bounds, ks, meta = (C.c_uint32 * 2)(0, 4), (C.c_uint8 * 1)(1), ar.empty(2, torch.int64)

    def approx_scan(**changed):
        given = dict(raw=raw, raw_bytes=100, raw_off=off, n_rec=2, mult=mult, pat=pat, pat_off=bounds, k=ks, n_pat=1, flags=True, hits=hits,
                     hits_cap=4, n_hits=meta.data_ptr(), counts=counts, status=meta.data_ptr() + 8)
        assert list(given) == [q.name for q in _lib.PARSED["hmse_approx_scan"][1][:-1]]
        ops._call("hmse_approx_scan", *{**given, **changed}.values())
        return lib.calls.pop()[2]

    # a device pointer: a tensor's address, None as NULL, an int as a raw address; a host array as it is; a scalar as an int; the stream last
    args = approx_scan()
    assert args == (raw.data_ptr(), 100, off.data_ptr(), 2, mult.data_ptr(), pat.data_ptr(), bounds, ks, 1, 1, hits.data_ptr(), 4, meta.data_ptr(),
                    counts.data_ptr(), meta.data_ptr() + 8, 77)
    assert args[6] is bounds and args[7] is ks and type(args[9]) is int
    assert approx_scan(mult=None, hits=None)[4::6] == (None, None)
    # `?`: NULL for an empty tensor; elsewhere whatever torch gives as its address
    assert approx_scan(raw=raw[:0])[0] is None and approx_scan(pat=pat[:0])[5] == pat[:0].data_ptr()
    # the declared width, for every device pointer that has one
    for name, t, width in (("raw", off, 1), ("raw_off", mult, 8), ("mult", off, 4), ("pat", mult, 1), ("hits", mult, 8), ("counts", raw, 8)):
        _refused(lib, lambda: approx_scan(**{name: t}), f"hmse_approx_scan: {name} must have {width}-byte elements")
    with pytest.raises(TypeError, match="takes 15 arguments"):
        ops._call("hmse_approx_scan", raw, 100)

    # host structs by reference: an IngestConfig as its hmse_cfg, a StreamArrays as its hmse_stream, a mirror as it is; void*: any width
    cfg, s, gl4, ws = IngestConfig(min_size=2048), ops.StreamArrays(world=2, rank=1, cuts=off), _lib.HmseGl4(world=2), ar.empty(256, torch.uint8)
    ops._call("hmse_stream_piece_bases", 1 << 20, cfg, s, off, gl4, ws, ws.numel())
    args = lib.calls.pop()[2]
    assert (args[0], args[3], args[5], args[6], args[7]) == (1 << 20, off.data_ptr(), ws.data_ptr(), 256, 77)
    assert isinstance(args[1]._obj, _lib.HmseCfg) and args[1]._obj.min_size == 2048 and args[2]._obj is s.c and args[4]._obj is gl4
    copy = _lib.HmseStream.from_buffer_copy(s.c)            # (tests/test_gpu_stream_descriptor.py hands over edited copies like this one)
    ops._call("hmse_stream_piece_bases", 1 << 20, cfg, SimpleNamespace(c=copy), off, gl4, ws, ws.numel())
    assert lib.calls.pop()[2][2]._obj is copy
    hdr = ops.Regex(p(np.zeros(6, np.int16)), p(np.zeros(256, np.uint8)), 2, 3, 1).header()
    ops._call("hmse_regex_scan", raw, 100, off, 2, None, hdr, None, 0, meta.data_ptr(), counts, meta.data_ptr() + 8)
    assert lib.calls.pop()[2][5]._obj is hdr
    ar.check()


def test_call_raises_the_library_s_status_under_the_entry_point_s_name(monkeypatch):
    """The real library refuses a workspace off its alignment before any HIP call: _call turns the status into HmseError, and an _ex entry
    point reports under the name of the call it extends."""
    from hmse_amd import IngestConfig, ops
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    with pytest.raises(ops.HmseError, match=r"^hmse_l1_deflate: .*\(-1\)$") as ei:
        ops._call("hmse_l1_deflate_ex", None, 0, None, None, None, 0, IngestConfig(), 0, None, 0, None, None, None, 1, 4096)
    assert ei.value.code == -1
    with pytest.raises(ops.HmseError, match=r"^hmse_l3_sha256: "):
        ops._call("hmse_l3_sha256", None, 0, None, 0, None, 1, 4096)
