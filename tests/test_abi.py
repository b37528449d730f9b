"""CPU: the C-ABI library loads and exports every symbol include/hmse.h declares; host-side entry points
(config, sizing, Gear table, error strings) behave; the device ops refuse to run without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "hmse.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hmse_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    names = declared_functions()
    assert {"hmse_l2_cdc", "hmse_l3_sha256", "hmse_l3_dedup", "hmse_l4_minhash", "hmse_l4_lsh", "hmse_l1_deflate",
            "hmse_workspace_bytes", "hmse_cfg_default", "hmse_cfg_validate"} <= set(names)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/hmse.h but not exported"
    assert set(_lib.EXPORTED_SYMBOLS) == set(names)
    assert lib.hmse_abi_version() == 3


def prototypes():
    """include/hmse.h -> {name: (return type, [(C type without const, is a pointer, parameter name)])}."""
    src = open(os.path.join(ROOT, "include", "hmse.h")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    out = {}
    for m in re.finditer(r"^([A-Za-z_][\w \*]*?[\s\*])(hmse_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", src, re.M):
        ret, name, params = (" ".join(g.split()) for g in m.groups())
        assert name not in out, name
        decls = []
        for p in ([] if params == "void" else params.split(",")):
            ty, star, pname, array = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*(\[\d+\])?\s*", p).groups()
            decls.append((ty, bool(star or array), pname))           # (`uint64_t table[256]` is a pointer)
        out[name] = (ret, decls)
    return out


_C_ELEM = {"u8": "uint8_t", "u32": "uint32_t", "i32": "int32_t", "u64": "uint64_t", "i64": "int64_t", "f64": "double"}
_C_SCALAR = {"u32": "uint32_t", "u64": "uint64_t", "size_t": "size_t", "int": "int"}
_C_RETURN = {"int": "int", "void": "void", "u64": "uint64_t", "size_t": "size_t", "str": "const char*"}


def kind_agrees(kind: str, c_type: str, is_pointer: bool) -> bool:
    """A kind of _lib.SIGNATURES against the C declaration: pointer or not, the pointee's width and signedness, the scalar's type.  Opaque
    bytes (`void*`) may stand for a `void*` or a `uint8_t*`."""
    if kind == "stream":
        return is_pointer and c_type == "void"
    if kind in _C_SCALAR:
        return not is_pointer and c_type == _C_SCALAR[kind]
    if kind.endswith("[]"):
        return is_pointer and c_type == _C_ELEM.get(kind[:-2])
    base = kind.rstrip("?")
    if not is_pointer or not base.endswith("*"):
        return False
    base = base[:-1]
    if base == "void":
        return c_type in ("void", "uint8_t")
    return c_type == (base if base.startswith("hmse_") else _C_ELEM.get(base))


def test_the_signature_table_is_the_header():
    """Every prototype of include/hmse.h has its entry in _lib.SIGNATURES: the same parameters under the same names in the same order, each of a
    kind that agrees with its C type, the same return type — and the table names nothing else.  What ctypes is told follows from the table."""
    import ctypes as C
    from hmse_amd import _lib
    protos = prototypes()
    assert len(protos) == 64 and set(protos) == set(_lib.SIGNATURES) and _lib.EXPORTED_SYMBOLS == tuple(_lib.SIGNATURES)
    lib = _lib.hip_lib()
    for name, (ret, decls) in protos.items():
        t_ret, _, t_params = _lib.SIGNATURES[name].partition(":")
        assert _C_RETURN[t_ret] == ret, (name, t_ret, ret)
        entries = [p.split() for p in t_params.split(",") if p.strip()]
        entries = [e if len(e) == 2 else [e[0], e[0]] for e in entries]                   # ("stream" is its own name)
        assert [e[1] for e in entries] == [d[2] for d in decls], name
        for (kind, pname), (c_type, is_pointer, _) in zip(entries, decls):
            assert kind_agrees(kind, c_type, is_pointer), (name, pname, kind, c_type)
        assert "stream" not in [e[0] for e in entries[:-1]], name                          # the stream comes last
        fn, (restype, params) = getattr(lib, name), _lib.PARSED[name]
        assert fn.restype is restype and list(fn.argtypes) == [p.ctype for p in params] and (restype is None) == (ret == "void"), name
        for p, (kind, _), (c_type, _, _) in zip(params, entries, decls):
            assert p.kind == (_lib.STREAM if kind == "stream" else _lib.SCALAR if kind in _C_SCALAR else _lib.HOST if kind.endswith("[]") else
                              _lib.STRUCT if kind.startswith("hmse_") else _lib.DEVICE), (name, p)
            if p.kind == _lib.DEVICE:
                width = 0 if kind.startswith("void") else C.sizeof(getattr(C, "c_" + c_type[:-2]))     # uint64_t -> c_uint64
                assert p.ctype is C.c_void_p and p.width == width and p.null_if_empty == kind.endswith("?"), (name, p)
    assert [n for n, (r, _) in _lib.PARSED.items() if r is None] == ["hmse_cfg_default", "hmse_gear_table", "hmse_profile_enable"]


def test_the_table_check_sees_one_changed_width():
    """The comparison above fails for a table that is wrong in one width, one signedness, a scalar for a pointer or a host array's type."""
    assert kind_agrees("u64*", "uint64_t", True) and kind_agrees("u64*?", "uint64_t", True) and kind_agrees("void*", "uint8_t", True)
    assert kind_agrees("u32[]", "uint32_t", True) and kind_agrees("hmse_cfg*", "hmse_cfg", True) and kind_agrees("size_t", "size_t", False)
    for kind, c_type, is_pointer in (("u32*", "uint64_t", True), ("u64*", "uint32_t", True), ("u64*", "int64_t", True), ("u32", "uint64_t", False),
                                     ("u64", "size_t", False), ("u64", "uint64_t", True), ("u64*", "uint64_t", False), ("u8[]", "uint32_t", True),
                                     ("void*", "uint32_t", True), ("hmse_cfg*", "hmse_stream", True), ("stream", "uint8_t", True), ("int", "uint32_t", False)):
        assert not kind_agrees(kind, c_type, is_pointer), (kind, c_type)


def test_library_exports_nothing_but_the_declared_abi():
    """exported == declared: no diagnostic hook or probe entry point ships in the product library."""
    import subprocess
    from hmse_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[1:2] and ln.split()[1] in "TW"}
    c_abi = sorted(s for s in exported if not s.startswith("_"))
    undeclared = [s for s in c_abi if s not in set(declared_functions()) and not s.startswith("__hip")]
    assert undeclared == [], undeclared
    assert [s for s in c_abi if s.startswith("hmsedbg")] == []
    src = "".join(open(os.path.join(ROOT, "hmse_amd", "csrc", f)).read() for f in ("l4_minhash.hip", "l1_inflate.hip"))
    assert src.count("#ifdef HMSE_DIAG") >= 3 and "getenv" not in re.sub(r"#ifdef HMSE_DIAG.*?#e(lse|ndif)", "", src, flags=re.S)


def test_deflate_record_bytes_formula_matches_the_abi():
    """ops.record_bytes (evaluated on the device for a whole shard) == hmse_l1_deflate_record_bytes[_dict] for every chunk
    length; the FULL stream (copied out in whole 16-byte stores) fits the token area it overwrites, the DELTA slot behind
    the tokens is 16-byte aligned and leaves 16 bytes behind the largest stream."""
    import torch
    from hmse_amd import _lib, ops
    lib = _lib.hip_lib()
    lens = torch.arange(0, 32769, dtype=torch.int64)
    got = ops.record_bytes(lens).numpy()
    got_d = ops.record_bytes(lens, torch.ones_like(lens, dtype=torch.bool)).numpy()
    mixed = ops.record_bytes(lens, lens % 2 == 1).numpy()
    want = np.array([lib.hmse_l1_deflate_record_bytes(int(v)) for v in range(32769)], dtype=np.int64)
    want_d = np.array([lib.hmse_l1_deflate_record_bytes_dict(int(v)) for v in range(32769)], dtype=np.int64)
    assert np.array_equal(got, want) and np.array_equal(got_d, want_d)
    assert np.array_equal(mixed, np.where(np.arange(32769) % 2 == 1, want_d, want))
    L = lens.numpy()
    body = 1296 + 4 * ((L + 3) & ~3)
    assert (body % 16 == 0).all() and (want >= body).all() and (want % 256 == 0).all() and (want_d % 256 == 0).all()
    assert (((L[1:] + 5 + 15) & ~15) <= body[1:] - 1296).all()          # FULL stream over the tokens, 16-byte stores
    assert (want_d - body - (L + 5) >= 16).all()                        # DELTA slot
    assert lib.hmse_l1_deflate_record_bytes(32769) == 0 and lib.hmse_l1_deflate_record_bytes_dict(32769) == 0


def test_cfg_default_matches_oracle_and_dataclass(orc):
    from hmse_amd import IngestConfig, _lib
    lib = _lib.hip_lib()
    c = _lib.HmseCfg()
    lib.hmse_cfg_default(C.byref(c))
    o = orc.default_cfg()
    d = IngestConfig().to_c()
    assert C.sizeof(c) == 64 == c.struct_size
    for name, _ in _lib.HmseCfg._fields_:
        assert getattr(c, name) == getattr(o, name) == getattr(d, name), name
    assert lib.hmse_cfg_validate(C.byref(c)) == 0


@pytest.mark.parametrize("kw", [dict(min_size=32), dict(avg_size=6000), dict(max_size=65536), dict(n_hashes=64), dict(shingle=5),
                                dict(bands=5), dict(level=10), dict(seg_size=1024), dict(norm_level=9)])
def test_cfg_validate_rejects(kw):
    from hmse_amd import IngestConfig, _lib
    c = IngestConfig(**kw).to_c()
    assert _lib.hip_lib().hmse_cfg_validate(C.byref(c)) == -1  # HMSE_EINVAL, like miniz/mbedtls negative status codes


def test_reference_preset_and_ablations():
    from hmse_amd import ABLATIONS, IngestConfig, _lib
    p = IngestConfig.reference_preset()                      # README.md:2444-2446
    assert (p.min_size, p.avg_size, p.max_size) == (1024, 4096, 16384)
    assert _lib.hip_lib().hmse_cfg_validate(C.byref(p.to_c())) == 0
    assert set(ABLATIONS) == {"l1_only", "l1_cdc", "l1_cdc_dedupe", "full", "l4_only", "cdc_dedupe"}  # VALIDATION_METHODS.md:458-464 + BASELINE configs[1]
    assert ABLATIONS["full"] == 15


def test_gear_table_and_sizing_host_side(orc):
    from hmse_amd import IngestConfig, _lib, ops
    t = np.zeros(256, np.uint64)
    _lib.hip_lib().hmse_gear_table(t.ctypes.data)
    assert np.array_equal(t, orc.gear_table())
    cfg = IngestConfig()
    for stage in (2, 3, 4, 5, 6, 7):
        assert ops.workspace_bytes(stage, 1 << 20, cfg) > 0
    assert ops.workspace_bytes(2, 1 << 30, cfg) > ops.workspace_bytes(2, 1 << 20, cfg)
    assert ops.workspace_bytes(99, 1, cfg) == 0
    assert _lib.hip_lib().hmse_strerror(-2) == b"buffer or workspace too small"


def test_product_path_fails_loudly_without_gpu():
    """No CPU fallback anywhere in hmse_amd: host tensors are refused."""
    import torch
    from hmse_amd import IngestConfig, ops
    x = torch.zeros(1000, dtype=torch.uint8)
    with pytest.raises(ops.HmseError):
        ops.l2_cdc(x, IngestConfig())
    with pytest.raises(ops.HmseError):
        ops.l3_sha256(x, torch.tensor([0, 1000]))
    with pytest.raises(ops.HmseError):
        ops.l4_minhash(x, torch.tensor([0, 1000]), IngestConfig())


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "hmse_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".c", ".cpp")):
                src = open(os.path.join(dp, fn), errors="ignore").read()
                assert "import oracle" not in src and "from oracle" not in src and "liborc" not in src, fn


def test_torch_ops_are_registered_and_have_no_cpu_path():
    """the stage operators are reachable as torch.ops.hmse.* (tensors in, tensors out); like ops.py they
    refuse host tensors — there is no CPU implementation behind the registration."""
    import torch
    from hmse_amd import ops, torch_ops  # noqa: F401  (importing registers the library)
    for name in ("l2_cdc", "l3_sha256", "l3_dedup", "l4_minhash", "l4_lsh", "l1_deflate", "l1_inflate"):
        assert hasattr(torch.ops.hmse, name), name
    assert "min_size" in str(torch.ops.hmse.l2_cdc.default._schema)
    x = torch.zeros(5000, dtype=torch.uint8)
    with pytest.raises(ops.HmseError):
        torch.ops.hmse.l2_cdc(x)
    with pytest.raises(ops.HmseError):
        torch.ops.hmse.l3_sha256(x, torch.tensor([0, 5000]))


def test_inflate_mode_knob_and_minhash_workspace():
    """hmse_l1_inflate_mode accepts 0/1/2 only; the MinHash workspace carries the 2 MiB memo table (include/hmse.h)."""
    from hmse_amd import IngestConfig, _lib, ops
    lib = _lib.hip_lib()
    assert lib.hmse_l1_inflate_mode(3) == -1 and lib.hmse_l1_inflate_mode(-1) == -1
    for m in (1, 2, 0):
        assert lib.hmse_l1_inflate_mode(m) == 0
    assert ops.workspace_bytes(ops.STAGE_MINHASH, 1000, IngestConfig()) == 256 + (8 << 18)
