"""ctypes loader for the C-ABI libraries built in hmse_amd/csrc (include/hmse.h).

The HIP library is the product: if it is missing the import FAILS LOUDLY — there is no CPU
fallback anywhere in this package (the CPU oracle lives in oracle/ and is test infrastructure).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# HMSE_LIB_VARIANT=<tag> (diagnostics / A-B experiments only): load csrc/libhmse_hip_<tag>.so instead — e.g. the stamps or diag build
HIP_LIB_PATH = os.path.join(_CSRC, "libhmse_hip" + ("_" + os.environ["HMSE_LIB_VARIANT"] if os.environ.get("HMSE_LIB_VARIANT") else "") + ".so")
CORPUS_LIB_PATH = os.path.join(_CSRC, "libhmse_corpus.so")


class HmseCfg(C.Structure):
    """Mirror of `hmse_cfg` (include/hmse.h)."""

    _fields_ = [(n, C.c_uint32) for n in (
        "struct_size", "min_size", "avg_size", "max_size", "norm_level", "seg_size",
        "n_hashes", "shingle", "seed_base", "bands", "rows", "band_bits",
        "level", "chain_depth", "layers", "delta_max_ratio_pct")]


class HmseGl4(C.Structure):
    """Mirror of `hmse_gl4` (include/hmse.h): the global-L4 arrays of a multi-rank stream (device pointers and capacities)."""

    _fields_ = [("struct_size", C.c_uint32), ("world", C.c_uint32), ("rank", C.c_uint32), ("reserved", C.c_uint32),
                ("sig_cap", C.c_uint64), ("max_stored_g", C.c_uint64), ("gstate", C.c_void_p), ("sig_g", C.c_void_p), ("band_keys_g", C.c_void_p),
                ("base_g", C.c_void_p), ("lsh_tables_g", C.c_void_p), ("lsh_slots_g", C.c_uint64), ("g_owner", C.c_void_p), ("g_local", C.c_void_p),
                ("ug", C.c_void_p), ("base_global", C.c_void_p), ("req_counts", C.c_void_p), ("req_slots", C.c_void_p), ("ghost_chunk0", C.c_uint64)]


class HmseStream(C.Structure):
    """Mirror of `hmse_stream` (include/hmse.h): what is fixed for a stream's life — its persistent arrays (device pointers) and capacities."""

    _fields_ = [("struct_size", C.c_uint32), ("world", C.c_uint32), ("rank", C.c_uint32), ("reserved", C.c_uint32),
                ("state", C.c_void_p), ("cuts", C.c_void_p), ("max_chunks", C.c_uint64), ("gidx", C.c_void_p), ("digests", C.c_void_p), ("max_chunks_g", C.c_uint64),
                ("first_occ", C.c_void_p), ("refcount", C.c_void_p), ("l3_table", C.c_void_p), ("l3_slots", C.c_uint64), ("uniq", C.c_void_p), ("max_unique", C.c_uint64),
                ("sig", C.c_void_p), ("band_keys", C.c_void_p), ("base", C.c_void_p), ("lsh_tables", C.c_void_p), ("lsh_slots", C.c_uint64),
                ("kind", C.c_void_p), ("stream_off", C.c_void_p), ("out", C.c_void_p), ("out_cap", C.c_uint64)]


class HmseFindset(C.Structure):
    """Mirror of `hmse_findset` (include/hmse.h): a compiled pattern set — its header and its device arrays."""

    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_entries", C.c_uint32), ("n_ids", C.c_uint32), ("dir_bits", C.c_uint32),
                ("max_len", C.c_uint32), ("pat_bytes", C.c_uint64), ("upat", C.c_void_p), ("uoff", C.c_void_p), ("ukey", C.c_void_p),
                ("uid", C.c_void_p), ("dir", C.c_void_p), ("bitmap", C.c_void_p)]


class HmseRegex(C.Structure):
    """Mirror of `hmse_regex` (include/hmse.h): a compiled regular expression — its header and its device arrays."""

    _fields_ = [("struct_size", C.c_uint32), ("n_states", C.c_uint32), ("n_classes", C.c_uint32), ("reach", C.c_uint32),
                ("table", C.c_void_p), ("classmap", C.c_void_p)]


def build(force: bool = False) -> None:
    """Compile every HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "-s", "-j8"]
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "-s", "clean"])
    subprocess.check_call(args)


_hip = None
_corpus = None

_VP, _U64, _U32, _SZ = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t


def hip_lib():
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise ImportError(
                f"{HIP_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hmse_amd has no CPU fallback)")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same SONAME as
        # /opt/rocm's).  Import torch FIRST so that the C-ABI library binds to the runtime that owns the
        # tensors and streams it will be handed; loaded the other way round, the process ends up with
        # two runtimes and every launch fails with a HIP error.
        import torch  # noqa: F401
        L = C.CDLL(HIP_LIB_PATH)
        cfgp, strp = C.POINTER(HmseCfg), C.POINTER(HmseStream)
        L.hmse_cfg_default.argtypes = [cfgp]
        L.hmse_cfg_validate.argtypes = [cfgp]
        L.hmse_cfg_validate.restype = C.c_int
        L.hmse_abi_version.restype = C.c_int
        L.hmse_strerror.restype = C.c_char_p
        L.hmse_strerror.argtypes = [C.c_int]
        L.hmse_gear_table.argtypes = [_VP]
        L.hmse_workspace_bytes.restype = _SZ
        L.hmse_workspace_bytes.argtypes = [C.c_int, _U64, cfgp]
        L.hmse_l2_cdc.restype = C.c_int
        L.hmse_l2_cdc.argtypes = [_VP, _U64, _VP, _U32, cfgp, _VP, _U64, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_l3_sha256.restype = C.c_int
        L.hmse_l3_sha256.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _SZ, _VP]
        L.hmse_l3_dedup.restype = C.c_int
        L.hmse_l3_dedup.argtypes = [_VP, _U64, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_l3_index_slots.restype = _U64
        L.hmse_l3_index_slots.argtypes = [_U64]
        L.hmse_l3_index_update.restype = C.c_int
        L.hmse_l3_index_update.argtypes = [_VP, _U64, _U64, _VP, _VP, _VP, _U64, _VP]
        L.hmse_l4_lsh_slots.restype = _U64
        L.hmse_l4_lsh_slots.argtypes = [_U64]
        L.hmse_l4_lsh_update.restype = C.c_int
        L.hmse_l4_lsh_update.argtypes = [_VP, _U64, _U64, cfgp, _VP, _VP, _VP, _U64, _U32, _VP]
        L.hmse_l4_minhash.restype = C.c_int
        L.hmse_l4_minhash.argtypes = [_VP, _U64, _VP, _VP, _U64, cfgp, _VP, _VP, _SZ, _VP]
        L.hmse_l4_lsh.restype = C.c_int
        L.hmse_l4_lsh.argtypes = [_VP, _U64, cfgp, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_l1_deflate.restype = C.c_int
        L.hmse_l1_deflate.argtypes = [_VP, _U64, _VP, _VP, _VP, _U64, cfgp, _VP, _U64, _VP, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_l1_deflate_ex.restype = C.c_int
        L.hmse_l1_deflate_ex.argtypes = [_VP, _U64, _VP, _VP, _VP, _U64, cfgp, _U32, _VP, _U64, _VP, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_l1_deflate_record_bytes.restype = _U64
        L.hmse_l1_deflate_record_bytes.argtypes = [_U32]
        L.hmse_l1_deflate_record_bytes_dict.restype = _U64
        L.hmse_l1_deflate_record_bytes_dict.argtypes = [_U32]
        L.hmse_l1_inflate_mode.restype = C.c_int
        L.hmse_l1_inflate_mode.argtypes = [C.c_int]
        L.hmse_l1_inflate.restype = C.c_int
        L.hmse_l1_inflate.argtypes = [_VP, _U64, _VP, _VP, _VP, _VP, _U64, _VP, _VP, _U64, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_read_assemble.restype = C.c_int
        L.hmse_read_assemble.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _VP, _U64, _VP, _VP]
        L.hmse_stream_batch_workspace_bytes.restype = _U64
        L.hmse_stream_batch_workspace_bytes.argtypes = [_U64, cfgp]
        L.hmse_stream_workspace_init.restype = C.c_int
        L.hmse_stream_workspace_init.argtypes = [_VP, _SZ, _U64, cfgp, _VP]
        L.hmse_stream_batch.restype = C.c_int
        L.hmse_stream_batch.argtypes = [_VP, _U64, _U64, _VP, _U32, cfgp, strp, _VP, _SZ, _VP]
        L.hmse_stream_row_bytes.restype = _U64
        L.hmse_stream_row_bytes.argtypes = [_U64, cfgp]
        L.hmse_stream_piece_hash.restype = C.c_int
        L.hmse_stream_piece_hash.argtypes = [_VP, _U64, _U64, _U64, _VP, _U32, cfgp, strp, _VP, _VP, _SZ, _VP]
        L.hmse_stream_piece_encode.restype = C.c_int
        L.hmse_stream_piece_encode.argtypes = [_VP, _U64, _U64, _U64, cfgp, strp, _VP, _VP, _SZ, _VP]
        L.hmse_stream_sig_cap.restype = _U64
        L.hmse_stream_sig_cap.argtypes = [_U64, cfgp]
        L.hmse_stream_sig_row_bytes.restype = _U64
        L.hmse_stream_sig_row_bytes.argtypes = [_U64, cfgp]
        L.hmse_stream_piece_sign.restype = C.c_int
        L.hmse_stream_piece_sign.argtypes = [_VP, _U64, _U64, _U64, cfgp, strp, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_stream_piece_bases.restype = C.c_int
        L.hmse_stream_piece_bases.argtypes = [_U64, cfgp, strp, _VP, C.POINTER(HmseGl4), _VP, _SZ, _VP]
        L.hmse_stream_piece_encode_g.restype = C.c_int
        L.hmse_stream_piece_encode_g.argtypes = [_VP, _U64, _U64, _U64, cfgp, strp, _VP, _VP, _SZ, _VP]
        L.hmse_manifest_pack.restype = C.c_int
        L.hmse_manifest_pack.argtypes = [_VP, _VP, _VP, _VP, _VP, _U64, _VP, _VP, _VP, _U64, _VP, _U64, _U32, _VP, _U32, _VP, _U32, _VP,
                                         _VP, _U64, _VP, _VP, _VP, _U64, _VP, _VP, _SZ, _VP]
        L.hmse_manifest_pack_ex.restype = C.c_int
        L.hmse_manifest_pack_ex.argtypes = [_VP, _VP, _VP, _VP, _VP, _U64, _VP, _VP, _VP, _U64, _VP, _U64, _U32, _VP, _U32, _U32, _VP, _U32, _VP,
                                            _VP, _U64, _VP, _VP, _VP, _U64, _VP, _VP, _SZ, _VP]
        L.hmse_gc_plan.restype = C.c_int
        L.hmse_gc_plan.argtypes = [_VP, _U64, _VP, _U64, _VP, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_record_gather.restype = C.c_int
        L.hmse_record_gather.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _VP, _U64, _VP, _U64, _VP, _VP]
        L.hmse_band_tables_bound.restype = _U64
        L.hmse_band_tables_bound.argtypes = [_U64, _U32, _U32, _U32]
        L.hmse_band_tables_workspace_bytes.restype = _SZ
        L.hmse_band_tables_workspace_bytes.argtypes = [_U64]
        L.hmse_band_tables_write.restype = C.c_int
        L.hmse_band_tables_write.argtypes = [_VP, _U64, _U32, _U32, _VP, _U32, _VP, _U64, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_l4_index_build.restype = C.c_int
        L.hmse_l4_index_build.argtypes = [_VP, _U64, _U32, _VP, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_l4_query.restype = C.c_int
        L.hmse_l4_query.argtypes = [_VP, _VP, _U64, _VP, _U64, _VP, _VP, cfgp, _U32, _U32, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _SZ, _VP]
        L.hmse_scrub_records.restype = C.c_int
        L.hmse_scrub_records.argtypes = [_VP, _U64, _U64, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP, _VP, _VP]
        L.hmse_scrub_attribute.restype = C.c_int
        L.hmse_scrub_attribute.argtypes = [_U64, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _U64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                           _VP, _SZ, _VP]
        u32p = C.POINTER(C.c_uint32)      # the patterns' bounds: a HOST array, read during the call
        L.hmse_find_scan.restype = C.c_int
        L.hmse_find_scan.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, u32p, _U32, _U32, _VP, _U64, _VP, _VP, _VP, _VP]
        L.hmse_find_seams.restype = C.c_int
        L.hmse_find_seams.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _U64, _VP, u32p, _U32, _U32, _VP, _U64, _VP, _VP, _VP, _VP]
        L.hmse_find_place.restype = C.c_int
        L.hmse_find_place.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _U64, _VP, _VP, _U64, _VP, _VP]
        fsp = C.POINTER(HmseFindset)      # the set's header: a HOST struct, read during the call
        L.hmse_findset_scan.restype = C.c_int
        L.hmse_findset_scan.argtypes = [_VP, _U64, _VP, _U64, _VP, fsp, _U32, _VP, _U64, _VP, _VP, _VP, _VP]
        L.hmse_findset_seams.restype = C.c_int
        L.hmse_findset_seams.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _U64, fsp, _U32, _VP, _U64, _VP, _VP, _VP, _VP]
        L.hmse_findset_place.restype = C.c_int
        L.hmse_findset_place.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _U64, _VP, _VP, _U64, _VP, _VP]
        rxp = C.POINTER(HmseRegex)        # the automaton's header: a HOST struct, read during the call
        L.hmse_regex_scan.restype = C.c_int
        L.hmse_regex_scan.argtypes = [_VP, _U64, _VP, _U64, _VP, rxp, _VP, _U64, _VP, _VP, _VP, _VP]
        L.hmse_regex_seams.restype = C.c_int
        L.hmse_regex_seams.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _U64, rxp, _VP, _U64, _VP, _VP, _VP, _VP]
        u8p = C.POINTER(C.c_uint8)        # the patterns' error bounds: a HOST array, read during the call
        L.hmse_approx_scan.restype = C.c_int
        L.hmse_approx_scan.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, u32p, u8p, _U32, _U32, _VP, _U64, _VP, _VP, _VP, _VP]
        L.hmse_approx_seams.restype = C.c_int
        L.hmse_approx_seams.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _U64, _VP, u32p, u8p, _U32, _U32, _VP, _U64, _VP, _VP, _VP, _VP]
        L.hmse_approx_spans.restype = C.c_int
        L.hmse_approx_spans.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _U64, _VP, u32p, _U32, _U32, _VP, _U64, _VP, _VP, _VP]
        L.hmse_crc32.restype = C.c_int
        L.hmse_crc32.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _VP]
        L.hmse_crc32_combine.restype = C.c_int
        L.hmse_crc32_combine.argtypes = [_VP, _VP, _U64, _VP, _VP, _VP]
        L.hmse_gzip_members.restype = C.c_int
        L.hmse_gzip_members.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _VP, _VP, _VP, _U64, _VP, _U64, _VP, _U32, _VP, _U64, _VP, _VP]
        L.hmse_sync_match.restype = C.c_int
        L.hmse_sync_match.argtypes = [_VP, _U64, _VP, _VP, _U64, _VP, _U64, _VP, _VP, _U64, _VP, _VP, _VP, _VP]
        L.hmse_lines_extent.restype = C.c_int
        L.hmse_lines_extent.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _U64, _VP, _U64, _U32, _U32, _U32, _U32, _VP, _VP, _VP, _VP, _VP]
        L.hmse_lines_gather.restype = C.c_int
        L.hmse_lines_gather.argtypes = [_VP, _U64, _VP, _U64, _VP, _VP, _U64, _VP, _VP, _VP, _U64, _VP, _U64, _VP, _VP]
        L.hmse_profile_enable.argtypes = [C.c_int]
        L.hmse_profile_read.restype = C.c_int
        L.hmse_profile_read.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.hmse_profile_counter.restype = C.c_int
        L.hmse_profile_counter.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.c_int]
        _hip = L
    return _hip


def corpus_lib():
    global _corpus
    if _corpus is None:
        if not os.path.exists(CORPUS_LIB_PATH):
            raise ImportError(f"{CORPUS_LIB_PATH} is missing: run __graft_entry__.build()")
        L = C.CDLL(CORPUS_LIB_PATH)
        L.hmse_corpus_generate.restype = C.c_int
        L.hmse_corpus_generate.argtypes = [_VP, _U64, _U64, _U32, _U64, C.c_int, C.c_int]
        _corpus = L
    return _corpus


EXPORTED_SYMBOLS = (
    "hmse_cfg_default", "hmse_cfg_validate", "hmse_abi_version", "hmse_strerror", "hmse_gear_table",
    "hmse_workspace_bytes", "hmse_l2_cdc", "hmse_l3_sha256", "hmse_l3_dedup", "hmse_l3_index_slots", "hmse_l3_index_update",
    "hmse_l4_lsh_slots", "hmse_l4_lsh_update", "hmse_l4_minhash",
    "hmse_l4_lsh", "hmse_l1_deflate", "hmse_l1_deflate_ex", "hmse_l1_deflate_record_bytes", "hmse_l1_deflate_record_bytes_dict", "hmse_l1_inflate", "hmse_l1_inflate_mode", "hmse_read_assemble", "hmse_manifest_pack", "hmse_manifest_pack_ex", "hmse_stream_batch", "hmse_stream_batch_workspace_bytes", "hmse_stream_workspace_init", "hmse_stream_row_bytes", "hmse_stream_piece_hash", "hmse_stream_piece_encode", "hmse_stream_sig_cap", "hmse_stream_sig_row_bytes", "hmse_stream_piece_sign", "hmse_stream_piece_bases", "hmse_stream_piece_encode_g", "hmse_gc_plan", "hmse_record_gather", "hmse_band_tables_bound", "hmse_band_tables_workspace_bytes", "hmse_band_tables_write", "hmse_l4_index_build", "hmse_l4_query", "hmse_scrub_records", "hmse_scrub_attribute", "hmse_find_scan", "hmse_find_seams", "hmse_find_place", "hmse_findset_scan", "hmse_findset_seams", "hmse_findset_place", "hmse_sync_match", "hmse_lines_extent", "hmse_lines_gather", "hmse_regex_scan", "hmse_regex_seams", "hmse_approx_scan", "hmse_approx_seams", "hmse_approx_spans", "hmse_crc32", "hmse_crc32_combine", "hmse_gzip_members", "hmse_profile_enable", "hmse_profile_read", "hmse_profile_counter")
