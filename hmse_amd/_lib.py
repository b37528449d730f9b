"""ctypes loader for the C-ABI libraries built in hmse_amd/csrc (include/hmse.h).

The HIP library is the product: if it is missing the import FAILS LOUDLY — there is no CPU
fallback anywhere in this package (the CPU oracle lives in oracle/ and is test infrastructure).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import NamedTuple

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# HMSE_LIB_VARIANT=<tag> (diagnostics / A-B experiments only): load csrc/libhmse_hip_<tag>.so instead — e.g. the stamps or diag build
HIP_LIB_PATH = os.path.join(_CSRC, "libhmse_hip" + ("_" + os.environ["HMSE_LIB_VARIANT"] if os.environ.get("HMSE_LIB_VARIANT") else "") + ".so")
CORPUS_LIB_PATH = os.path.join(_CSRC, "libhmse_corpus.so")
GUNZIP_LIB_PATH = os.path.join(_CSRC, "libhmse_gunzip.so")     # include/hmse_gunzip.h: the gzip import, beside the C ABI of include/hmse.h
REGEXA_LIB_PATH = os.path.join(_CSRC, "libhmse_regexa.so")     # include/hmse_regexa.h: the regex search with assertions, likewise
TALLY_LIB_PATH = os.path.join(_CSRC, "libhmse_tally.so")       # include/hmse_tally.h: the tally of search results, likewise
SUBST_LIB_PATH = os.path.join(_CSRC, "libhmse_subst.so")       # include/hmse_subst.h: the substitution of ranges, likewise
ORDER_LIB_PATH = os.path.join(_CSRC, "libhmse_order.so")       # include/hmse_order.h: the order of search results, likewise


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


class HmseRegexa(C.Structure):
    """Mirror of `hmse_regexa` (include/hmse_regexa.h): a regular expression compiled with assertions — its header and its device arrays."""

    _fields_ = [("struct_size", C.c_uint32), ("n_states", C.c_uint32), ("n_classes", C.c_uint32), ("reach", C.c_uint32),
                ("start", C.c_uint32 * 4), ("table", C.c_void_p), ("classmap", C.c_void_p)]


def build(force: bool = False) -> None:
    """Compile every HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "-s", "-j8"]
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "-s", "clean"])
    subprocess.check_call(args)


# Every entry point of include/hmse.h, once: "<return>: <kind> <name>, ..." in the header's parameter order and under its parameter names
# (tests/test_abi.py holds the table against the header).  A parameter's kind is one of
#   u8* u32* i32* u64* i64*       a DEVICE pointer to elements of that width -> c_void_p; ops._call refuses a tensor of another element size
#   void*                         a device pointer to opaque bytes (workspaces, exchange rows, packed records): no width to check
#   u8*? ... void*?               the same, and ops._call passes NULL for an EMPTY tensor
#   u8[] u32[] u64[] f64[]        a HOST array, read or written during the call -> POINTER(c_...)
#   hmse_cfg* hmse_stream* hmse_gl4* hmse_findset* hmse_regex*      a HOST struct -> POINTER(its mirror above)
#   u32 u64 size_t int            a scalar
#   stream                        the HIP stream, always last: the entry point enqueues device work (ops._call appends the current stream)
# and it returns int (a status), void, u64, size_t or str.  hmse_gear_table fills a host table; it takes its address like a device pointer's.
SIGNATURES = {
    "hmse_cfg_default": "void: hmse_cfg* cfg",
    "hmse_cfg_validate": "int: hmse_cfg* cfg",
    "hmse_abi_version": "int:",
    "hmse_strerror": "str: int code",
    "hmse_gear_table": "void: u64* table",
    "hmse_workspace_bytes": "size_t: int stage, u64 n, hmse_cfg* cfg",
    "hmse_l2_cdc": "int: u8* data, u64 n, u64* seg_off, u32 n_seg, hmse_cfg* cfg, u64* cuts, u64 cuts_cap, u64* n_cuts, u32* status, "
                   "void* ws, size_t ws_bytes, stream",
    "hmse_l3_sha256": "int: u8* data, u64 n, u64* cuts, u64 n_chunks, u8* digests, void* ws, size_t ws_bytes, stream",
    "hmse_l3_dedup": "int: u8* digests_all, u64 n_all, u64* first_occ, u32* refcount, void* ws, size_t ws_bytes, stream",
    "hmse_l3_index_slots": "u64: u64 capacity_chunks",
    "hmse_l3_index_update": "int: u8* digests_all, u64 n_old, u64 n_new, u64* first_occ, u32* refcount, u32* table, u64 slots, stream",
    "hmse_l4_minhash": "int: u8* data, u64 n, u64* cuts, u64* chunk_ids, u64 n_sel, hmse_cfg* cfg, u32* sig, void* ws, size_t ws_bytes, stream",
    "hmse_l4_lsh": "int: u32* sig, u64 n_sel, hmse_cfg* cfg, u32* band_keys, i64* base, void* ws, size_t ws_bytes, stream",
    "hmse_l4_lsh_slots": "u64: u64 capacity_chunks",
    "hmse_l4_lsh_update": "int: u32* sig_all, u64 n_old, u64 n_new, hmse_cfg* cfg, u32* band_keys, i64* base, u32* tables, u64 slots, u32 keys_given, stream",
    "hmse_l1_deflate": "int: u8* data, u64 n, u64* cuts, u64* chunk_ids, i64* base, u64 n_sel, hmse_cfg* cfg, u8* out, u64 out_cap, u64* out_off, "
                       "u8* kind, u32* status, void* ws, size_t ws_bytes, stream",
    "hmse_l1_deflate_record_bytes": "u64: u32 chunk_len",
    "hmse_l1_deflate_record_bytes_dict": "u64: u32 chunk_len",
    "hmse_l1_deflate_ex": "int: u8* data, u64 n, u64* cuts, u64* chunk_ids, i64* base, u64 n_sel, hmse_cfg* cfg, u32 flags, u8* out, u64 out_cap, "
                          "u64* out_off, u8* kind, u32* status, void* ws, size_t ws_bytes, stream",
    "hmse_l1_inflate": "int: u8* streams, u64 streams_bytes, u64* stream_off, u32* stream_len, u8* kind, i64* base, u64 n_sel, u64* raw_off, "
                       "u8* raw_out, u64 raw_cap, u8* ok, u32* status, void* ws, size_t ws_bytes, stream",
    "hmse_l1_inflate_mode": "int: int mode",
    "hmse_read_assemble": "int: u64* cuts, u64 n_chunks, u64* slot_of_chunk, u64 n_slots, u64* raw_off, u8* raw, u8* data_out, u64 n, u32* status, stream",
    "hmse_stream_batch_workspace_bytes": "u64: u64 batch_bytes, hmse_cfg* cfg",
    "hmse_stream_workspace_init": "int: void* ws, size_t ws_bytes, u64 batch_bytes, hmse_cfg* cfg, stream",
    "hmse_stream_batch": "int: u8* data, u64 data_cap, u64 batch_bytes, u64* seg_off, u32 n_seg, hmse_cfg* cfg, hmse_stream* s, "
                         "void* ws, size_t ws_bytes, stream",
    "hmse_stream_row_bytes": "u64: u64 cap_bytes, hmse_cfg* cfg",
    "hmse_stream_piece_hash": "int: u8* data, u64 data_cap, u64 piece_bytes, u64 cap_bytes, u64* seg_off, u32 n_seg, hmse_cfg* cfg, hmse_stream* s, "
                              "void* row, void* ws, size_t ws_bytes, stream",
    "hmse_stream_piece_encode": "int: u8* data, u64 data_cap, u64 piece_bytes, u64 cap_bytes, hmse_cfg* cfg, hmse_stream* s, void* rows, "
                                "void* ws, size_t ws_bytes, stream",
    "hmse_stream_sig_cap": "u64: u64 cap_bytes, hmse_cfg* cfg",
    "hmse_stream_sig_row_bytes": "u64: u64 cap_bytes, hmse_cfg* cfg",
    "hmse_stream_piece_sign": "int: u8* data, u64 data_cap, u64 piece_bytes, u64 cap_bytes, hmse_cfg* cfg, hmse_stream* s, void* rows, void* sig_row, "
                              "void* ws, size_t ws_bytes, stream",
    "hmse_stream_piece_bases": "int: u64 cap_bytes, hmse_cfg* cfg, hmse_stream* s, void* sig_rows, hmse_gl4* g, void* ws, size_t ws_bytes, stream",
    "hmse_stream_piece_encode_g": "int: u8* data, u64 data_cap, u64 piece_bytes, u64 cap_bytes, hmse_cfg* cfg, hmse_stream* s, u64* gstate, "
                                  "void* ws, size_t ws_bytes, stream",
    "hmse_manifest_pack": "int: u8* streams, u64* stream_off, u8* kind, i64* base, u64* uniq_ids, u64 n_unique, u8* digests, u32* refcount, u64* cuts, "
                          "u64 n_chunks, u64* first_occ, u64 chunk_base, u32 shard, u64* shard_bases, u32 n_shards, u64* rec_off, u32 lba_unit, "
                          "u64* ptr_index, u8* blob, u64 blob_bytes, void* index, void* chunk_map, void*? pointers, u64 n_pointers, u32* status, "
                          "void* ws, size_t ws_bytes, stream",
    "hmse_manifest_pack_ex": "int: u8* streams, u64* stream_off, u8* kind, i64* base, u64* uniq_ids, u64 n_unique, u8* digests, u32* refcount, u64* cuts, "
                             "u64 n_chunks, u64* first_occ, u64 chunk_base, u32 shard, u64* shard_bases, u32 n_shards, u32 flags, u64* rec_off, "
                             "u32 lba_unit, u64* ptr_index, u8* blob, u64 blob_bytes, void* index, void* chunk_map, void*? pointers, u64 n_pointers, "
                             "u32* status, void* ws, size_t ws_bytes, stream",
    "hmse_gc_plan": "int: u64* cuts, u64 n_chunks, u32* slot, u64 n_slots, u64* seg_off, u32 n_seg, u8* drop, u8* digests_old, u64* counts, "
                    "i64* old_chunk, i64* first_occ, u32* refcount, u8* digests, i64* uniq_ids, i64* old_slot, i64* new_slot_of_old, u32* status, "
                    "void* ws, size_t ws_bytes, stream",
    "hmse_record_gather": "int: u8*? src0, u64 src0_bytes, u8*? src1, u64 src1_bytes, u64* src_off, u8* src_sel, u64* dst_off, u64 n, u8*? dst, "
                          "u64 dst_bytes, u32* status, stream",
    "hmse_band_tables_bound": "u64: u64 n, u32 bands, u32 band_bits, u32 n_hashes",
    "hmse_band_tables_workspace_bytes": "size_t: u64 n",
    "hmse_band_tables_write": "int: u32*? band_keys, u64 n, u32 bands, u32 band_bits, u32*? sig, u32 n_hashes, u8* out, u64 out_cap, u64* out_bytes, "
                              "u32* status, void* ws, size_t ws_bytes, stream",
    "hmse_l4_index_build": "int: u32*? keys, u64 n, u32 bands, u32*? sorted_keys, u32*? sorted_ids, u32* status, void* ws, size_t ws_bytes, stream",
    "hmse_l4_query": "int: u32*? sig_q, u32*? keys_q, u64 n_q, u32*? sig_s, u64 n_s, u32*? sorted_keys, u32*? sorted_ids, hmse_cfg* cfg, u32 top_k, "
                     "u32 min_score, u32 flags, i64*? out_ids, i32*? out_scores, u32*? n_hits, u64*? n_candidates, u32* status, "
                     "void* ws, size_t ws_bytes, stream",
    "hmse_scrub_records": "int: u8* blob, u64 blob_bytes, u64 n, u32 n_shards, u32*? rec_shard, u64*? shard_blob, u64*? shard_slot, u32*? lba_unit, "
                          "u32*? lba, u32*? rec_len, u8*? kind, i64*? remote, u32*? sorted_lba, u32*? sorted_slot, u32 steps, u8*? meta, u8* status, "
                          "i64* dict, u64* padding, stream",
    "hmse_scrub_attribute": "int: u64 n, u8*? status, i64*? dict, u8*? ok, u8*? got_sha, u8*? want_sha, u32 check_digest, u32 max_depth_log2, "
                            "u64 n_chunks, i64*? chunk_slot, u64* cuts, u8* status_out, i64* root, i64* chunk_root, u64* root_records, u64* root_chunks, "
                            "u64* root_bytes, u64* ranges, u64* counts, void* ws, size_t ws_bytes, stream",
    "hmse_find_scan": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u32* mult, u8* pat, u32[] pat_off, u32 n_pat, u32 flags, "
                      "u64* hits, u64 hits_cap, u64* n_hits, u64* counts, u32* status, stream",
    "hmse_find_seams": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u8* pat, u32[] pat_off, u32 n_pat, "
                       "u32 flags, u64* hits, u64 hits_cap, u64* n_hits, u64* counts, u32* status, stream",
    "hmse_find_place": "int: u64*? hits, u64 n_hits, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u64* chunk_out, "
                       "u64* out, u64 out_cap, u32* status, stream",
    "hmse_findset_scan": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u32* mult, hmse_findset* set, u32 flags, "
                         "u64* hits, u64 hits_cap, u64* n_hits, u64*? counts, u32* status, stream",
    "hmse_findset_seams": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, hmse_findset* set, u32 flags, "
                          "u64* hits, u64 hits_cap, u64* n_hits, u64*? counts, u32* status, stream",
    "hmse_findset_place": "int: u64*? hits, u64 n_hits, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u64* chunk_out, "
                          "u64* out, u64 out_cap, u32* status, stream",
    "hmse_sync_match": "int: u8*? a, u64 a_bytes, u64*? a_off, u32*? a_len, u64 n, u8*? b, u64 b_bytes, u64*? b_off, u32*? b_len, u64 n_b, i64*? cand, "
                       "u8*? same, u32* status, stream",
    "hmse_lines_extent": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u64*? pos, u64 n, u32 delim, "
                         "u32 before, u32 after, u32 reach, u64*? start, u64*? end, u8*? flags, u32* status, stream",
    "hmse_lines_gather": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u64*? start, u64*? end, "
                         "u64* out_off, u64 n, u8* out, u64 out_cap, u32* status, stream",
    "hmse_regex_scan": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u32* mult, hmse_regex* rx, "
                       "u64* hits, u64 hits_cap, u64* n_hits, u64* count, u32* status, stream",
    "hmse_regex_seams": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, hmse_regex* rx, "
                        "u64* hits, u64 hits_cap, u64* n_hits, u64* count, u32* status, stream",
    "hmse_approx_scan": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u32* mult, u8* pat, u32[] pat_off, u8[] k, u32 n_pat, u32 flags, "
                        "u64* hits, u64 hits_cap, u64* n_hits, u64* counts, u32* status, stream",
    "hmse_approx_seams": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u8* pat, u32[] pat_off, u8[] k, "
                         "u32 n_pat, u32 flags, u64* hits, u64 hits_cap, u64* n_hits, u64* counts, u32* status, stream",
    "hmse_approx_spans": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u8* pat, u32[] pat_off, u32 n_pat, "
                         "u32 flags, u64*? hits, u64 n, u64* start, u32* status, stream",
    "hmse_crc32": "int: u8*? data, u64 n, u64* cuts, u64 n_chunks, u32*? crc_out, u32* status, stream",
    "hmse_crc32_combine": "int: u32*? crc, u64*? len, u64 n, u32* out, u32* status, stream",
    "hmse_gzip_members": "int: u8*? src0, u64 src0_bytes, u8*? src1, u64 src1_bytes, u64* src_off, u64* stream_len, u8* src_sel, u32* crc, u64* raw_off, "
                         "u64 n_rec, u64* slot, u64 n_chunks, u64* member_off, u32 flags, u8*? dst, u64 dst_bytes, u32* status, stream",
    "hmse_profile_enable": "void: int on",
    "hmse_profile_read": "int: int stage, f64[] total_ms, u64[] launches, int reset",
    "hmse_profile_counter": "int: int slot, u64[] value, int reset",
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
# The entry points of include/hmse_gunzip.h (the gzip import, csrc/libhmse_gunzip.so) in the same notation; tests/test_gunzip_host.py holds this
# table against that header.  hip_lib() hands them out beside the others, so ops._call is the one call path for both libraries.
GUNZIP_SIGNATURES = {
    "hmse_gzip_workspace_bytes": "size_t: u64 n",
    "hmse_gzip_candidates": "int: u8*? data, u64 n, u64*? cand_off, u64 cap, u64* count, u32* status, void* ws, size_t ws_bytes, stream",
    "hmse_gzip_measure": "int: u8*? data, u64 n, u64*? cand_off, u64 n_cand, u64*? stream_off, u64*? end, u64*? raw_len, u32*? crc, u32*? flags, "
                         "u32* status, void* ws, size_t ws_bytes, stream",
}
# The entry points of include/hmse_regexa.h (the regex search with assertions, csrc/libhmse_regexa.so); tests/test_regexa_host.py holds this
# table against that header.  Parsed into a table of its own (PARSED_REGEXA); ops._call looks a name up in PARSED, then there.
REGEXA_SIGNATURES = {
    "hmse_regexa_scan": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u32* mult, hmse_regexa* rx, "
                        "u64* hits, u64 hits_cap, u64* n_hits, u64* count, u32* status, stream",
    "hmse_regexa_seams": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, hmse_regexa* rx, "
                         "u64* hits, u64 hits_cap, u64* n_hits, u64* count, u32* status, stream",
}
# The entry points of include/hmse_tally.h (the tally of search results, csrc/libhmse_tally.so); tests/test_tally_host.py holds this table
# against that header.  Parsed into a table of its own (PARSED_TALLY); ops._call looks a name up in PARSED, PARSED_REGEXA, then there.
TALLY_SIGNATURES = {
    "hmse_tally_keys": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u64*? start, u64*? end, u64 n, "
                       "u32 flags, u64 seed, u32 key_bits, u64*? key, u32* status, stream",
    "hmse_tally_same": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u64*? start, u64*? end, u64*? rep, "
                       "u64 n, u32 flags, u8*? same, u32* status, stream",
}
# The entry point of include/hmse_subst.h (the substitution of ranges, csrc/libhmse_subst.so); tests/test_subst_host.py holds this table
# against that header.  Parsed into a table of its own (PARSED_SUBST); ops._call looks a name up there after PARSED_TALLY.
SUBST_SIGNATURES = {
    "hmse_subst_apply": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u64*? start, u64*? end, u64*? sel, "
                        "u64 n, u8*? rep, u64 rep_bytes, u64*? rep_off, u64 n_rep, u32 flags, u64* out_off, u8*? out, u64 out_cap, u32* status, stream",
}
# The entry points of include/hmse_order.h (the order of search results, csrc/libhmse_order.so); tests/test_order_host.py holds this table
# against that header.  Parsed into a table of its own (PARSED_ORDER); ops._call looks a name up there after PARSED_SUBST.
ORDER_SIGNATURES = {
    "hmse_order_keys": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u64*? start, u64*? end, u64*? depth, "
                       "u64 n, u32 flags, u64*? key, u32* status, stream",
    "hmse_order_lcp": "int: u8*? raw, u64 raw_bytes, u64* raw_off, u64 n_rec, u64* cuts, u64*? slot, u64 n_chunks, u64*? start, u64*? end, u64*? rep, "
                      "u64*? from, u64 n, u32 flags, u64*? lcp, u32* status, stream",
}

_ELEM = {"u8": C.c_uint8, "u32": C.c_uint32, "i32": C.c_int32, "u64": C.c_uint64, "i64": C.c_int64, "f64": C.c_double}
_SCALAR = {"u32": C.c_uint32, "u64": C.c_uint64, "size_t": C.c_size_t, "int": C.c_int}
_STRUCT = {"hmse_cfg": HmseCfg, "hmse_stream": HmseStream, "hmse_gl4": HmseGl4, "hmse_findset": HmseFindset, "hmse_regex": HmseRegex,
           "hmse_regexa": HmseRegexa}
_RETURN = {"int": C.c_int, "void": None, "u64": C.c_uint64, "size_t": C.c_size_t, "str": C.c_char_p}
DEVICE, HOST, STRUCT, SCALAR, STREAM = range(5)


class Param(NamedTuple):
    name: str
    kind: int          # DEVICE, HOST, STRUCT, SCALAR or STREAM
    ctype: type
    width: int         # DEVICE: the element size a tensor must have; 0: opaque bytes
    null_if_empty: bool


def _param(text: str) -> Param:
    if text == "stream":
        return Param("stream", STREAM, C.c_void_p, 0, False)
    ty, name = text.split()
    if ty in _SCALAR:
        return Param(name, SCALAR, _SCALAR[ty], 0, False)
    if ty.endswith("[]"):
        return Param(name, HOST, C.POINTER(_ELEM[ty[:-2]]), 0, False)
    base = ty.rstrip("?")[:-1]
    if base in _STRUCT:
        return Param(name, STRUCT, C.POINTER(_STRUCT[base]), 0, False)
    return Param(name, DEVICE, C.c_void_p, 0 if base == "void" else C.sizeof(_ELEM[base]), ty.endswith("?"))


def _parse(sig: str):
    ret, _, params = sig.partition(":")
    return _RETURN[ret], tuple(_param(p.strip()) for p in params.split(",") if p.strip())


PARSED = {name: _parse(sig) for name, sig in {**SIGNATURES, **GUNZIP_SIGNATURES}.items()}      # name -> (restype, parameters)
PARSED_REGEXA = {name: _parse(sig) for name, sig in REGEXA_SIGNATURES.items()}
PARSED_TALLY = {name: _parse(sig) for name, sig in TALLY_SIGNATURES.items()}
PARSED_SUBST = {name: _parse(sig) for name, sig in SUBST_SIGNATURES.items()}
PARSED_ORDER = {name: _parse(sig) for name, sig in ORDER_SIGNATURES.items()}

_hip = None
_corpus = None


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
        if not os.path.exists(GUNZIP_LIB_PATH):
            raise ImportError(f"{GUNZIP_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L._gunzip = G = C.CDLL(GUNZIP_LIB_PATH)          # (it links against libhmse_hip.so, loaded above)
        for name, (restype, params) in PARSED.items():
            fn = getattr(G if name in GUNZIP_SIGNATURES else L, name)
            fn.restype, fn.argtypes = restype, [p.ctype for p in params]
            if name in GUNZIP_SIGNATURES:
                setattr(L, name, fn)
        if not os.path.exists(REGEXA_LIB_PATH):
            raise ImportError(f"{REGEXA_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L._regexa = A = C.CDLL(REGEXA_LIB_PATH)          # (it links against libhmse_hip.so as well)
        for name, (restype, params) in PARSED_REGEXA.items():
            fn = getattr(A, name)
            fn.restype, fn.argtypes = restype, [p.ctype for p in params]
            setattr(L, name, fn)
        if not os.path.exists(TALLY_LIB_PATH):
            raise ImportError(f"{TALLY_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L._tally = T = C.CDLL(TALLY_LIB_PATH)            # (it links against libhmse_hip.so as well)
        for name, (restype, params) in PARSED_TALLY.items():
            fn = getattr(T, name)
            fn.restype, fn.argtypes = restype, [p.ctype for p in params]
            setattr(L, name, fn)
        if not os.path.exists(SUBST_LIB_PATH):
            raise ImportError(f"{SUBST_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L._subst = S = C.CDLL(SUBST_LIB_PATH)            # (it links against libhmse_hip.so as well)
        for name, (restype, params) in PARSED_SUBST.items():
            fn = getattr(S, name)
            fn.restype, fn.argtypes = restype, [p.ctype for p in params]
            setattr(L, name, fn)
        if not os.path.exists(ORDER_LIB_PATH):
            raise ImportError(f"{ORDER_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L._order = O = C.CDLL(ORDER_LIB_PATH)            # (it links against libhmse_hip.so as well)
        for name, (restype, params) in PARSED_ORDER.items():
            fn = getattr(O, name)
            fn.restype, fn.argtypes = restype, [p.ctype for p in params]
            setattr(L, name, fn)
        _hip = L
    return _hip


def corpus_lib():
    global _corpus
    if _corpus is None:
        if not os.path.exists(CORPUS_LIB_PATH):
            raise ImportError(f"{CORPUS_LIB_PATH} is missing: run __graft_entry__.build()")
        L = C.CDLL(CORPUS_LIB_PATH)
        L.hmse_corpus_generate.restype = C.c_int
        L.hmse_corpus_generate.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int]
        _corpus = L
    return _corpus
