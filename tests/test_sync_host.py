"""CPU: replication (hmse_amd.sync) without a GPU — the reference of tests/sync_ref.py on hand-written cases, the patch's serialisation,
the tiling check, the numpy piece table applied by the reference, and the refusals of the wrapper and the entry point.  Stores come from
the CPU oracle through tests/manifest_ref.build."""
import ctypes as C
import dataclasses
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sync_ref as ref
from hmse_amd import sync        # (at import: every test of this file needs the module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 65536


def corpora():
    """S: the eight 64 KiB segments of wiki_synth(8 * 65536, seed=42); Vk: 1-in-200-byte mutations of S0, S0, S1, S0.
    -> the corpora A, B, B2 of the replication tests."""
    from hmse_amd import corpus
    w = corpus.wiki_synth(8 * SEG, seed=42)
    S = [w[i * SEG:(i + 1) * SEG] for i in range(8)]
    rng = np.random.Generator(np.random.PCG64(7))
    V = []
    for k, s in enumerate((S[0], S[0], S[1], S[0])):
        v = s.copy()
        pos = rng.choice(SEG, SEG // 200, replace=False)
        v[pos] ^= rng.integers(1, 256, len(pos), dtype=np.uint8)
        V.append(v)
    cat = lambda *p: np.concatenate(p)
    return {"A": cat(S[0], S[1], V[0], S[2], V[2], S[1]), "B": cat(S[0], S[1], V[1], V[0], S[3], V[2], S[0], S[5][:30000]),
            "B2": cat(V[0], S[0], V[2], S[1])}


@pytest.fixture(scope="module")
def stores(orc):
    import manifest_ref
    from test_host import _shard_result_from_oracle
    return {k: manifest_ref.build(_shard_result_from_oracle(orc, d, {"seg_size": SEG})) for k, d in corpora().items()}


def _patch_from_ref(have, want):
    p = ref.plan(have, want)
    meta = dataclasses.replace(want, blob=np.zeros(0, np.uint8)).to_bytes()
    copied = sum(len(r["stream"]) for r, s in zip(ref.records(want), p["src"]) if s >= 0)
    return sync.Patch(meta, int(want.blob.size), p["delta_hdrs"], p["src"], p["literals"], sync.have_id(have), copied)


# ---- the reference itself -------------------------------------------------------------------------------------------------------------
def test_reference_match_on_hand_written_cases():
    a = b"0123456789abcdef"
    b = b"xx0123456789abcdeX"
    #        equal      last byte differs  shorter     no candidate  candidate out of range   empty = empty   a out of bounds  b out of bounds
    a_off = [0, 0, 0, 0, 0, 16, 10, 0]
    a_len = [15, 16, 15, 4, 4, 0, 7, 4]
    cand = [0, 1, 2, -1, 5, 3, 0, 4]
    b_off, b_len = [2, 2, 2, 18, 16], [15, 16, 14, 0, 3]
    same, status = ref.match(a, a_off, a_len, b, b_off, b_len, cand)
    assert same == [1, 0, 0, 0, 0, 1, 0, 0] and status == 1
    assert ref.match(a, a_off[:4], a_len[:4], b, b_off, b_len, cand[:4]) == ([1, 0, 0, 0], 0)      # unequal lengths and -1: no status bit
    assert ref.match(a, [6], [0], b, [], [], [0]) == ([0], 1)                                        # n_b = 0: every candidate is out of range
    assert ref.match(b"", [], [], b, b_off, b_len, []) == ([], 0)


def test_reference_diff_plan_and_apply_on_the_oracle_s_stores(stores):
    """A = [S0, S1, V0, S2, V2, S1] against B = [S0, S1, V1, V0, S3, V2, S0, S5[:30000]]: records of every class; against
    B2 = [V0, S0, V2, S1]: records whose digest A holds with DIFFERENT stored bytes (the same chunk FULL in one store and DELTA in the
    other) — a plan that copies on digest equality alone does not reproduce B2."""
    from hmse_amd import manifest
    from hmse_amd.config import KIND_DELTA, KIND_POINTER
    A, B, B2 = stores["A"], stores["B"], stores["B2"]
    data = corpora()
    for X, name in ((B, "B"), (B2, "B2")):
        assert manifest.reconstruct(X) == data[name].tobytes()
        d = ref.diff(A, X)
        assert d["shared_bytes"] + d["new_bytes"] == data[name].size and int(d["new_ranges"][:, 1].sum()) == d["new_bytes"]
        assert d["new_unique_bytes"] <= d["new_bytes"] and 0 < d["present"].sum() <= len(d["present"])
        if name == "B":
            assert 0 < d["new_unique_bytes"] and not d["present"].all() and len(d["unreferenced"]) > 0
        p = ref.plan(A, X)
        empty = dataclasses.replace(X, blob=np.zeros(0, np.uint8))
        assert ref.apply(A, empty, X.blob.size, p["src"], p["literals"], p["delta_hdrs"]).to_bytes() == X.to_bytes()
    cls = ref.plan(A, B)["class"]
    assert cls.count("absent") > 0 and cls.count("same") > 0
    assert (B.chunk_map["kind"] == KIND_DELTA).any() and (B.chunk_map["kind"] == KIND_POINTER).any()
    assert (A.chunk_map["kind"] == KIND_DELTA).any() and (A.chunk_map["kind"] == KIND_POINTER).any()
    p2 = ref.plan(A, B2)
    differs = [i for i, c in enumerate(p2["class"]) if c == "differs"]
    assert differs and (p2["src"][differs] == -1).all()                          # digest present, stored bytes not: literals
    ha = {r["sha"]: r["kind"] for r in ref.records(A)}
    assert all(ha[r["sha"]] != r["kind"] for i, r in enumerate(ref.records(B2)) if i in differs)     # the kind differs in all of them
    q = ref.plan(A, B2, digest_only=True)
    empty = dataclasses.replace(B2, blob=np.zeros(0, np.uint8))
    assert ref.apply(A, empty, B2.blob.size, q["src"], q["literals"], q["delta_hdrs"]).to_bytes() != B2.to_bytes()
    same = ref.plan(A, A)
    assert (same["src"] >= 0).all() and same["literals"].size == 0
    none = ref.diff(A, A)
    assert none["present"].all() and none["new_bytes"] == 0 and len(none["unreferenced"]) == 0 and len(none["new_ranges"]) == 0


def test_coalesce():
    got = sync.coalesce(np.array([0, 10, 20, 40, 45, 45, 61]), np.array([10, 10, 5, 5, 0, 15, 1]))
    assert got.tolist() == [[0, 25], [40, 20], [61, 1]]
    assert sync.coalesce(np.zeros(0, np.int64), np.zeros(0, np.int64)).shape == (0, 2)


# ---- the patch ------------------------------------------------------------------------------------------------------------------------
def test_patch_round_trip_and_refusals(stores):
    p = _patch_from_ref(stores["A"], stores["B"])
    b = p.to_bytes()
    assert b[:8] == b"HMSEPTCH" and len(b) == p.nbytes and p.literal_bytes == p.literals.size > 0 and p.copied_bytes > 0
    q = sync.Patch.from_bytes(b)
    assert q.meta == p.meta and q.blob_size == p.blob_size and q.have_id == p.have_id and q.copied_bytes == p.copied_bytes
    assert np.array_equal(q.src, p.src) and np.array_equal(q.literals, p.literals) and np.array_equal(q.delta_hdrs, p.delta_hdrs)
    assert q.to_bytes() == b
    for bad in (b"HMSEPTCX" + b[8:], b[:-1], b + b"\0", b[:8] + (2).to_bytes(4, "little") + b[12:], b[:20]):
        with pytest.raises(ValueError):
            sync.Patch.from_bytes(bad)
    src = p.src.copy()
    src[np.nonzero(src >= 0)[0][0]] = -1                          # one more literal than the literal area holds
    with pytest.raises(ValueError, match="do not match"):
        sync.Patch.from_bytes(dataclasses.replace(p, src=src).to_bytes())
    empty = _patch_from_ref(stores["A"], dataclasses.replace(stores["A"], index=stores["A"].index[:0], chunk_map=stores["A"].chunk_map[:0],
                                                              pointers=stores["A"].pointers[:0], blob=np.zeros(0, np.uint8)))
    assert sync.Patch.from_bytes(empty.to_bytes()).src.size == 0


def test_have_id_binds_a_patch_to_its_store(stores):
    from hmse_amd import manifest
    A, B = stores["A"], stores["B"]
    assert sync.have_id(A) == sync.have_id(manifest.Manifest.from_bytes(A.to_bytes())) != sync.have_id(B)
    assert sync.have_id(manifest.Store([A])) == sync.have_id(A) and len(sync.have_id(A)) == 32
    idx = A.index.copy()
    idx["refcount"][0] ^= 1
    assert sync.have_id(dataclasses.replace(A, index=idx)) != sync.have_id(A)
    with pytest.raises(ValueError, match="another store"):       # refused on the host, in front of every device call
        sync.apply_patch(B, _patch_from_ref(A, B), torch.device("cpu"))


def test_make_patch_refuses_what_a_patch_cannot_describe(stores):
    from hmse_amd import manifest
    A = stores["A"]
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="2 shards"):
        sync.make_patch(A, manifest.Store([A, A]), cpu)
    rb = np.zeros(1, manifest.REMOTE_BASE_DTYPE)
    with pytest.raises(ValueError, match="other shards"):
        sync.make_patch(A, dataclasses.replace(A, remote_bases=rb), cpu)
    with pytest.raises(ValueError, match="Manifest or a Store"):
        sync.make_patch(A, b"bytes", cpu)
    idx = A.index.copy()
    idx["sha256"] = 0
    with pytest.raises(ValueError, match="without L3"):
        sync.make_patch(A, dataclasses.replace(A, index=idx), cpu)


def test_tiling_check_refuses_gap_overlap_and_non_zero_padding(stores):
    B = stores["B"]
    kind = sync.slot_kinds(B)
    order = sync.check_tiling(B.lba_unit, B.index, kind, B.blob.size, B.blob)
    assert np.array_equal(order, np.arange(len(B.index))) and B.lba_unit == 1
    P = ref.relay(B, 512)
    assert np.array_equal(sync.check_tiling(512, P.index, kind, P.blob.size, P.blob), np.arange(len(P.index))) and P.blob.size > B.blob.size
    with pytest.raises(ValueError, match="gap"):                 # unit 1: a blob one byte longer than its records
        sync.check_tiling(1, B.index, kind, B.blob.size + 1, np.concatenate([B.blob, [0]]).astype(np.uint8))
    idx = P.index.copy()
    idx["lba"][3:] += 1
    with pytest.raises(ValueError, match="gap"):                 # a whole unit between two records is no padding
        sync.check_tiling(512, idx, kind, P.blob.size + 512, None)
    idx = B.index.copy()
    idx["length"][2] += 1
    with pytest.raises(ValueError, match="overlap"):
        sync.check_tiling(1, idx, kind, B.blob.size, B.blob)
    with pytest.raises(ValueError, match="overlap"):             # the last record ends past the blob
        sync.check_tiling(1, B.index, kind, B.blob.size - 1, None)
    idx = B.index.copy()
    idx["lba"] += 1
    with pytest.raises(ValueError, match="gap"):                 # the first record does not start at byte 0
        sync.check_tiling(1, idx, kind, B.blob.size + 1, None)
    off, ln = P.index["lba"].astype(np.int64) * 512, P.index["length"].astype(np.int64)
    k = int(np.nonzero((off + ln) % 512)[0][0])                  # a record with padding behind it
    for at in (int(off[k] + ln[k]), int(off[k + 1]) - 1, P.blob.size - 1):
        blob = P.blob.copy()
        blob[at] = 1
        with pytest.raises(ValueError, match="non-zero padding"):
            sync.check_tiling(512, P.index, kind, blob.size, blob)
    short = B.index.copy()
    d = int(np.nonzero(kind == 2)[0][0])
    short["length"][d] = 7
    with pytest.raises(ValueError, match="shorter than"):
        sync.check_tiling(1, short, kind, B.blob.size, None)


def test_piece_table_of_the_numpy_planner_reproduces_want(stores):
    """plan_pieces over the reference's plan, applied by the reference's gather (slices): want.to_bytes(), for both pairs, for a store
    with padding (lba_unit 512), for an empty have (all literals) and an empty want."""
    from hmse_amd import manifest
    A = stores["A"]
    none = dataclasses.replace(A, index=A.index[:0], chunk_map=A.chunk_map[:0], pointers=A.pointers[:0], blob=np.zeros(0, np.uint8))
    two = manifest.Store([dataclasses.replace(stores["B2"], n_shards=2), dataclasses.replace(A, shard=1, n_shards=2)])     # blobs concatenate in shard order
    for have, want in ((A, stores["B"]), (A, stores["B2"]), (A, ref.relay(stores["B"], 512)), (ref.relay(A, 512), stores["B"]),
                       (none, stores["B"]), (A, none), (two, stores["B"]), (A, A)):
        p = _patch_from_ref(have, want)
        m = manifest.Manifest.from_bytes(p.meta)
        cat = np.concatenate([s.blob for s in ref.shards_of(have)])
        src_off, src_sel, dst_off, (hb, lb, zb) = sync.plan_pieces(m.lba_unit, m.index, sync.slot_kinds(m), p.blob_size, p.src, cat.size)
        assert hb == p.delta_hdrs.size and lb == p.literals.size and zb < m.lba_unit and (np.diff(dst_off) > 0).all()
        second = np.concatenate([p.delta_hdrs.reshape(-1), p.literals, np.zeros(zb, np.uint8)])
        blob = ref.gather(cat, second, src_off, src_sel, dst_off)
        assert dataclasses.replace(m, blob=blob).to_bytes() == want.to_bytes()
        assert manifest.reconstruct(dataclasses.replace(m, blob=blob)) == manifest.reconstruct(want)
    p = _patch_from_ref(A, stores["B"])
    m = manifest.Manifest.from_bytes(p.meta)
    src = p.src.copy()
    src[np.nonzero(src >= 0)[0][-1]] = A.blob.size - 1
    with pytest.raises(ValueError, match="outside the store"):
        sync.plan_pieces(m.lba_unit, m.index, sync.slot_kinds(m), p.blob_size, src, A.blob.size)
    with pytest.raises(ValueError, match="source table"):
        sync.plan_pieces(m.lba_unit, m.index, sync.slot_kinds(m), p.blob_size, p.src[:-1], A.blob.size)


# ---- the wrapper and the entry point --------------------------------------------------------------------------------------------------
def test_ops_sync_match_refuses_host_tensors():
    from hmse_amd import ops
    u8, i64, i32 = (lambda *v: torch.tensor(v, dtype=torch.uint8)), (lambda *v: torch.tensor(v, dtype=torch.int64)), (lambda *v: torch.tensor(v, dtype=torch.int32))
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.sync_match(u8(1, 2), i64(0), i32(2), u8(1, 2), i64(0), i32(2), i64(0))


def test_entry_point_refuses_null_arrays_with_no_gpu_present():
    """HMSE_EINVAL (-1), never HMSE_EHIP (-3): refused in front of every clear and launch.  (The pointers are host addresses; nothing may
    touch them.)"""
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr()
    ok = [b, 100, b, b, 4, b, 100, b, b, 4, b, b, b, None]
    for null in (2, 3, 10, 11, 12, 0, 5, 7, 8):                   # a_off, a_len, cand, same, status, a, b, b_off, b_len
        args = list(ok)
        args[null] = None
        assert lib.hmse_sync_match(*args) == -1, null
    assert lib.hmse_sync_match(*(ok[:4] + [1 << 33] + ok[5:])) == -1
    assert lib.hmse_sync_match(None, 0, None, None, 0, None, 0, None, None, 0, None, None, None, None) == -1      # n = 0 still needs the status word
    assert mem.sum().item() == 0


def test_symbol_is_exported_declared_and_takes_no_workspace():
    from hmse_amd import IngestConfig, _lib, ops
    assert "hmse_sync_match" in _lib.EXPORTED_SYMBOLS
    lib = _lib.hip_lib()
    assert lib.hmse_sync_match.restype is C.c_int and len(lib.hmse_sync_match.argtypes) == 14
    hdr = open(os.path.join(ROOT, "include", "hmse.h")).read()
    decl = re.search(r"int hmse_sync_match\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == 14
    assert int(re.search(r"HMSE_STAGE_SYNC_MATCH\s*=\s*(\d+)", hdr).group(1)) == ops.STAGE_SYNC_MATCH
    assert [int(v) for v in re.findall(r"HMSE_STAGE_\w+\s*=\s*(\d+)", hdr)].count(ops.STAGE_SYNC_MATCH) == 1
    assert ops.workspace_bytes(ops.STAGE_SYNC_MATCH, 1000, IngestConfig()) == 0
    assert lib.hmse_abi_version() == 3


def test_match_kernel_source_on_cpu_threads_equals_memcmp():
    """tools/sync_emu.py: the kernel's source compiled for the host as a stand-alone program, against memcmp on random tables."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sync_emu.py"), "--iters", "25", "--seed", "3"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
