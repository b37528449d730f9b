"""GPU: replication (hmse_amd.sync; hmse_sync_match) against the plain-Python reference of tests/sync_ref.py — the match kernel on
synthetic tables and on poisoned / misaligned / guarded memory (tests/arena.py), then diff, make_patch and apply_patch on stores with
FULL, DELTA and POINTER records on both sides.  All results are compared bit for bit."""
import dataclasses

import numpy as np
import pytest

import arena as A_
import sync_ref as ref
from test_sync_host import SEG, corpora

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 15, 16, 17, 63, 64, 1023, 1024, 1025, 4097, 32773)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev, dt=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return (t if dt is None else t.to(dt)).to(dev)


def run(dev, a, a_off, a_len, b, b_off, b_len, cand, place=None):
    """ops.sync_match on host inputs -> (same list, status), asserted equal to the reference."""
    import torch
    from hmse_amd import ops
    place = place or (lambda x, **kw: _t(x, dev))
    i64, i32 = (lambda v: np.asarray(v, np.int64).reshape(-1)), (lambda v: np.asarray(v, np.int32).reshape(-1))
    same, status = ops.sync_match(place(np.asarray(a, np.uint8), side="a"), place(i64(a_off)), place(i32(a_len)),
                                  place(np.asarray(b, np.uint8), side="b"), place(i64(b_off)), place(i32(b_len)), place(i64(cand)))
    assert same.dtype == torch.uint8 and same.numel() == len(cand)
    want, want_status = ref.match(a, a_off, a_len, b, b_off, b_len, cand)
    assert same.tolist() == want and status == want_status
    return want, status


# ---- the kernel on synthetic tables ---------------------------------------------------------------------------------------------------
def test_every_pair_of_misalignments_in_one_launch(dev):
    """256 record pairs of 1025 bytes, one per combination of a_off % 16 and b_off % 16: all equal, then each with one byte flipped."""
    rng = np.random.default_rng(1)
    L, pitch = 1025, 1072
    rec = rng.integers(0, 256, (256, L), dtype=np.uint8)
    a, b = rng.integers(0, 256, 256 * pitch, dtype=np.uint8), rng.integers(0, 256, 256 * pitch, dtype=np.uint8)
    k = np.arange(256)
    a_off, b_off = k * pitch + k // 16, k[::-1] * pitch + k % 16          # (b's records lie in the opposite order)
    for i in k:
        a[a_off[i]:a_off[i] + L] = rec[i]; b[b_off[i]:b_off[i] + L] = rec[i]
    assert len({(int(x) % 16, int(y) % 16) for x, y in zip(a_off, b_off)}) == 256
    same, status = run(dev, a, a_off, [L] * 256, b, b_off, [L] * 256, k)
    assert same == [1] * 256 and status == 0
    at = rng.integers(0, L, 256)
    at[:4] = (0, L - 1, 1023, 1024)
    a[a_off + at] ^= rng.integers(1, 256, 256, dtype=np.uint8)
    same, status = run(dev, a, a_off, [L] * 256, b, b_off, [L] * 256, k)
    assert same == [0] * 256 and status == 0


@pytest.mark.parametrize("mis", [(0, 0), (5, 11)])
def test_lengths_and_planted_differences(dev, mis):
    """Every length equal, then with a difference at byte 0, at byte len - 1, and at bytes 1023 and 1024 (the trip boundary; with a
    misaligned start also at the boundary of the first full trip behind the head)."""
    rng = np.random.default_rng(2)
    b_parts, b_off, b_len, pos = [], [], [], mis[1]
    for L in LENGTHS:
        b_parts.append(rng.integers(0, 256, pos - sum(len(p) for p in b_parts), dtype=np.uint8))
        b_off.append(pos); b_len.append(L)
        b_parts.append(rng.integers(0, 256, L, dtype=np.uint8))
        pos += L + 16 + int(rng.integers(0, 16))
    b = np.concatenate(b_parts)
    a_parts, a_off, a_len, cand, expect, pos = [np.zeros(mis[0], np.uint8)], [], [], [], [], mis[0]
    for j, L in enumerate(LENGTHS):
        for v in range(7):
            head = (16 - pos % 16) % 16                              # (tensors start 256-byte aligned)
            at = (None, 0, L - 1, 1023, 1024, head + 1023, head + 1024)[v]
            if at is not None and not 0 <= at < L:
                continue
            r = b[b_off[j]:b_off[j] + L].copy()
            if at is not None:
                r[at] ^= 0x40
            a_off.append(pos); a_len.append(L); cand.append(j); expect.append(int(at is None))
            a_parts.append(r); pos += L
    a = np.concatenate(a_parts)
    same, status = run(dev, a, a_off, a_len, b, b_off, b_len, cand)
    assert same == expect and status == 0 and sum(expect) == len(LENGTHS)


def test_candidates_lengths_and_bounds(dev):
    rng = np.random.default_rng(3)
    b = rng.integers(0, 256, 5000, dtype=np.uint8)
    a = b.copy()
    b_off, b_len = [0, 100, 2100, 4000], [100, 2000, 1900, 1000]           # b's last record ends at b_bytes
    # no candidate; candidate = n_b and beyond: status bit 0, same 0
    assert run(dev, a, [0, 0], [100, 100], b, b_off, b_len, [-1, -7]) == ([0, 0], 0)
    assert run(dev, a, [0, 0, 100], [100, 100, 2000], b, b_off, b_len, [0, 4, 1]) == ([1, 0, 1], 1)
    assert run(dev, a, [0], [100], b, b_off, b_len, [1 << 40]) == ([0], 1)
    # unequal lengths: 0 without a status bit (also when the shorter one is a prefix of the longer)
    assert run(dev, a, [100, 100, 0], [1999, 2000, 0], b, b_off, b_len, [1, 1, 0]) == ([0, 1, 0], 0)
    # a record that ends past a_bytes / b_bytes, an offset past the blob, a length near 2^32: status bit 0, the others still answered
    assert run(dev, a, [4000, 4000, 0], [1000, 1001, 100], b, b_off, b_len, [3, 3, 0]) == ([1, 0, 1], 1)
    assert run(dev, a, [5001, 0], [0, 100], b, b_off, b_len, [0, 0]) == ([0, 1], 1)
    assert run(dev, a, [16, 0], [-16, 100], b, b_off, b_len, [0, 0]) == ([0, 1], 1)
    assert run(dev, a, [4000, 0], [1000, 100], b, b_off, [100, 2000, 1900, 1001], [3, 0]) == ([0, 1], 1)
    assert run(dev, a, [4000], [1000], b, [0, 100, 2100, -8], b_len, [3]) == ([0], 1)
    # n = 0; n_b = 0 (every candidate is out of range); empty blobs with empty records
    assert run(dev, a, [], [], b, b_off, b_len, []) == ([], 0)
    assert run(dev, a, [0, 0], [100, 0], b, [], [], [0, -1]) == ([0, 0], 1)
    assert run(dev, [], [0, 0], [0, 0], [], [0], [0], [0, -1]) == ([1, 0], 0)
    assert run(dev, [], [0], [1], [], [0], [1], [0]) == ([0], 1)


@pytest.mark.parametrize("pattern", ["random", "ones", "zero"])
def test_match_on_poisoned_misaligned_guarded_memory(dev, monkeypatch, pattern):
    """Blobs at byte misalignments whose last records end exactly at the guarded end, outputs from poisoned memory: `same` is fully
    determined for every k — the refused records included — and no guard band is touched."""
    rng = np.random.default_rng(4)
    ar = A_.Arena(dev, pattern, seed=9).install(monkeypatch, distrust_zeros=True, byte_misalign=3)
    b = rng.integers(0, 256, 7000, dtype=np.uint8)
    b_off, b_len = [0, 17, 1042, 3091, 6999 - 1500], [17, 1025, 2049, 1030, 1501]               # the last one ends at b_bytes
    recs = [b[o:o + l].copy() for o, l in zip(b_off, b_len)]
    recs[2][2048] ^= 1                                                                            # the last byte differs
    a = np.concatenate([rng.integers(0, 256, 9, dtype=np.uint8)] + recs)
    a_off = (9 + np.concatenate([[0], np.cumsum(b_len)[:-1]])).tolist()                           # a's last record ends at a_bytes
    assert a_off[-1] + b_len[-1] == a.size
    mis = {"a": 5, "b": 11}
    place = lambda x, side=None: ar.place(x, misalign=mis.get(side, 0))
    # five copies (one with a differing last byte), then: one that ends one byte past a_bytes, no candidate, candidate = n_b, lengths
    # differ, the first copy again
    a_off2, a_len2 = a_off + [a_off[-1]] + [a_off[0]] * 4, b_len + [b_len[-1] + 1, 17, 17, 17, 17]
    cand = [0, 1, 2, 3, 4, 4, -1, 5, 1, 0]
    same, status = run(dev, a, a_off2, a_len2, b, b_off, b_len, cand, place=place)
    assert same == [1, 1, 0, 1, 1, 0, 0, 0, 0, 1] and status == 1
    ar.check()


# ---- stores ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg():
    from hmse_amd import IngestConfig
    return IngestConfig(seg_size=SEG)


@pytest.fixture(scope="module")
def data():
    return corpora()


@pytest.fixture(scope="module")
def stores(dev, cfg, data):
    import torch
    from hmse_amd import ingest, manifest
    out = {k: manifest.Manifest.from_bytes(manifest.build_manifest(ingest.ingest_shard(torch.from_numpy(d).to(dev), cfg)).to_bytes())
           for k, d in data.items()}
    A = out["A"]
    out["none"] = dataclasses.replace(A, index=A.index[:0], chunk_map=A.chunk_map[:0], pointers=A.pointers[:0], blob=np.zeros(0, np.uint8))
    return out


def _same_diff(got, want):
    assert np.array_equal(got.present, want["present"]) and got.present.dtype == np.bool_
    assert np.array_equal(got.new_ranges, want["new_ranges"]) and np.array_equal(got.unreferenced, want["unreferenced"])
    assert got.unreferenced.dtype == np.int64
    assert (got.shared_bytes, got.new_bytes, got.new_unique_bytes) == (want["shared_bytes"], want["new_bytes"], want["new_unique_bytes"])


def _round_trip(have, want, corpus, dev):
    """make_patch / apply_patch against the reference: the plan bit for bit, the result byte for byte, the corpus read back; the
    serialised patch applies the same way.  Returns (patch, the reference's record classes)."""
    from hmse_amd import read, sync
    p = sync.make_patch(have, want, dev)
    r = ref.plan(have, want)
    assert np.array_equal(p.src, r["src"]) and np.array_equal(p.literals, r["literals"]) and np.array_equal(p.delta_hdrs, r["delta_hdrs"])
    assert p.literal_bytes == r["literals"].size and p.nbytes == len(p.to_bytes())
    assert p.copied_bytes == sum(len(x["stream"]) for x, s in zip(ref.records(want), r["src"]) if s >= 0)
    out = sync.apply_patch(have, p, dev)
    assert out.to_bytes() == want.to_bytes()
    if len(want.chunk_map):
        assert np.array_equal(read.read_manifest(out, dev).cpu().numpy(), corpus)
    again = sync.apply_patch(have, sync.Patch.from_bytes(p.to_bytes()), dev, verify=False)
    assert again.to_bytes() == want.to_bytes()
    return p, r["class"]


def test_diff_patch_apply_with_every_class_of_record(dev, stores, data):
    """A = [S0, S1, V0, S2, V2, S1] -> B = [S0, S1, V1, V0, S3, V2, S0, S5[:30000]]: absent and byte-identical records, DELTA and POINTER
    records on both sides."""
    from hmse_amd import sync
    from hmse_amd.config import KIND_DELTA, KIND_POINTER
    A, B = stores["A"], stores["B"]
    for m in (A, B):
        assert (m.chunk_map["kind"] == KIND_DELTA).any() and (m.chunk_map["kind"] == KIND_POINTER).any()
    _same_diff(sync.diff(A, B, dev), ref.diff(A, B))
    p, cls = _round_trip(A, B, data["B"], dev)
    assert cls.count("absent") > 0 and cls.count("same") > 0
    assert int((p.src < 0).sum()) == cls.count("absent") + cls.count("differs") and int((p.src >= 0).sum()) == cls.count("same")
    assert 0 < p.nbytes < len(B.to_bytes())


def test_equal_digests_with_different_stored_bytes_are_literals(dev, stores, data):
    """A -> B2 = [V0, S0, V2, S1]: every chunk of B2 is in A, but some records are FULL in one store and DELTA in the other.  Their
    digests join; hmse_sync_match says their streams differ; they travel as literals.  A plan that copies on digest equality alone
    would NOT reproduce B2 (shown with the reference's apply)."""
    from hmse_amd import sync
    A, B2 = stores["A"], stores["B2"]
    d = sync.diff(A, B2, dev)
    _same_diff(d, ref.diff(A, B2))
    assert d.present.all() and d.new_bytes == 0
    p, cls = _round_trip(A, B2, data["B2"], dev)
    differs = [i for i, c in enumerate(cls) if c == "differs"]
    assert len(differs) >= 1 and (p.src[differs] == -1).all() and p.literal_bytes > 0
    q = ref.plan(A, B2, digest_only=True)
    empty = dataclasses.replace(B2, blob=np.zeros(0, np.uint8))
    assert ref.apply(A, empty, B2.blob.size, q["src"], q["literals"], q["delta_hdrs"]).to_bytes() != B2.to_bytes()


def test_patch_of_a_store_onto_itself_has_no_literals(dev, stores, data):
    from hmse_amd import sync
    A = stores["A"]
    p, cls = _round_trip(A, A, data["A"], dev)
    assert p.literal_bytes == 0 and set(cls) == {"same"} and p.copied_bytes > 0
    d = sync.diff(A, A, dev)
    _same_diff(d, ref.diff(A, A))
    assert d.present.all() and len(d.unreferenced) == 0 and len(d.new_ranges) == 0


def test_empty_have_and_empty_want(dev, stores, data):
    from hmse_amd import sync
    B, none = stores["B"], stores["none"]
    p, cls = _round_trip(none, B, data["B"], dev)
    assert set(cls) == {"absent"} and (p.src == -1).all() and p.copied_bytes == 0
    _same_diff(sync.diff(none, B, dev), ref.diff(none, B))
    p, cls = _round_trip(B, none, np.zeros(0, np.uint8), dev)
    assert cls == [] and p.literal_bytes == 0 and p.blob_size == 0
    d = sync.diff(B, none, dev)
    _same_diff(d, ref.diff(B, none))
    assert len(d.unreferenced) == len(B.index)


def test_have_as_a_two_shard_merged_store(dev, cfg, stores, data):
    """have = A's corpus ingested as two shards and merged: byte positions count through the shards' blobs in shard order."""
    import torch
    from hmse_amd import ingest, manifest, sync
    half = 3 * SEG
    rs = ingest.ingest_shards_local([torch.from_numpy(data["A"][:half].copy()).to(dev), torch.from_numpy(data["A"][half:].copy()).to(dev)], cfg)
    have = manifest.Store.from_bytes(manifest.merge_manifests([manifest.build_manifest(r, i, 2) for i, r in enumerate(rs)]).to_bytes())
    assert len(have.shards) == 2 and all(len(m.index) for m in have.shards)
    B = stores["B"]
    _same_diff(sync.diff(have, B, dev), ref.diff(have, B))
    _round_trip(have, B, data["B"], dev)
    p, cls = _round_trip(have, stores["A"], data["A"], dev)            # the same corpus as one shard: S2's records sit in shard 1
    assert (p.src >= have.shards[0].blob.size).any() and ((p.src >= 0) & (p.src < have.shards[0].blob.size)).any()       # copies from both shards
    _same_diff(sync.diff(B, have, dev), ref.diff(B, have))                                                             # a two-shard want can be compared
    with pytest.raises(ValueError, match="2 shards"):
        sync.make_patch(B, have, dev)


def test_want_with_padding_at_lba_unit_512(dev, stores, data):
    from hmse_amd import sync
    A, P = stores["A"], ref.relay(stores["B"], 512)
    assert P.lba_unit == 512 and P.blob.size > stores["B"].blob.size
    p, _ = _round_trip(A, P, data["B"], dev)
    assert (p.src >= 0).any() and (p.src < 0).any()
    _round_trip(ref.relay(A, 512), P, data["B"], dev)                  # both sides padded
    _same_diff(sync.diff(A, P, dev), ref.diff(A, P))
    bad = P.blob.copy()
    off, ln = P.index["lba"].astype(np.int64) * 512, P.index["length"].astype(np.int64)
    bad[int((off + ln)[np.nonzero((off + ln) % 512)[0][0]])] = 7
    with pytest.raises(ValueError, match="non-zero padding"):
        sync.make_patch(A, dataclasses.replace(P, blob=bad), dev)


def test_wrong_or_damaged_have_is_refused(dev, stores):
    from hmse_amd import read, sync
    A, B = stores["A"], stores["B"]
    p = sync.make_patch(A, B, dev)
    with pytest.raises(ValueError, match="another store"):
        sync.apply_patch(stores["B2"], p, dev)
    lens = np.array([len(r["stream"]) if s >= 0 else 0 for r, s in zip(ref.records(B), p.src)])
    k = int(np.argmax(lens))                                           # the longest copied stream: one byte of it flipped in have
    blob = A.blob.copy()
    blob[int(p.src[k]) + lens[k] // 2] ^= 0x10
    damaged = dataclasses.replace(A, blob=blob)
    with pytest.raises(read.ReadError):
        sync.apply_patch(damaged, p, dev, verify=True)
    assert sync.apply_patch(damaged, p, dev, verify=False).to_bytes() != B.to_bytes()    # what verify=True keeps from passing silently


def test_stores_without_digests_are_refused(dev, stores):
    from hmse_amd import sync
    A, B = stores["A"], stores["B"]
    idx = A.index.copy()
    idx["sha256"] = 0
    for have, want in ((dataclasses.replace(A, index=idx), B), (B, dataclasses.replace(A, index=idx))):
        with pytest.raises(ValueError, match="without L3"):
            sync.diff(have, want, dev)
        with pytest.raises(ValueError, match="without L3"):
            sync.make_patch(have, want, dev)
