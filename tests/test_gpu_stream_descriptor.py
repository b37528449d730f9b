"""GPU: the stream descriptor (include/hmse.h: hmse_stream) at the boundary — every streaming entry point refuses a descriptor that misses
a field it requires, is of another size or names a rank outside its world, before it enqueues anything; the intact descriptor then runs."""
import ctypes as C
from types import SimpleNamespace

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
ALL = ("state", "cuts", "digests", "first_occ", "refcount", "l3_table", "uniq", "sig", "band_keys", "base", "lsh_tables", "kind", "stream_off", "out")
REQUIRED = {                                  # (gidx: only with several ranks — this stream has one and leaves it NULL)
    "hash": ("state", "cuts"),
    "encode": ALL,
    "batch": ALL,
    "sign": ("state", "cuts", "digests", "first_occ", "refcount", "l3_table", "uniq", "sig"),
    "bases": ("state", "uniq", "band_keys", "base"),
    "encode_g": ("state", "cuts", "kind", "stream_off", "out"),
}


def test_a_broken_descriptor_is_refused_before_anything_is_enqueued_and_the_intact_one_runs():
    import torch
    from hmse_amd import IngestConfig, _lib, corpus, ingest, ops, stream
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    cfg = IngestConfig(seg_size=MIB)
    data = corpus.wiki_synth(3 * MIB, seed=23)
    s = stream.StreamIngest(cfg, data.size, dev, graph=True, stream_capacity=4 * MIB)
    arrays = s._stream_arrays()
    assert set(ALL) == set(arrays.tensors) and arrays.c.world == 1 and arrays.c.gidx is None
    assert set(ALL) | {"gidx"} == {n for n, t in _lib.HmseStream._fields_ if t is C.c_void_p}

    # what changes per call: real buffers of the right sizes, so that only the descriptor can be what a call is refused for
    z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device=dev)
    seg_off, ws = ops.segment_offsets(MIB, cfg.seg_size, dev), ops.stream_workspace(MIB, cfg, dev)
    row, sig_row = z(ops.stream_row_bytes(MIB, cfg)), z(ops.stream_sig_row_bytes(MIB, cfg))
    mg, sig_cap = 64, ops.stream_sig_cap(MIB, cfg)
    g_arrays = dict(gstate=z(16, torch.int64), sig_g=z((mg, cfg.n_hashes), torch.int32), band_keys_g=z((mg, cfg.bands), torch.int32), base_g=z(mg, torch.int64),
                    lsh_tables_g=z((cfg.bands, ops.l4_lsh_slots(mg)), torch.int32), g_owner=z(mg, torch.int32), g_local=z(mg, torch.int64),
                    ug=z(s.max_unique, torch.int64), base_global=z(s.max_unique, torch.int64), req_counts=z(1 + 2, torch.int64), req_slots=z(sig_cap, torch.int64))
    gl4 = _lib.HmseGl4(struct_size=C.sizeof(_lib.HmseGl4), world=1, rank=0, sig_cap=sig_cap, max_stored_g=mg, lsh_slots_g=g_arrays["lsh_tables_g"].shape[1],
                       ghost_chunk0=s.max_chunks + 1, **{k: t.data_ptr() for k, t in g_arrays.items()})
    calls = {
        "hash": lambda d: ops.stream_piece_hash(s.data, MIB, MIB, seg_off, cfg, d, row, ws),
        "encode": lambda d: ops.stream_piece_encode(s.data, MIB, MIB, cfg, d, row, ws),
        "batch": lambda d: ops.stream_batch(s.data, MIB, seg_off, cfg, d, ws),
        "sign": lambda d: ops.stream_piece_sign(s.data, MIB, MIB, cfg, d, row, sig_row, ws),
        "bases": lambda d: ops.stream_piece_bases(MIB, cfg, d, sig_row, gl4, ws),
        "encode_g": lambda d: ops.stream_piece_encode_g(s.data, MIB, MIB, cfg, d, g_arrays["gstate"], ws),
    }
    assert set(calls) == set(REQUIRED)

    def broken(**fields):
        c = _lib.HmseStream.from_buffer_copy(arrays.c)
        for k, v in fields.items():
            setattr(c, k, v)
        return SimpleNamespace(c=c)

    torch.cuda.synchronize()
    watched = {**arrays.tensors, **g_arrays, "row": row, "sig_row": sig_row, "ws": ws}
    before = {k: t.clone() for k, t in watched.items()}
    n_refused = 0
    for name, call in calls.items():
        for d, what in [(broken(**{f: None}), f) for f in REQUIRED[name]] + [(broken(struct_size=C.sizeof(_lib.HmseStream) - 8), "struct_size"),
                                                                              (broken(rank=1), "rank == world")]:
            with pytest.raises(ops.HmseError) as ei:
                call(d)
            assert ei.value.code == -1, (name, what)
            n_refused += 1
    assert n_refused == sum(len(v) + 2 for v in REQUIRED.values()) == 59
    torch.cuda.synchronize()
    for k, t in watched.items():
        assert torch.equal(t, before[k]), k            # the state block and every array: nothing was enqueued

    # the refusals did not disturb the stream: three batches through the intact descriptor == the one-shot ingest
    whole = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    for a in range(0, data.size, MIB):
        s.push(torch.from_numpy(data[a: a + MIB].copy()))
    res = s.finish()
    assert s._stream_arrays() is arrays
    for name in ("cuts", "digests", "first_occ", "refcount", "uniq_ids", "sig", "band_keys", "base", "kind", "stream_off", "streams"):
        assert torch.equal(getattr(res, name), getattr(whole, name)), name
    assert res.stats == whole.stats
