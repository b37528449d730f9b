"""GPU: global L4 of a multi-rank stream as hipGraph-captured phases (hmse_amd/stream_gl4.py; VERDICT r3 item 6, SURVEY.md §8f-3,
BASELINE configs[4]).  Bar: every rank's records, put in global stored order, are bit-identical to ONE pass of the oracle over the
logical stream — the same check the eager implementation (stream_dist.GlobalL4StreamIngest) passes — with every phase replayed from
a hipGraph; with one rank the captured chain equals one-shot ingest, also with the RCCL collectives between the replays."""
from dataclasses import asdict

import numpy as np
import pytest

from test_gpu_stream_dist import NAMES, _dataset, oracle_whole_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ranks_equal_the_oracle(res, want):
    """Every rank's records, put in global stored order, against ONE pass of the oracle over the logical stream.  -> (records with a
    dictionary on another rank, of these: on a later-numbered rank)."""
    n_global = len(want["cuts"]) - 1
    assert all(r.n_global == n_global for r in res)
    U = len(want["uniq"])
    assert sorted(np.concatenate([r.ug.cpu().numpy() for r in res]).tolist()) == list(range(U))
    n_remote = n_later = 0
    for rank, r in enumerate(res):
        g = r.gidx.cpu().numpy()
        c = r.cuts.cpu().numpy().astype(np.int64)
        gl = np.diff(want["cuts"].astype(np.int64))
        assert np.array_equal(np.diff(c), gl[g])
        assert np.array_equal(r.first_occ.cpu().numpy().astype(np.uint64), want["first_occ"][g])
        assert np.array_equal(r.refcount.cpu().numpy().astype(want["refcount"].dtype), want["refcount"][g])
        assert np.array_equal(r.digests.cpu().numpy(), want["digests"][g])
        ug = r.ug.cpu().numpy()
        assert np.array_equal(g[r.uniq_ids.cpu().numpy()].astype(np.uint64), want["uniq"][ug])
        assert np.array_equal(r.sig.cpu().numpy().view(np.uint32), want["sig"][ug])
        assert np.array_equal(r.band_keys.cpu().numpy().view(np.uint32), want["keys"][ug])
        assert np.array_equal(r.base_global.cpu().numpy(), want["base"][ug].astype(np.int64))
        assert np.array_equal(r.kind.cpu().numpy(), want["kind"][ug])
        so, st = r.stream_off.cpu().numpy(), r.streams.cpu().numpy()
        wo = want["off"].astype(np.int64)
        for j, u in enumerate(ug):
            assert np.array_equal(st[so[j]: so[j + 1]], want["streams"][wo[u]: wo[u + 1]]), (rank, j)
        if r.remote_bases is not None:
            n_remote += len(r.remote_bases)
            n_later += int((r.remote_bases["shard"] > rank).sum())
    return n_remote, n_later


def _reads_back(res, batches, data, cfg, world, dev):
    from hmse_amd import manifest, read, stream_dist
    back = read.reconstruct_shards(res, verify=True)
    bounds = [stream_dist.deal_batch(b.numel(), world, cfg.seg_size) for b in batches]
    for r in range(world):
        mine = np.concatenate([b.numpy()[bd[r]: bd[r + 1]] for b, bd in zip(batches, bounds)])
        assert np.array_equal(back[r].cpu().numpy(), mine), r
    sr = stream_dist.store_results(res)
    parts = [manifest.Manifest.from_bytes(manifest.build_manifest(sr[r], r, world).to_bytes()) for r in range(world)]
    store = manifest.Store.from_bytes(manifest.merge_manifests(parts).to_bytes())
    assert manifest.reconstruct(store) == data.tobytes()
    assert np.array_equal(read.read_store(store, dev).cpu().numpy(), data)


@pytest.mark.parametrize("world,graph", [(2, True), (3, True), (2, False)])
def test_captured_global_l4_stream_stores_the_bytes_of_the_one_rank_run(orc, dev, world, graph):
    import torch
    from hmse_amd import IngestConfig, manifest, read, stream_dist, stream_gl4
    cfg = IngestConfig(seg_size=1 << 20)
    data = _dataset().copy()
    B = 4 << 20
    # near-duplicates whose originals sit on a LATER-numbered rank of an earlier batch
    src = data[(2 << 20) + 300000: (2 << 20) + 300000 + 700000].copy()
    src[::1500] ^= 0x20
    data[(8 << 20) + 50000: (8 << 20) + 50000 + src.size] = src
    want = oracle_whole_stream(orc, data, cfg)
    batches = [torch.from_numpy(data[a: a + B].copy()) for a in range(0, data.size, B)]
    res = stream_gl4.stream_shards_local_gl4_graph(batches, cfg, world, dev, graph=graph)
    n_remote, n_later = _ranks_equal_the_oracle(res, want)
    assert n_remote > 10 and n_later > 5
    back = read.reconstruct_shards(res, verify=True)
    bounds = [stream_dist.deal_batch(b.numel(), world, cfg.seg_size) for b in batches]
    for r in range(world):
        mine = np.concatenate([b.numpy()[bd[r]: bd[r + 1]] for b, bd in zip(batches, bounds)])
        assert np.array_equal(back[r].cpu().numpy(), mine), r
    sr = stream_dist.store_results(res)
    parts = [manifest.Manifest.from_bytes(manifest.build_manifest(sr[r], r, world).to_bytes()) for r in range(world)]
    store = manifest.Store.from_bytes(manifest.merge_manifests(parts).to_bytes())
    assert manifest.reconstruct(store) == data.tobytes()
    assert np.array_equal(read.read_store(store, dev).cpu().numpy(), data)


def test_one_rank_captured_global_l4_chain_equals_one_shot_ingest_also_over_rccl(dev):
    """One rank: the global numbering IS the local one, so the four captured phases must give the one-shot result; run once plainly and
    once with always_exchange on backend "nccl" (world size 1): replay A -> RCCL all-gather -> replay B1 -> RCCL all-gather -> replay B2 ->
    replay B3 per batch — what one GPU can show of the N-rank loop on RCCL itself."""
    import os
    import socket
    import torch
    import torch.distributed as dist
    from hmse_amd import IngestConfig, ingest, stream_gl4
    cfg = IngestConfig(seg_size=1 << 20)
    data = _dataset()[: 10 << 20]
    whole = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    P = 2 << 20

    def run(always):
        s = stream_gl4.GraphGlobalL4StreamIngest(cfg, data.size, P, dev, 1, 0, graph=True, always_exchange=always)
        for a in range(0, data.size, P):
            s.push(torch.from_numpy(data[a: a + P].copy()).pin_memory())
        res = s.finish()
        torch.cuda.synchronize()
        assert s._graphs.captured(P) == {"A", "B1", "B2", "B3"} and s._graphs.uses(P) == 5
        return res
    res = run(False)
    for name in NAMES:
        assert torch.equal(getattr(res, name), getattr(whole, name)), name
    assert torch.equal(res.base_global, whole.base) and torch.equal(res.ug, torch.arange(res.ug.numel(), device=dev))
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        res2 = run(True)
    finally:
        dist.destroy_process_group()
    for name in NAMES:
        assert torch.equal(getattr(res2, name), getattr(whole, name)), name


# ---------------------------------------------------------------------------------------------------------------- dense cut points
def _dense_stream(orc, cfg):
    """A logical stream of 6 MiB batches: ordinary batches around two batches that hold dense-cut pieces (tests/edge_inputs.py; facts pinned on
    the host in tests/test_edge_inputs_host.py).  Batch 1 STARTS with 2 MiB of dense cuts (text filler) and goes on with text, batch 2 starts
    with text (1 MiB of it dense, random filler) and ENDS with 2 MiB of near-duplicates of batch 1's dense chunks: with 2 ranks (3 MiB pieces)
    and with 3 (2 MiB pieces) first a low rank gets the dense piece while the others get text, then the last rank does — and finds its
    dictionaries on the low rank.  A nominal piece of it holds 993 chunks and more, all new; a signature row used to hold 576 (832)."""
    import edge_inputs as E
    G = orc.gear_table()
    ms, _ = orc.cdc_masks(orc.default_cfg(**asdict(cfg)))
    pair = E.dense_pairs(G, ms)[0]
    D = _dataset()
    A = E.dense_cut_piece(pair, 2 << 20, seed=5, text=True)
    R = E.dense_cut_piece(pair, 1 << 20, seed=6)
    M = 1 << 20
    data = np.concatenate([D[: 6 * M],
                           A, D[6 * M: 10 * M],
                           R, D[10 * M: 12 * M], D[4 * M: 5 * M], E.dense_cut_near_duplicate(A),
                           D[12 * M:]])
    return data, 6 * M


_DENSE_WANT = {}


def _dense_oracle(orc, cfg):
    if not _DENSE_WANT:
        data, B = _dense_stream(orc, cfg)
        _DENSE_WANT.update(data=data, B=B, want=oracle_whole_stream(orc, data, cfg))
    return _DENSE_WANT["data"], _DENSE_WANT["B"], _DENSE_WANT["want"]


@pytest.mark.parametrize("world,graph", [(2, True), (3, True), (2, False)])
def test_pieces_of_dense_cut_points_are_stored_like_the_one_rank_run(orc, dev, world, graph):
    """a signature row held 2 x piece / avg_size + 64 signatures while every other array of the chain is sized for piece / min_size
    chunks; a piece with more NEW stored chunks than that — legal FastCDC output — set status bit 7 and failed the whole multi-rank stream, so
    "every rank stores the records of the one-rank run" depended on the input.  The row is now sized like the digest row."""
    import torch
    from hmse_amd import IngestConfig, stream_dist, stream_gl4
    cfg = IngestConfig(seg_size=1 << 20)
    data, B, want = _dense_oracle(orc, cfg)
    batches = [torch.from_numpy(data[a: a + B].copy()) for a in range(0, data.size, B)]
    mc = data.size // cfg.min_size + 64                       # room for the dense bytes: every chunk of the stream at its smallest
    bd = stream_dist.deal_batch(B, world, cfg.seg_size)
    piece = max(b - a for a, b in zip(bd[:-1], bd[1:]))
    n_new = np.diff(np.searchsorted(want["cuts"][want["uniq"].astype(np.int64)].astype(np.int64), np.arange(0, data.size + piece, piece)))
    print(f"world {world}: nominal piece {piece} bytes, most new stored chunks in one aligned piece {int(n_new.max())}, "
          f"the former row held {2 * (piece // cfg.avg_size) + 64}")
    assert int(n_new.max()) > 2 * (piece // cfg.avg_size) + 64  # (whole pieces of the stream are aligned to the piece size at both world sizes)
    res = stream_gl4.stream_shards_local_gl4_graph(batches, cfg, world, dev, graph=graph, max_chunks=mc, max_chunks_global=mc)
    n_remote, _ = _ranks_equal_the_oracle(res, want)
    assert n_remote > 900                                      # the near-duplicates of the dense chunks found their originals on another rank
    _reads_back(res, batches, data, cfg, world, dev)


def test_one_rank_stream_of_dense_cut_pieces_equals_one_shot_ingest(orc, dev):
    """The one-rank side of the claim on the same bytes: the single-rank captured chain over the same batches == one ingest of the stream
    (== the oracle, by the test above)."""
    import torch
    from hmse_amd import IngestConfig, ingest, stream
    cfg = IngestConfig(seg_size=1 << 20)
    data, B = _dense_stream(orc, cfg)
    whole = ingest.ingest_shard(torch.from_numpy(data).to(dev), cfg)
    st = stream.StreamIngest(cfg, data.size, dev, graph=True, max_chunks=data.size // cfg.min_size + 64)
    for a in range(0, data.size, B):
        st.push(torch.from_numpy(data[a: a + B].copy()))
    r0 = st.finish()
    for name in NAMES:
        assert torch.equal(getattr(r0, name), getattr(whole, name)), name
    # dense indeed: the 2 MiB at the head of batch 1 alone hold more chunks than the former signature row of a 2 MiB piece
    c = whole.cuts.cpu().numpy().astype(np.int64)
    assert int(((c >= B) & (c < B + (2 << 20))).sum()) > 2 * ((2 << 20) // cfg.avg_size) + 64


# ---------------------------------------------------------------------------------------------------------------- real processes
GL4_NAMES = ("ug", "gidx", "base_global", "kind", "stream_off", "streams", "sig", "band_keys")
COUNTERS = (0, 1, 3, 5, 8)          # state words: bytes, chunks, stored chunks, stream bytes, chunks of all ranks


def _gl4_dataset():
    """The dataset of the lock-step test above: near-duplicates whose originals sit on a LATER-numbered rank of an earlier batch."""
    data = _dataset().copy()
    src = data[(2 << 20) + 300000: (2 << 20) + 300000 + 700000].copy()
    src[::1500] ^= 0x20
    data[(8 << 20) + 50000: (8 << 20) + 50000 + src.size] = src
    return data


def _deal(batches, world, cfg):
    from hmse_amd import stream_dist
    pieces = [[] for _ in range(world)]
    for b in batches:
        bd = stream_dist.deal_batch(b.numel(), world, cfg.seg_size)
        for r in range(world):
            pieces[r].append(b[bd[r]: bd[r + 1]].numpy().copy())
    return pieces


def _gloo_rank_gl4_graph(rank, world, port, pieces, cfg_kw, piece_bytes, kw, out_q):
    """One rank of a 2-process captured global-L4 stream on GPU 0: push -> replay A -> all-gather (gloo) -> replay B1 -> all-gather -> replay B2
    -> one host read -> four all-to-alls -> ghost -> replay B3.  Reports its result, or what finish() raised and the state it left."""
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    from hmse_amd import IngestConfig, stream_gl4
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    cfg = IngestConfig(**cfg_kw)
    s = stream_gl4.GraphGlobalL4StreamIngest(cfg, max(sum(p.size for p in pieces[rank]), 1), piece_bytes, dev, world, rank, graph=True, **kw[rank])
    for p in pieces[rank]:
        s.push(torch.from_numpy(p))
    out = {"captured": sorted(s._graphs.captured(piece_bytes)), "error": None}
    try:
        res = s.finish()
        out.update({nm: getattr(res, nm).cpu().numpy() for nm in GL4_NAMES})
        out["remote_dictionaries"] = s.remote_dictionaries
    except ValueError as e:
        out["error"] = str(e)
    torch.cuda.synchronize()
    st = s._state.tolist()
    out["state"] = st
    out.update(_cuts=s._cuts[: st[1] + 1].cpu().numpy(), _uniq=s._uniq[: st[3]].cpu().numpy(), _kind=s._kind[: st[3]].cpu().numpy(),
               _streams=s._streams[: st[5]].cpu().numpy())
    out_q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def _run_two_processes(pieces, cfg, piece_bytes, kw):
    import socket
    import torch.multiprocessing as mp
    world = 2
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_rank_gl4_graph, args=(r, world, port, pieces, asdict(cfg), piece_bytes, kw, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=300) for _ in range(world))
        for p in procs:
            p.join(timeout=120)
        codes = [p.exitcode for p in procs]
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    return got, codes


def test_captured_global_l4_stream_two_processes_over_gloo_equal_the_emulation(orc, dev):
    """The world > 1 branch of GraphGlobalL4StreamIngest._process between two REAL processes sharing this GPU (gloo): requests() ->
    ingest.fetch_chunks_routed -> write_ghost, the graphs captured at the second use of the piece size and replayed between the collectives.
    Every rank's records equal the lock-step emulation's, which equal the oracle's single pass over the stream."""
    import torch
    from hmse_amd import IngestConfig, stream_gl4
    cfg = IngestConfig(seg_size=1 << 20)
    data = _gl4_dataset()
    B, world = 4 << 20, 2
    batches = [torch.from_numpy(data[a: a + B].copy()) for a in range(0, data.size, B)]
    emu = stream_gl4.stream_shards_local_gl4_graph(batches, cfg, world, dev, graph=True)
    _ranks_equal_the_oracle(emu, oracle_whole_stream(orc, data, cfg))
    want = [{nm: getattr(r, nm).cpu().numpy() for nm in GL4_NAMES} for r in emu]
    got, codes = _run_two_processes(_deal(batches, world, cfg), cfg, 2 << 20, [{}, {}])
    assert codes == [0, 0]
    for rank in range(world):
        assert got[rank]["error"] is None, got[rank]["error"]
        assert got[rank]["captured"] == ["A", "B1", "B2", "B3"]
        for nm in GL4_NAMES:
            assert np.array_equal(got[rank][nm], want[rank][nm]), (rank, nm)
    assert sum(got[r]["remote_dictionaries"] for r in range(world)) > 5


def _ghost_needs(monkeypatch, batches, cfg, world, dev, **kw):
    """A lock-step run that records, per rank, the bytes of remote dictionaries each batch fetched.  -> (ranks, needs[rank][batch])"""
    from hmse_amd import stream_gl4
    needs = [[] for _ in range(world)]
    plain = stream_gl4.GraphGlobalL4StreamIngest.write_ghost

    def recording(self, ghost, lens):
        needs[self.rank].append(int(ghost.numel()))
        return plain(self, ghost, lens)
    with monkeypatch.context() as m:
        m.setattr(stream_gl4.GraphGlobalL4StreamIngest, "write_ghost", recording)
        ranks = stream_gl4.lockstep_gl4_graph(batches, cfg, world, dev, **kw)
    return ranks, needs


def _refusal_dataset():
    """_gl4_dataset() plus near-duplicates in batch 2's LAST piece (rank 1 of 2) of bytes of batch 0's first piece: rank 1 needs many remote
    dictionaries in a batch behind the second."""
    data = _gl4_dataset()
    src = data[300000: 300000 + 900000].copy()
    src[::1500] ^= 0x20
    data[(10 << 20) + 50000: (10 << 20) + 50000 + src.size] = src
    return data


def test_a_ghost_area_too_small_on_one_rank_fails_both_processes_at_finish_with_the_good_batches_intact(dev, monkeypatch):
    """write_ghost used to raise on the rank whose ghost area a batch's dictionaries do not fit, between two collectives — its
    peer then waited in the next batch's all-gather for ever.  Now the batch is refused through the chain (status bit 16), the rank stays
    in every collective, and finish() raises on BOTH ranks.  Rank 1's ghost area is sized, from the emulation's own fetches, so that
    batches 0 and 1 fit and a later batch does not.  Rank 1's counters are frozen at, and both ranks' arrays start with, what an
    emulation over the good batches alone gives; both ranks' counters are those of an emulation with the same small ghost area
    (rank 0 never dropped a batch: it went on, indexing chunks of the refused batch that nobody stores — why the stream fails as a whole)."""
    import torch
    from hmse_amd import IngestConfig, stream_gl4
    cfg = IngestConfig(seg_size=1 << 20)
    data = _refusal_dataset()
    B, world = 4 << 20, 2
    batches = [torch.from_numpy(data[a: a + B].copy()) for a in range(0, data.size, B)]
    _, needs = _ghost_needs(monkeypatch, batches, cfg, world, dev, graph=True)
    need = needs[1]
    print("remote dictionary bytes per batch, rank 0:", needs[0], "rank 1:", need)
    assert len(need) == len(batches) and max(need[2:]) > max(need[:2]) + 128
    ghost_bytes = max(need[:2]) + 64
    k = next(b for b in range(2, len(need)) if need[b] > ghost_bytes)       # the first batch that does not fit
    prefix = stream_gl4.lockstep_gl4_graph(batches[:k], cfg, world, dev, graph=True)
    small = stream_gl4.lockstep_gl4_graph(batches, cfg, world, dev, graph=True, rank_kw=[{}, {"ghost_bytes": ghost_bytes}])
    torch.cuda.synchronize()
    got, codes = _run_two_processes(_deal(batches, world, cfg), cfg, 2 << 20, [{}, {"ghost_bytes": ghost_bytes}])
    assert codes == [0, 0]
    for rank in range(world):
        g = got[rank]
        assert g["error"] is not None and "status" in g["error"], rank                   # finish() raised ValueError on both
        st, stp, sts = g["state"], prefix[rank]._state.tolist(), small[rank]._state.tolist()
        print(f"rank {rank}: status {st[7]:#x}, counters {[st[i] for i in COUNTERS]}, prefix run {[stp[i] for i in COUNTERS]}, "
              f"emulation with the small ghost area {[sts[i] for i in COUNTERS]} status {sts[7]:#x}")
        assert [st[i] for i in COUNTERS] == [sts[i] for i in COUNTERS] and st[7] == sts[7]
        if rank == 1:
            assert st[7] & 0x10000 and "ghost area" in g["error"]
            assert [st[i] for i in COUNTERS] == [stp[i] for i in COUNTERS]               # frozen where the last good batch left them
        p = prefix[rank]
        assert np.array_equal(g["_cuts"][: stp[1] + 1], p._cuts[: stp[1] + 1].cpu().numpy())
        assert np.array_equal(g["_uniq"][: stp[3]], p._uniq[: stp[3]].cpu().numpy())
        assert np.array_equal(g["_kind"][: stp[3]], p._kind[: stp[3]].cpu().numpy())
        assert np.array_equal(g["_streams"][: stp[5]], p._streams[: stp[5]].cpu().numpy())
    with pytest.raises(ValueError, match="status"):                                     # the emulation: finish() raises, write_ghost did not
        small[1].finish()


# ---------------------------------------------------------------------------------------------------------------- capacities, lock step
@pytest.mark.parametrize("which", ["max_chunks", "stored", "stream_capacity", "max_chunks_global", "ghost_bytes"])
def test_capacity_refusals_of_the_captured_global_l4_stream(dev, monkeypatch, which):
    """The captured class's own capacities at world 2, rank 1 refusing: the expected sticky bit on rank 1, finish() raises there, the first
    batch is intact, nothing was written behind the arrays' fill — and the stream as a whole fails (stream_shards_local_gl4_graph raises):
    rank 0, which dropped nothing, has by then indexed chunks of the refused batch that no rank stores (printed)."""
    import torch
    from hmse_amd import IngestConfig, stream_gl4
    cfg = IngestConfig(seg_size=1 << 20)
    data = _refusal_dataset()[: 12 << 20]
    B, world = 4 << 20, 2
    batches = [torch.from_numpy(data[a: a + B].copy()) for a in range(0, data.size, B)]
    first, needs = _ghost_needs(monkeypatch, batches[:1], cfg, world, dev, graph=True)
    f = first[1]
    sf = f._state.tolist()
    b1, n1, u1, s1, g1 = (sf[i] for i in COUNTERS)
    assert sf[7] == 0 and n1 > 100 and u1 > 100
    if which == "ghost_bytes":
        _, all_needs = _ghost_needs(monkeypatch, batches, cfg, world, dev, graph=True)
        print("remote dictionary bytes per batch, rank 1:", all_needs[1])
        assert all_needs[1][1] > needs[1][0] + 128                # batch 1 is the one that does not fit
    kw = {"max_chunks": dict(max_chunks=n1 + 10, max_chunks_global=4 * g1), "stored": dict(max_chunks=4 * n1), "stream_capacity": dict(stream_capacity=s1 + 1000),
          "max_chunks_global": dict(max_chunks_global=g1 + 10), "ghost_bytes": dict(ghost_bytes=needs[1][0] + 64)}[which]
    guard = {}

    def setup(ranks):
        s = ranks[1]
        if which == "stored":
            s.max_unique = u1 + 10                                  # the chain takes the bound as an argument
        s.data[s.capacity:] = 0xAB                                   # the ghost area
        for nm in ("_cuts", "_uniq", "_first_occ_g", "_refcount_g"):
            guard[nm] = getattr(s, nm).clone()
    rank_kw = [{}, kw]
    ranks = stream_gl4.lockstep_gl4_graph(batches, cfg, world, dev, graph=True, rank_kw=rank_kw, setup=setup)
    s, peer = ranks[1], ranks[0]
    st, sp = s._state.tolist(), peer._state.tolist()
    want_bit = {"max_chunks": 1, "stored": 2, "stream_capacity": 0x100, "max_chunks_global": 1, "ghost_bytes": 0x10000}[which]
    assert st[7] & want_bit, hex(st[7])
    with pytest.raises(ValueError, match="status"):
        s.finish()
    # the first batch is intact, the counters are frozen there, nothing of the failed batches was committed
    assert [st[i] for i in COUNTERS] == [b1, n1, u1, s1, g1]
    assert torch.equal(s._cuts[: n1 + 1], f._cuts[: n1 + 1]) and torch.equal(s._uniq[:u1], f._uniq[:u1])
    assert torch.equal(s._streams[:s1], f._streams[:s1]) and torch.equal(s._kind[:u1], f._kind[:u1])
    assert torch.equal(s._base_global[:u1], f._base_global[:u1]) and torch.equal(s._ug[:u1], f._ug[:u1])
    # canaries
    if which == "max_chunks":
        assert torch.equal(s._cuts[n1 + 1: s.max_chunks + 1], guard["_cuts"][n1 + 1: s.max_chunks + 1])     # not one cut of the dropped batch
    if which == "stored":
        assert torch.equal(s._uniq[s.max_unique:], guard["_uniq"][s.max_unique:])
    if which == "max_chunks_global":
        assert torch.equal(s._first_occ_g[g1:], guard["_first_occ_g"][g1:]) and torch.equal(s._refcount_g[g1:], guard["_refcount_g"][g1:])
    k0 = int(f.remote_dictionaries)
    assert s.remote_dictionaries == k0 or which != "ghost_bytes"
    if which == "ghost_bytes":
        assert bool((s.data[s.capacity + needs[1][0]:] == 0xAB).all())                                       # no byte of the refused dictionaries
        assert torch.equal(s._cuts[s.ghost_chunk0 + k0 + 1:], guard["_cuts"][s.ghost_chunk0 + k0 + 1:])      # and none of their bounds
        assert "ghost area" in s._host_error
    # the peer: it dropped nothing itself, and holds index entries for chunks of rank 1's refused batch
    print(f"{which}: rank 1 status {st[7]:#x} counters {[st[i] for i in COUNTERS]}; peer rank 0 status {sp[7]:#x} counters {[sp[i] for i in COUNTERS]}")
    assert sp[8] > st[8]                                             # the global numbering has diverged: silent in lock step without the rule below
    with pytest.raises(ValueError, match="status"):
        stream_gl4.stream_shards_local_gl4_graph(batches, cfg, world, dev, graph=True, rank_kw=rank_kw,
                                                 setup=(lambda rk: setattr(rk[1], "max_unique", u1 + 10)) if which == "stored" else None)
