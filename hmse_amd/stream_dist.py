"""Multi-GPU streaming (BASELINE.json configs[4]: "4 x 10 GB mixed corpora streamed, 8 x MI355X, hipGraph-captured per-batch
pipeline"; the reference's batch loop README.md:1519-1580 against ONE index, one process per GPU).

Definition.  The stream arrives as GLOBAL BATCHES.  A batch is dealt to the ranks as contiguous runs of whole segments
("pieces": rank 0 gets the first run, rank 1 the next, ...), so the concatenation of the pieces in (batch, rank) order IS the
logical stream, and the global chunk order is (batch, rank, local index) — the natural order of that stream.  Per batch:

  phase A   every rank: L2 FastCDC + L3 SHA-256 of ITS piece -> its exchange row {count, digests}       hmse_stream_piece_hash
  exchange  ONE all-gather of the rows (fixed-size rows: no count round trip, capturable)                RCCL over xGMI
  phase B   every rank: rows -> the global digest array in (batch, rank, local) order -> the same persistent L3 table on every
            rank (order-independent first occurrences, hmse_l3_index_update's rule) -> ITS stored chunks -> L4 MinHash +
            ITS persistent band tables -> L1 dictionary DEFLATE -> index tails, state advanced           hmse_stream_piece_encode

Dedupe is therefore GLOBAL over the stream so far (a chunk is stored by the rank that holds its first occurrence in stream
order); L4 bases and dictionaries are scoped to the rank (the dictionary bytes must be resident), exactly as in the sharded
one-shot ingest (ingest.ingest_shard(distributed=True)) — which is the one-batch special case of this definition.  No host
read happens between the stages; with graph=True phase A and phase B of a piece size are captured into two hipGraphs at their
second use and replayed from then on (the collective stays an ordinary stream-ordered RCCL call between the two replays).

tests/ and ingest-on-one-GPU emulations drive several ranks in lock step inside one process, without collectives
(stream_shards_local; stream_common.RankStream.lockstep).  The oracle of this definition is tests/test_gpu_stream_dist.py::oracle_stream_pipeline.
"""
from __future__ import annotations

import os

import torch

from . import ops
from .config import IngestConfig
from .ingest import ShardResult
from .stream_common import all_gather_rows, deal_batch  # noqa: F401  (part of this module's surface: tests/ and tools/ call them here)
from .stream_common import (SB_G_OLD, SB_N_OLD, SB_OFF, SB_S_OLD, SB_U_OLD, CapturedRankStream, RankStream, deflate_ws_bytes, lockstep_ranks, max_stored,
                            remote_base_rows, serve_chunks, serve_requests)

_DEBUG_SYNC = os.environ.get("HMSE_STREAM_DEBUG_SYNC") == "1"


class DistStreamIngest(CapturedRankStream):
    """This rank's side of a stream sharded over `world` ranks.  Every rank pushes ITS piece of every global batch, in the
    same order (a rank with no bytes in a batch pushes an empty tensor) — the per-batch exchange is a collective."""

    def __init__(self, cfg: IngestConfig, capacity_bytes: int, piece_bytes: int, device, world: int, rank: int,
                 max_chunks_global: int | None = None, max_chunks: int | None = None, stream_capacity: int | None = None,
                 graph: bool = True, group=None, always_exchange: bool = False):
        super().__init__(cfg, capacity_bytes, piece_bytes, device, world, rank, group, max_chunks, max_chunks_global,
                         stream_capacity=stream_capacity, graph=graph, always_exchange=always_exchange, before=self._debug_sync if _DEBUG_SYNC else None)
        self._lsh_tables = torch.empty((cfg.bands, ops.l4_lsh_slots(self.max_unique)), dtype=torch.int32, device=device)    # this rank's band tables
        ops.l4_lsh_update(self._sig, 0, 0, cfg, self._band_keys, self._base, self._lsh_tables)               # clears the tables

    # ------------------------------------------------------------------ the two phases (enqueue only)
    def _debug_sync(self, phase: str, n: int) -> None:
        """HMSE_STREAM_DEBUG_SYNC=1: localise a device fault to (rank, batch, phase) — diagnostics only."""
        import sys
        torch.cuda.synchronize()
        cap = (self.row_bytes - 32) // 32
        o = (((cap + 1) * 8 + 255) // 256) * 256
        l2o = o + 512 + 2 * ((cap * 8 + 255) // 256 * 256) + 256 + (((cap + 1) * 8 + 255) // 256) * 256 + ((cap + 255) // 256) * 256 + 256 + ((self.row_bytes + 255) // 256) * 256
        print(f"[stream_dist] rank {self.rank} batch {self.n_batches} phase {phase} n={n} state={self._state.tolist()[:11]} n_cuts={self._ws[o:o + 8].view(torch.int64).item()} "
              f"l2_status={self._ws[o + 256:o + 260].view(torch.int32).item()} l2hdr={self._ws[l2o:l2o + 32].view(torch.int64).tolist()}", file=sys.stderr, flush=True)

    def hash_piece(self, n: int) -> torch.Tensor:
        """Phase A for the next piece (its bytes are at data[state.off ..)): returns this rank's exchange row."""
        seg_off = self._graphs.entry(n).seg_off
        self._graphs.run(n, "A", lambda: ops.stream_piece_hash(self.data, n, self.cap_bytes, seg_off, self.cfg, self._stream_arrays(), self._row, self._ws))
        return self._row

    def encode_piece(self, n: int, rows: torch.Tensor) -> None:
        """Phase B: `rows` = the rows of all ranks in rank order (a tensor whose address is stable across batches when graphs are on)."""
        rows = self._stable(rows, self._row, self._rows)
        self._graphs.run(n, "B", lambda: ops.stream_piece_encode(self.data, n, self.cap_bytes, self.cfg, self._stream_arrays(), rows, self._ws))
        self._graphs.end_batch(n)
        self.n_batches += 1

    def _process(self, off: int, n: int, copied: torch.cuda.Event) -> None:
        torch.cuda.current_stream().wait_event(copied)
        rows = self._gather(self.hash_piece(n), self._rows)
        self.encode_piece(n, rows)

    # ------------------------------------------------------------------ results
    def finish(self, check: bool = True) -> ShardResult:
        self._drain()
        st = self.read_state(check)
        n_unique = st[SB_U_OLD]
        return self._result(st[SB_OFF], st[SB_N_OLD], st[SB_G_OLD], self._uniq[:n_unique], self._sig[:n_unique], self._band_keys[:n_unique],
                            self._base[:n_unique], self._streams[: st[SB_S_OLD]], self._stream_off[: n_unique + 1], self._kind[:n_unique])


def stream_shards_local(batches: list, cfg: IngestConfig, world: int, device, piece_bytes: int | None = None, graph: bool = True,
                        **kw) -> list:
    """A `world`-rank stream with every rank on THIS GPU, in lock step: phase A of every rank, the rows concatenated as the
    all-gather would deliver them, phase B of every rank — per global batch.  `batches`: host uint8 tensors (the global
    batches, whole segments except the last).  Each result is what the rank would hold after DistStreamIngest.finish()."""
    ranks, steps = lockstep_ranks(batches, cfg, world, lambda cap, pb, r: DistStreamIngest(cfg, cap, pb, device, world, r, graph=graph, **kw), piece_bytes)
    rows = torch.zeros(world * ranks[0].row_bytes, dtype=torch.uint8, device=device)
    for ns in steps:
        for r, (n, s) in enumerate(zip(ns, ranks)):
            rows[r * s.row_bytes: (r + 1) * s.row_bytes].copy_(s.hash_piece(n))
        for n, s in zip(ns, ranks):
            s.encode_piece(n, rows)
    return [s.finish() for s in ranks]


def store_results(results: list, only: int | None = None) -> list:
    """The ranks' results of a multi-rank stream in the STORE numbering — what manifest.build_manifest needs to write one manifest
    per rank that manifest.merge_manifests can join: chunk indices become (shard, local) = vbase[shard] + local, so every shard's
    chunks are contiguous again (`chunk_base`, `shard_bases`), `first_occ` is translated, and `pieces` records where the shard's
    chunks sit in the STREAM order (the shards interleave; the reader restores the stream from it).  A first occurrence may live on
    a later-numbered shard (HMSE_MANIFEST_ANY_SHARD_TARGET).  `results`: every rank's DistStreamIngest.finish(), in rank order
    (stream_shards_local returns exactly that; N processes all-gather their `gidx` first — gather_global_index — and convert
    `only` their own)."""
    import dataclasses

    import numpy as np
    from .manifest import PIECE_DTYPE
    dev = results[0].cuts.device
    counts = [int(r.gidx.numel()) for r in results]
    vbase = [sum(counts[:i]) for i in range(len(results))]
    n_global = results[0].n_global
    to_store = torch.full((n_global,), -1, dtype=torch.int64, device=dev)
    for r, vb in zip(results, vbase):
        to_store[r.gidx] = torch.arange(vb, vb + r.gidx.numel(), dtype=torch.int64, device=dev)
    if bool((to_store < 0).any()):
        raise ValueError("store_results: the ranks' chunks do not tile the stream")
    out = []
    for rank, (r, vb) in enumerate(zip(results, vbase)):
        if only is not None and rank != only:
            out.append(None)
            continue
        g = r.gidx.cpu().numpy()
        starts = np.nonzero(np.diff(g, prepend=g[:1] - 2) != 1)[0] if len(g) else np.zeros(0, np.int64)
        ends = np.append(starts[1:], len(g))
        pieces = np.zeros(len(starts), PIECE_DTYPE)
        pieces["g0"] = g[starts] if len(g) else 0
        pieces["n"] = ends - starts
        out.append(dataclasses.replace(r, first_occ=to_store[r.first_occ], chunk_base=vb, shard_bases=list(vbase), pieces=pieces))
    return out


def gather_global_index(res, group=None):
    """N processes: every rank's `gidx` (all-gather; 8 B per chunk), as the list store_results() wants — only the index maps travel,
    the other ranks' results stay where they are: returns light stand-ins carrying (gidx, n_global) for the other ranks."""
    import types
    import torch.distributed as dist
    from .ingest import gather_rows
    allg, base, total, bases = gather_rows(res.gidx.reshape(-1, 1), group)
    world = dist.get_world_size(group)
    bases = list(bases) + [total]
    out = []
    for r in range(world):
        out.append(res if r == dist.get_rank(group) else types.SimpleNamespace(gidx=allg[bases[r]: bases[r + 1], 0], n_global=res.n_global, cuts=res.cuts))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Global L4 for a multi-rank stream ("cross-GPU base-chunk fetch over xGMI for global L4 (config 5)")
# ---------------------------------------------------------------------------------------------------------------------------
class GlobalL4StreamIngest(RankStream):
    """This rank's side of a multi-rank stream whose L4 base selection spans ALL ranks (README.md:1375-1383 against one band
    table): besides the digests, every batch all-gathers the signatures of its newly stored chunks; every rank keeps the same
    band tables over the GLOBAL stored-chunk order (batch, rank, local) and so finds the same bases as a one-rank run; a base
    stored on another rank is fetched over xGMI (three all-to-alls, ingest.fetch_chunks_routed) into a ghost area behind the
    rank's data, where the DEFLATE kernel addresses it by chunk id.  Dedupe AND dictionaries are then those of the one-rank
    stream: the records of all ranks, put in global stored order, are bit-identical to its records.

    Per batch the host sizes three ragged exchanges, so this path is enqueued stage by stage (no hipGraph); the shard-local
    DistStreamIngest stays the captured fast path.  The stages are methods so that tests/ can drive several ranks in lock step on
    one GPU (stream_shards_local_global_l4): stage_hash -> [digests of all ranks] -> stage_index -> [signatures of all ranks] ->
    stage_lsh -> [ghost chunks] -> stage_encode.

    finish() -> ShardResult with: gidx (local chunk -> global chunk), ug (local stored slot -> global stored index), base (local
    slot of the dictionary, -1 if none or remote), base_global (GLOBAL STORED index of the dictionary in stream order, -1 none),
    remote_bases ((slot, owner rank, owner's slot) table for manifest.build_manifest)."""

    def __init__(self, cfg: IngestConfig, capacity_bytes: int, piece_bytes: int, device, world: int, rank: int, group=None,
                 max_chunks: int | None = None, max_chunks_global: int | None = None, ghost_bytes: int | None = None):
        super().__init__(cfg, capacity_bytes, piece_bytes, device, world, rank, group, max_chunks, max_chunks_global,
                         ghost_bytes=ghost_bytes if ghost_bytes is not None else 2 * piece_bytes, limit_pieces=False)    # (stages are sized per batch: a piece may have any size)
        mg = self.max_chunks_g
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        self._cuts = z(self.max_chunks + 1, torch.int64)
        self.n_chunks = 0
        # this rank's stored chunks (appended per batch)
        self._uniq, self._ug, self._base, self._base_global, self._kind, self._sig_l, self._keys_l = [], [], [], [], [], [], []
        self._stream_parts, self._stream_lens = [], []
        self.n_unique = 0
        # the global band tables: identical on every rank (like the global index)
        self._mug = max_stored(mg)
        self._sig_g = torch.empty((self._mug, cfg.n_hashes), dtype=torch.int32, device=device)
        self._keys_g = z((self._mug, cfg.bands), torch.int32)
        self._base_g = z(self._mug, torch.int64)
        self._lsh_tables = torch.empty((cfg.bands, ops.l4_lsh_slots(self._mug)), dtype=torch.int32, device=device)
        self._g_owner = z(self._mug, torch.int64)     # global stored chunk -> owning rank, that rank's stored slot
        self._g_local = z(self._mug, torch.int64)
        ops.l4_lsh_update(self._sig_g, 0, 0, cfg, self._keys_g, self._base_g, self._lsh_tables)               # clears the tables
        self.n_global = 0
        self.u_global = 0
        self.u_counts = [0] * self.world
        self._ws = None
        self.remote_dictionaries = 0
        self.ghost_bytes_fetched = 0

    # ------------------------------------------------------------------ the four stages of one batch
    def stage_hash(self, off: int, n: int) -> torch.Tensor:
        """L2 + L3 of this rank's piece (bytes [off, off + n) of its data): cuts appended, -> digests uint8[n_b, 32]."""
        n_old = self.n_chunks
        if n:
            cuts_b = ops.l2_cdc(self.data[off: off + n], self.cfg)
            n_b = cuts_b.numel() - 1
            if n_old + n_b > self.max_chunks:
                raise ValueError("stream index capacity exceeded (max_chunks)")
            self._cuts[n_old + 1: n_old + n_b + 1] = cuts_b[1:] + off
            dg = ops.l3_sha256(self.data[: off + n], self._cuts[n_old: n_old + n_b + 1])
        else:
            n_b, dg = 0, torch.empty((0, 32), dtype=torch.uint8, device=self.dev)
        self._cur = dict(off=off, n=n, n_old=n_old, n_b=n_b)
        return dg

    def stage_index(self, all_digests: torch.Tensor, counts: list) -> torch.Tensor:
        """The batch's digests of ALL ranks (rank order) join the global index; -> signatures int32[u_b, 128] of the chunks THIS
        rank stores (first occurrences in global order)."""
        c = self._cur
        g_old, g_new = self.n_global, int(sum(counts))
        if g_old + g_new > self.max_chunks_g:
            raise ValueError("global index capacity exceeded (max_chunks_global)")
        self._digests_g[g_old: g_old + g_new] = all_digests
        ops.l3_index_update(self._digests_g, g_old, g_new, self._first_occ_g, self._refcount_g, self._l3_table)
        mine0 = g_old + int(sum(counts[: self.rank]))
        g = torch.arange(mine0, mine0 + c["n_b"], dtype=torch.int64, device=self.dev)
        self._gidx[c["n_old"]: c["n_old"] + c["n_b"]] = g
        uniq_new = c["n_old"] + (self._first_occ_g[mine0: mine0 + c["n_b"]] == g).nonzero().flatten()
        self.n_global = g_old + g_new
        self.n_chunks = c["n_old"] + c["n_b"]
        c["uniq_new"] = uniq_new
        end = c["off"] + c["n"]
        c["sig"] = ops.l4_minhash(self.data[:end], self._cuts[: self.n_chunks + 1], self.cfg, uniq_new) if uniq_new.numel() else \
            torch.empty((0, self.cfg.n_hashes), dtype=torch.int32, device=self.dev)
        return c["sig"]

    def stage_lsh(self, all_sigs: torch.Tensor, counts_u: list):
        """The batch's signatures of ALL ranks (rank order) join the global band tables; this rank's bases are resolved.
        -> (counts per owner rank, owners' local stored slots grouped by owner): the remote dictionaries to fetch."""
        c = self._cur
        u_old, u_new = self.u_global, int(sum(counts_u))
        if u_old + u_new > self._mug:
            raise ValueError("global stored-chunk capacity exceeded")
        if u_new:
            self._sig_g[u_old: u_old + u_new] = all_sigs
            o = u_old
            for r, cnt in enumerate(counts_u):
                if cnt:
                    self._g_owner[o: o + cnt] = r
                    self._g_local[o: o + cnt] = torch.arange(self.u_counts[r], self.u_counts[r] + cnt, dtype=torch.int64, device=self.dev)
                    self.u_counts[r] += cnt
                    o += cnt
            ops.l4_lsh_update(self._sig_g, u_old, u_new, self.cfg, self._keys_g, self._base_g, self._lsh_tables)
        self.u_global = u_old + u_new
        m0 = u_old + int(sum(counts_u[: self.rank]))
        u_b = int(counts_u[self.rank])
        bg = self._base_g[m0: m0 + u_b].clone()
        has = bg >= 0
        own = has & (self._g_owner[bg.clamp(min=0)] == self.rank)
        remote = has & ~own
        c.update(m0=m0, u_b=u_b, bg=bg, own=own, remote=remote)
        req = torch.unique(bg[remote])                                     # ascending global stored indices
        owner = self._g_owner[req]
        perm = torch.argsort(owner, stable=True)                            # grouped by owner, ascending inside a group
        c["req"] = req[perm]
        counts = torch.bincount(owner, minlength=self.world)[: self.world]
        return counts, self._g_local[c["req"]]

    def serve(self, local_slots: torch.Tensor):
        """Raw bytes of this rank's stored chunks `local_slots` (what fetch_chunks_routed sends to a peer): (bytes, lens)."""
        uniq = torch.cat(self._uniq) if self._uniq else torch.empty(0, dtype=torch.int64, device=self.dev)
        c = getattr(self, "_cur", None)
        if c is not None and "uniq_new" in c and not c.get("committed", False):
            uniq = torch.cat([uniq, c["uniq_new"]])                          # (a chunk of THIS batch can already be a peer's dictionary)
        return serve_chunks(uniq, self._cuts, self.data, local_slots)

    def stage_encode(self, ghost: torch.Tensor, ghost_lens: torch.Tensor) -> None:
        """DEFLATE of this rank's newly stored chunks; a remote dictionary is ghost chunk j (the j-th request of stage_lsh)."""
        c = self._cur
        cfg, dev = self.cfg, self.dev
        uniq_new, bg, own, remote = c["uniq_new"], c["bg"], c["own"], c["remote"]
        gb = int(ghost.numel())
        if gb > self.ghost_cap:
            raise ValueError(f"a batch needs {gb} bytes of remote dictionaries, the ghost area holds {self.ghost_cap} (ghost_bytes=)")
        uniq_all = torch.cat(self._uniq + [uniq_new]) if (self._uniq or uniq_new.numel()) else uniq_new
        base_local = torch.where(own, self._g_local[bg.clamp(min=0)], torch.full_like(bg, -1))
        base_chunk = torch.where(own, uniq_all[base_local.clamp(min=0)] if uniq_all.numel() else bg, torch.full_like(bg, -1))
        cuts_x = self._cuts[: self.n_chunks + 1]
        if c["req"].numel():
            self.data[self.capacity: self.capacity + gb] = ghost
            gcuts = self.capacity + torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(ghost_lens, 0)])
            cuts_x = torch.cat([cuts_x, gcuts])                              # chunk n_chunks = the gap up to the ghost area (never named)
            rs, inv = torch.sort(c["req"])
            j = inv[torch.searchsorted(rs, bg.clamp(min=0)).clamp(max=rs.numel() - 1)]
            base_chunk = torch.where(remote, self.n_chunks + 1 + j, base_chunk)
            self.remote_dictionaries += int(remote.sum().item())
            self.ghost_bytes_fetched += gb
        if uniq_new.numel():
            n_b = c["n_b"]
            worst = deflate_ws_bytes(c["n"], n_b, cfg)
            if self._ws is None or self._ws.numel() < worst:
                self._ws = None
                self._ws = torch.empty(worst, dtype=torch.uint8, device=dev)
            streams, off, kind = ops.l1_deflate(self.data, cuts_x, cfg, uniq_new, base_chunk, base_is_chunk_id=True, ws=self._ws)
            self._stream_parts.append(streams); self._stream_lens.append(off[1:] - off[:-1])
            self._kind.append(kind)
        self._uniq.append(uniq_new)
        self._ug.append(torch.arange(c["m0"], c["m0"] + c["u_b"], dtype=torch.int64, device=dev))
        self._base.append(base_local); self._base_global.append(bg)
        self._sig_l.append(c["sig"]); self._keys_l.append(self._keys_g[c["m0"]: c["m0"] + c["u_b"]].clone())
        self.n_unique += c["u_b"]
        c["committed"] = True
        self.n_batches += 1

    # ------------------------------------------------------------------ N processes: the stages joined by collectives
    def _agree(self, err) -> None:
        """COLLECTIVE: did this rank's last step fail?  If ANY rank says yes, EVERY rank raises — a rank that raised alone between two
        collectives would leave its peers blocked in the next one with no diagnosis.  (This mode is host-sized: it
        synchronises per stage anyway.)"""
        if self.world == 1:
            if err is not None:
                raise err
            return
        import torch.distributed as dist
        flags = [None] * self.world
        dist.all_gather_object(flags, None if err is None else str(err), group=self.group)
        bad = [(r, m) for r, m in enumerate(flags) if m is not None]
        if bad:
            self.failed = True
            raise ValueError("global-L4 stream abandoned on every rank: " + "; ".join(f"rank {r}: {m}" for r, m in bad))

    def _guard(self, fn, *args):
        """Run one stage; its rank-local refusal (a capacity) is agreed with the peers before anybody meets the next collective."""
        try:
            out, err = fn(*args), None
        except Exception as e:        # (ops.HmseError is a RuntimeError)
            out, err = None, e
        self._agree(err)
        return out

    def _refuse(self, err) -> bool:
        """push(): a piece this rank cannot take is agreed with the peers — every rank raises, none goes on to the batch's collectives."""
        self._agree(None if err is None else ValueError(err))
        return False

    def _process(self, off: int, n: int, copied) -> None:
        from .ingest import fetch_chunks_routed, gather_rows
        torch.cuda.current_stream().wait_event(copied)
        dg = self._guard(self.stage_hash, off, n)
        if self.world == 1:       # one rank: no process group needed, every dictionary is local
            sig = self.stage_index(dg, [int(dg.shape[0])])
            self.stage_lsh(sig, [int(sig.shape[0])])
            self.stage_encode(torch.empty(0, dtype=torch.uint8, device=self.dev), torch.empty(0, dtype=torch.int64, device=self.dev))
            return
        alld, _, _, bases = gather_rows(dg, self.group)
        counts = [b - a for a, b in zip(bases, list(bases[1:]) + [alld.shape[0]])]
        sig = self._guard(self.stage_index, alld, counts)
        alls, _, _, ub = gather_rows(sig, self.group)
        counts_u = [b - a for a, b in zip(ub, list(ub[1:]) + [alls.shape[0]])]
        rc, rl = self._guard(self.stage_lsh, alls, counts_u)
        uniq_all = torch.cat(self._uniq + [self._cur["uniq_new"]])
        # (the fetch completes its collectives whatever a peer sent and raises behind the last one: agreed like a stage's refusal)
        ghost, glens = self._guard(fetch_chunks_routed, rc, rl, self.data, self._cuts, uniq_all, self.group)
        self._guard(self.stage_encode, ghost, glens)

    def finish(self) -> ShardResult:
        self._drain()
        dev = self.dev
        cat = lambda parts, dt, shape=(0,): torch.cat(parts) if parts else torch.empty(shape, dtype=dt, device=dev)
        lens = cat(self._stream_lens, torch.int64)
        off = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=off[1:])
        base, bg = cat(self._base, torch.int64), cat(self._base_global, torch.int64)
        kind = cat(self._kind, torch.uint8)
        return self._result(self.n_bytes, self.n_chunks, self.n_global, cat(self._uniq, torch.int64), cat(self._sig_l, torch.int32, (0, self.cfg.n_hashes)),
                            cat(self._keys_l, torch.int32, (0, self.cfg.bands)), base, cat(self._stream_parts, torch.uint8), off, kind,
                            base_global=bg, ug=cat(self._ug, torch.int64), remote_bases=remote_base_rows(bg, base, kind, self._g_owner, self._g_local))


def stream_shards_local_global_l4(batches: list, cfg: IngestConfig, world: int, device, **kw) -> list:
    """A `world`-rank global-L4 stream with every rank on THIS GPU, in lock step: per global batch each stage of every rank, the
    exchanges delivered as the collectives would (concatenation in rank order; remote dictionaries served by the owner's
    `serve`).  Each result is what the rank would hold after GlobalL4StreamIngest.finish()."""
    ranks, steps = lockstep_ranks(batches, cfg, world, lambda cap, pb, r: GlobalL4StreamIngest(cfg, cap, pb, device, world, r, **kw))
    for ns in steps:
        dgs = [s.stage_hash(s.n_bytes, n) for n, s in zip(ns, ranks)]
        alld, counts = torch.cat(dgs), [int(d.shape[0]) for d in dgs]
        sigs = [s.stage_index(alld, counts) for s in ranks]
        alls, counts_u = torch.cat(sigs), [int(x.shape[0]) for x in sigs]
        reqs = [s.stage_lsh(alls, counts_u) for s in ranks]
        ghosts = [serve_requests(ranks, rc.tolist(), rl) for rc, rl in reqs]       # (every rank is served before any commits its batch)
        for s, ghost in zip(ranks, ghosts):
            s.stage_encode(*ghost)
    return [s.finish() for s in ranks]
