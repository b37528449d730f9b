"""Global L4 for a multi-rank stream as hipGraph-captured phases (round 4; SURVEY.md §8f-3 "cross-GPU base-chunk fetch over xGMI P2P for
global L4 (config 5)"; BASELINE.json configs[4] "hipGraph-captured per-batch pipeline"; the reference has ONE set of band tables,
README.md:1375-1383, and one batch loop, README.md:1519-1580).

`stream_dist.GlobalL4StreamIngest` (round 3) gives an N-rank stream the records of the one-rank run, but enqueues every stage eagerly and
sizes three ragged exchanges per batch on the host (2.1-2.3 x the shard-local chain in rehearsal).  Here everything that can be
fixed-size is: per batch and rank

    phase A   hmse_stream_piece_hash      L2 + L3 hash of the piece -> digest row          | all-gather (fixed-size rows)
    phase B1  hmse_stream_piece_sign      global index, new stored chunks, MinHash -> signature row | all-gather (fixed-size rows)
    phase B2  hmse_stream_piece_bases     global band tables -> dictionaries (own chunk ids / remote requests)
    --        remote dictionaries fetched (ingest.fetch_chunks_routed: the ONE step left eager; skipped with one rank)
    phase B3  hmse_stream_piece_encode_g  DEFLATE, tails, states advanced

each phase captured into a hipGraph at its second use and replayed afterwards; the host reads ONE small array per batch (the request counts
and this rank's stored count, only when world > 1).  Whatever a rank cannot do between two collectives (a fetch that a peer refused, a
ghost area too small, a phase's error code) becomes sticky status bit 16 on the device: the rank drops the batch, stays in every
collective with empty rows, and finish() raises on every rank.  The result of every rank equals `GlobalL4StreamIngest`'s
(tests/test_gpu_stream_gl4.py: 2 and 3 ranks in lock step, and two real processes over gloo, against the oracle's single pass over the
logical stream).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops
from .config import IngestConfig
from .ingest import ShardResult
from .stream_common import (GL4_REQ_EXTRA, GL4_REQ_STORED, GL4_REQ_TOTAL, SB_G_OLD, SB_N_OLD, SB_OFF, SB_S_OLD, SB_STATUS, SB_U_OLD, SB_WORDS,
                            CapturedRankStream, chain_status_error, lockstep_ranks, max_stored, remote_base_rows, serve_chunks, serve_requests)


class GraphGlobalL4StreamIngest(CapturedRankStream):
    """This rank's side of a global-L4 stream over `world` ranks, every phase a hipGraph replay.  COLLECTIVE: every rank pushes its
    piece of every global batch, in the same order (an empty tensor if it has no bytes in a batch)."""

    def __init__(self, cfg: IngestConfig, capacity_bytes: int, piece_bytes: int, device, world: int, rank: int, group=None,
                 max_chunks: int | None = None, max_chunks_global: int | None = None, stream_capacity: int | None = None,
                 ghost_bytes: int | None = None, graph: bool = True, always_exchange: bool = False):
        self.sig_cap = ops.stream_sig_cap(int(piece_bytes), cfg)
        # the cut array continues behind this rank's chunks with the bounds of the batch's fetched dictionaries ("ghost" chunks)
        super().__init__(cfg, capacity_bytes, piece_bytes, device, world, rank, group, max_chunks, max_chunks_global,
                         ghost_bytes=ghost_bytes if ghost_bytes is not None else 2 * piece_bytes, stream_capacity=stream_capacity, graph=graph,
                         always_exchange=always_exchange, extra_cuts=self.sig_cap + 2)
        self.ghost_chunk0 = self.max_chunks + 1
        self.max_stored_g = max_stored(self.max_chunks_g)
        mu, mug = self.max_unique, self.max_stored_g
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        self._base_global = z(mu, torch.int64)       # global stored index of the dictionary
        self._ug = z(mu, torch.int64)                # global stored index of the chunk
        # the global band tables: identical on every rank (like the global index)
        self._sig_g = torch.empty((mug, cfg.n_hashes), dtype=torch.int32, device=device)
        self._keys_g = z((mug, cfg.bands), torch.int32)
        self._base_g = z(mug, torch.int64)
        self._lsh_tables_g = torch.empty((cfg.bands, ops.l4_lsh_slots(mug)), dtype=torch.int32, device=device)
        self._g_owner = z(mug, torch.int32)
        self._g_local = z(mug, torch.int64)
        ops.l4_lsh_update(self._sig_g, 0, 0, cfg, self._keys_g, self._base_g, self._lsh_tables_g)               # clears the tables
        self._gstate = z(SB_WORDS, torch.int64)
        self.sig_row_bytes = ops.stream_sig_row_bytes(self.cap_bytes, cfg)
        self._sig_row = z(self.sig_row_bytes, torch.uint8)
        self._sig_rows = z(self.world * self.sig_row_bytes, torch.uint8)
        self._req_counts = z(self.world + GL4_REQ_EXTRA, torch.int64)      # per rank, then the total and this rank's stored chunks, this batch's included
        self._req_slots = z(self.sig_cap, torch.int64)
        g = _lib.HmseGl4()
        g.struct_size = C.sizeof(_lib.HmseGl4); g.world = self.world; g.rank = self.rank; g.reserved = 0
        g.sig_cap = self.sig_cap; g.max_stored_g = mug
        g.gstate = self._gstate.data_ptr(); g.sig_g = self._sig_g.data_ptr(); g.band_keys_g = self._keys_g.data_ptr(); g.base_g = self._base_g.data_ptr()
        g.lsh_tables_g = self._lsh_tables_g.data_ptr(); g.lsh_slots_g = self._lsh_tables_g.shape[1]
        g.g_owner = self._g_owner.data_ptr(); g.g_local = self._g_local.data_ptr(); g.ug = self._ug.data_ptr(); g.base_global = self._base_global.data_ptr()
        g.req_counts = self._req_counts.data_ptr(); g.req_slots = self._req_slots.data_ptr(); g.ghost_chunk0 = self.ghost_chunk0
        self._gl4 = g
        self.remote_dictionaries = 0
        self.ghost_bytes_fetched = 0
        self.n_stored_now = 0                        # what requests() last read: the bound of the slots a peer may ask for

    # ------------------------------------------------------------------ the phases of one batch (enqueue only; captured at a size's second use)
    def phase_a(self, n: int) -> torch.Tensor:
        seg_off = self._graphs.entry(n).seg_off
        self._graphs.run(n, "A", lambda: ops.stream_piece_hash(self.data, n, self.cap_bytes, seg_off, self.cfg, self._stream_arrays(), self._row, self._ws))
        return self._row

    def phase_b1(self, n: int, rows: torch.Tensor) -> torch.Tensor:
        rows = self._stable(rows, self._row, self._rows)
        self._graphs.run(n, "B1", lambda: ops.stream_piece_sign(self.data, n, self.cap_bytes, self.cfg, self._stream_arrays(), rows, self._sig_row, self._ws))
        return self._sig_row

    def phase_b2(self, n: int, sig_rows: torch.Tensor) -> None:
        sig_rows = self._stable(sig_rows, self._sig_row, self._sig_rows)
        self._graphs.run(n, "B2", lambda: ops.stream_piece_bases(self.cap_bytes, self.cfg, self._stream_arrays(), sig_rows, self._gl4, self._ws))

    def phase_b3(self, n: int) -> None:
        self._graphs.run(n, "B3", lambda: ops.stream_piece_encode_g(self.data, n, self.cap_bytes, self.cfg, self._stream_arrays(), self._gstate, self._ws))
        self._graphs.end_batch(n)
        self.n_batches += 1

    # ------------------------------------------------------------------ the remote dictionaries of a batch (eager)
    def requests(self):
        """(requests per owner rank [world], the owners' stored slots grouped by owner) of the batch phase B2 just resolved — ONE host read,
        which also brings this rank's stored count (`n_stored_now`: what a peer may ask of it in this batch)."""
        c = self._req_counts.tolist()
        self.n_stored_now = c[self.world + GL4_REQ_STORED]
        if self._host_refused:          # this rank is out: it asks for nothing (the array may be a batch old), and goes on serving
            return [0] * self.world, self._req_slots[:0]
        return c[: self.world], self._req_slots[: c[self.world + GL4_REQ_TOTAL]]

    def serve(self, local_slots: torch.Tensor):
        """Raw bytes of this rank's stored chunks `local_slots` (what a peer's fetch gets): (bytes, lens).  A chunk stored by THIS batch
        can already be a peer's dictionary: phase B1 has appended it."""
        return serve_chunks(self._uniq, self._cuts, self.data, local_slots)

    def write_ghost(self, ghost: torch.Tensor, lens: torch.Tensor) -> None:
        """The fetched dictionaries, in request order, behind this rank's data; their bounds behind its cuts (request j = chunk ghost_chunk0 + j).
        A batch whose dictionaries do not fit is REFUSED through the chain (status bit 16), never raised: the peers are at the next collective."""
        gb, k = int(ghost.numel()), int(lens.numel())
        if gb > self.ghost_cap or k > self.sig_cap:
            self._host_refuse(f"a batch needs {gb} bytes / {k} remote dictionaries, the ghost area holds {self.ghost_cap} bytes / {self.sig_cap} chunks (ghost_bytes=)")
            return
        if k and not self._host_refused:
            self.data[self.capacity: self.capacity + gb] = ghost
            g0 = self.ghost_chunk0
            self._cuts[g0] = self.capacity
            self._cuts[g0 + 1: g0 + 1 + k] = self.capacity + torch.cumsum(lens, 0)
            self.remote_dictionaries += k
            self.ghost_bytes_fetched += gb

    # ------------------------------------------------------------------ N processes: the phases joined by collectives
    def _try(self, what: str, fn, *args):
        """One phase of a batch.  A rank that raised here alone would leave its peers blocked in the batch's next collective with no diagnosis
        (ADVICE r3), so its failure (ops.HmseError is a RuntimeError) is refused through the chain instead; -> None then."""
        try:
            return fn(*args)
        except Exception as e:
            self._host_refuse(f"{what}: {e}")
            return None

    def _process(self, off: int, n: int, copied) -> None:
        torch.cuda.current_stream().wait_event(copied)
        if self._try("phase A", self.phase_a, n) is None:
            self._row[:8] = 0                       # (the row of an earlier batch must not be gathered again)
        rows = self._gather(self._row, self._rows)
        if self._try("phase B1", self.phase_b1, n, rows) is None:
            self._sig_row[:8] = 0
        sig_rows = self._gather(self._sig_row, self._sig_rows)
        self._try("phase B2", self.phase_b2, n, sig_rows)
        if self.world > 1:
            from .ingest import fetch_chunks_routed
            counts, slots = self.requests()
            refused = []
            ghost, lens = fetch_chunks_routed(torch.tensor(counts, dtype=torch.int64), slots, self.data, self._cuts, self._uniq, self.group,
                                              n_stored=self.n_stored_now, refused=refused)
            if refused:
                self._host_refuse("; ".join(refused))
            self.write_ghost(ghost, lens)
        self._try("phase B3", self.phase_b3, n)     # (the status bit is on the device by now: B3 and every later batch are no-ops)

    # ------------------------------------------------------------------ results
    def finish(self, check: bool = True) -> ShardResult:
        self._drain()
        st = self.read_state(check)
        nu = st[SB_U_OLD]
        base, bg, kind = self._base[:nu], self._base_global[:nu], self._kind[:nu]
        return self._result(st[SB_OFF], st[SB_N_OLD], st[SB_G_OLD], self._uniq[:nu], self._sig[:nu], self._band_keys[:nu], base, self._streams[: st[SB_S_OLD]],
                            self._stream_off[: nu + 1], kind, base_global=bg, ug=self._ug[:nu],
                            remote_bases=remote_base_rows(bg, base, kind, self._g_owner, self._g_local))


def lockstep_gl4_graph(batches: list, cfg: IngestConfig, world: int, device, rank_kw: list | None = None, setup=None, **kw) -> list:
    """`world` ranks of a captured global-L4 stream on THIS GPU, driven in lock step over `batches`: per global batch each phase of every rank,
    the exchanges delivered as the collectives would (rows concatenated in rank order; remote dictionaries served by the owner's `serve`,
    a slot at or above the owner's stored count refused on both sides as ingest.fetch_chunks_routed does).  `rank_kw[r]`: keyword
    arguments of rank r alone; `setup(ranks)` runs before the first batch.  -> the ranks, before finish()."""
    mk = lambda cap, pb, r: GraphGlobalL4StreamIngest(cfg, cap, pb, device, world, r, **{**kw, **(rank_kw[r] if rank_kw else {})})
    ranks, steps = lockstep_ranks(batches, cfg, world, mk)
    if setup is not None:
        setup(ranks)
    for ns in steps:
        rows = torch.cat([s.phase_a(n).clone() for n, s in zip(ns, ranks)])
        sig_rows = torch.cat([s.phase_b1(n, rows).clone() for n, s in zip(ns, ranks)])
        for n, s in zip(ns, ranks):
            s.phase_b2(n, sig_rows)
        reqs = [s.requests() for s in ranks]          # (every rank's stored count is read before anybody is served)
        for s, (counts, slots) in zip(ranks, reqs):
            o, bad = 0, None
            for owner, cnt in enumerate(counts):
                if cnt and int(slots[o: o + cnt].max()) >= ranks[owner].n_stored_now:
                    bad = owner
                    ranks[owner]._host_refuse(f"fetch_chunks: a peer asked for stored chunk {int(slots[o: o + cnt].max())} of {ranks[owner].n_stored_now}")
                o += cnt
            if bad is not None:
                s._host_refuse(f"fetch_chunks: rank {bad} refused a request: no such stored chunk there")
            else:
                s.write_ghost(*serve_requests(ranks, counts, slots))
        for n, s in zip(ns, ranks):
            s.phase_b3(n)
    return ranks


def stream_shards_local_gl4_graph(batches: list, cfg: IngestConfig, world: int, device, **kw) -> list:
    """A `world`-rank captured global-L4 stream with every rank on THIS GPU (lockstep_gl4_graph).  Each result is what the rank would hold
    after GraphGlobalL4StreamIngest.finish() — which fails on EVERY rank if one rank dropped a batch (between processes: the all-reduce
    of the status; here the same rule by hand, for the peers of such a rank have indexed chunks that nobody stores)."""
    ranks = lockstep_gl4_graph(batches, cfg, world, device, **kw)
    status = [int(s._state[SB_STATUS].item()) for s in ranks]
    if any(status):
        r = max(range(world), key=lambda i: status[i])
        raise chain_status_error(status[r], f" on rank {r}", ranks[r]._host_error)
    return [s.finish() for s in ranks]
