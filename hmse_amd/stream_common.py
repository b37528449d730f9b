"""What the streaming front ends share (stream.StreamIngest, stream_dist.DistStreamIngest / GlobalL4StreamIngest,
stream_gl4.GraphGlobalL4StreamIngest): the eager -> capture -> replay policy of a batch size (PhaseGraphs), the text of the chain's
sticky status word and its agreement over the ranks, the feeder of a multi-rank stream (RankStream: argument checks, buffers, push,
the drain) with the refusal rule of the captured classes (CapturedRankStream), the result tables of a global-L4 stream, and the
scaffold that drives several ranks in lock step on one GPU.
"""
from __future__ import annotations

import gc
from dataclasses import dataclass, field

import numpy as np
import torch

from . import ops
from .config import LAYER_L1, LAYER_L2, LAYER_L3, LAYER_L4, IngestConfig
from .ingest import ShardResult, shard_stats


# ---------------------------------------------------------------------------------------------------------------------------
# sizing
# ---------------------------------------------------------------------------------------------------------------------------
def default_max_chunks(capacity_bytes: int, cfg: IngestConfig) -> int:
    """Index entries for `capacity_bytes`: twice the expected count at the configured average chunk size, one forced cut per segment."""
    return capacity_bytes // max(1, cfg.avg_size // 2) + capacity_bytes // cfg.seg_size + 64


def max_stored(max_chunks: int) -> int:
    return min(max_chunks, 1 << 23)     # the band tables hold 2^24 slots at load <= 0.5


def default_stream_capacity(capacity_bytes: int) -> int:
    return capacity_bytes // 2 + (64 << 20)


def deflate_ws_bytes(n_bytes: int, n_chunks: int, cfg: IngestConfig) -> int:
    """A DEFLATE workspace for the worst case of a batch of `n_bytes` in `n_chunks` chunks: every chunk stored, every one with a dictionary."""
    return (5 * n_bytes + 1600 * n_chunks) + ops.workspace_bytes(ops.STAGE_DEFLATE, n_chunks, cfg) + (1 << 20)


# ---------------------------------------------------------------------------------------------------------------------------
# capture policy
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class SizeEntry:
    seg_off: torch.Tensor | None            # segment offsets of a batch of this size (None: an empty piece)
    ws: torch.Tensor | None = None          # a workspace the owner keeps per size (StreamIngest)
    graphs: dict = field(default_factory=dict)      # phase -> CUDAGraph
    uses: int = 0                           # batches of this size that ran all their phases


class PhaseGraphs:
    """Per batch size: first use — plain enqueue (also sets the kernels' attributes before any capture); second use — every phase is
    captured into a hipGraph; from then on — replay.  `new_size(size) -> SizeEntry` allocates what a size needs once; `before(phase, size)`
    runs ahead of every phase (a diagnostics hook)."""

    def __init__(self, graph: bool, new_size, before=None):
        self.graph, self._new_size, self._before = bool(graph), new_size, before
        self._sizes: dict[int, SizeEntry] = {}

    def entry(self, size: int) -> SizeEntry:
        e = self._sizes.get(size)
        if e is None:
            e = self._sizes[size] = self._new_size(size)
        return e

    def run(self, size: int, phase: str, fn) -> None:
        e = self.entry(size)
        if self._before is not None:
            self._before(phase, size)
        if not self.graph or e.uses < 1:
            fn()
            return
        if phase not in e.graphs:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # No finaliser may run between capture_begin and capture_end.  A front end and its PhaseGraphs refer to each other, so a
            # dropped stream — its buffers and its captured graphs — is freed by the cycle collector only, whenever an allocation count
            # trips it; inside a capture that destroys another graph and frees its pool, which the runtime answers with an abort.
            # torch.cuda.graph no longer collects before it begins (torch.compiler.config.force_cudagraph_gc): collect here, then hold
            # the collector off until the capture has ended.
            gc.collect()
            was_enabled = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g):
                    fn()
            finally:
                if was_enabled:
                    gc.enable()
            e.graphs[phase] = g
        e.graphs[phase].replay()

    def end_batch(self, size: int) -> None:
        """After the LAST phase of a batch: the use counter advances once per batch, so all phases of the second batch are captured."""
        self.entry(size).uses += 1

    def captured(self, size: int) -> set:
        return set(self._sizes[size].graphs) if size in self._sizes else set()

    def uses(self, size: int) -> int:
        return self._sizes[size].uses if size in self._sizes else 0

    def sizes(self) -> list:
        return list(self._sizes)

    def drop_graphs(self) -> None:
        """The captured graphs hold addresses that are no longer right; the per-size offsets and workspaces stay, the next use captures again."""
        for e in self._sizes.values():
            e.graphs.clear()


# ---------------------------------------------------------------------------------------------------------------------------
# the chain's state block and its sticky status word: mirrors of HMSE_SB_*, HMSE_STREAM_ST_*, HMSE_GL4_REQ_* (include/hmse.h; tests/test_abi_layout.py)
# ---------------------------------------------------------------------------------------------------------------------------
SB_OFF, SB_N_OLD, SB_N_NEW, SB_U_OLD, SB_U_NEW, SB_S_OLD, SB_S_NEW, SB_STATUS, SB_G_OLD, SB_G_NEW, SB_G_BASE = range(11)
SB_WORDS = 16
ST_CHUNK_CAP, ST_STORED_CAP, ST_L2, ST_ROW, ST_WS_INIT, ST_STATE, ST_PUSH_REFUSED, ST_SIG_ROW = (1 << i for i in range(8))
ST_DEFLATE_SHIFT = 8
ST_HOST_REFUSED = 1 << 16   # set by the HOST of a captured rank between two phases of a batch (CapturedRankStream._host_refuse)
GL4_REQ_TOTAL, GL4_REQ_STORED, GL4_REQ_EXTRA = 0, 1, 2      # req_counts[world + ...]

# (bit, its name behind HMSE_STREAM_ST_ in the header, what it tells the caller) — chain_status_error's text
STATUS_BITS = (
    (ST_CHUNK_CAP, "CHUNK_CAP", "chunk capacity"),
    (ST_STORED_CAP, "STORED_CAP", "stored-chunk capacity"),
    (ST_L2, "L2", "L2 (the batch holds more cut candidates than the chain's fixed candidate list, or more chunks than its cut list: bytes that dense "
              "are ingested by ingest_shard or a graph=False stream, whose L2 call is run again with a larger list)"),
    (ST_ROW, "ROW", "exchange row"),
    (ST_WS_INIT, "WS_INIT", "workspace not initialised"),
    (ST_STATE, "STATE", "state block inconsistent ([8] != [1] on one rank)"),
    (ST_PUSH_REFUSED, "PUSH_REFUSED", "a piece refused by push()"),
    (ST_SIG_ROW, "SIG_ROW", "more new stored chunks than a signature row holds (the row is sized for the worst-case chunk count of a piece: a row of "
                     "another build)"),
    (ST_HOST_REFUSED, "HOST_REFUSED", "a batch refused on the host between two phases (a remote dictionary a peer did not serve, the ghost area, a "
                              "phase's error code)"),
)
DEFLATE_BITS = "bits 8..12 DEFLATE (0x100 stream capacity, 0x200 workspace)"


def chain_status_error(status: int, where: str = "", host_error: str | None = None, intact: str = "") -> ValueError:
    # the reason a rank gave itself goes behind the bit it set: HOST_REFUSED if that is up, else PUSH_REFUSED
    mine = {(ST_HOST_REFUSED if status & ST_HOST_REFUSED else ST_PUSH_REFUSED): f" (this rank: {host_error})"} if host_error else {}
    bits = [f"bit{bit.bit_length() - 1} {text}{mine.get(bit, '')}" for bit, _, text in STATUS_BITS]
    bits.insert(-1, DEFLATE_BITS)
    return ValueError(f"streaming chain status {status:#x}{where}: " + ", ".join(bits) + "; the failing batch and every later one were dropped" + intact)


def agreed_status(status: int, world: int, group, dev, lockstep: bool) -> int:
    """COLLECTIVE unless `lockstep`: the worst status of all ranks — a failed rank must fail the whole stream, its chunks are missing from
    every rank's index."""
    if world == 1 or lockstep:
        return status
    import torch.distributed as dist
    t = torch.tensor([status], dtype=torch.int64, device="cpu" if dist.get_backend(group) == "gloo" else dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return max(status, int(t.item()))


# ---------------------------------------------------------------------------------------------------------------------------
# the exchange of a multi-rank stream
# ---------------------------------------------------------------------------------------------------------------------------
def deal_batch(batch_bytes: int, world: int, seg_size: int) -> list:
    """Piece boundaries of a global batch of `batch_bytes`: contiguous runs of whole segments, rank r gets segments
    [r S / R, (r + 1) S / R) of the batch's S segments (the last segment may be partial: only the stream's last batch)."""
    n_seg = -(-batch_bytes // seg_size)
    b = [min(batch_bytes, (r * n_seg // world) * seg_size) for r in range(world)] + [batch_bytes]
    return b


def all_gather_rows(row: torch.Tensor, world: int, group=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """THE collective of a multi-rank stream's batch: all-gather of the ranks' fixed-size exchange rows, in rank order.
    RCCL over xGMI: device to device, stream-ordered, no host read (1 GiB pieces: 16.8 MB per rank and batch).  gloo (the CPU
    tests and the one-GPU rehearsal): staged through host memory."""
    import torch.distributed as dist
    if out is None:
        out = torch.empty(world * row.numel(), dtype=torch.uint8, device=row.device)
    if dist.get_backend(group) == "gloo":
        rows = torch.empty(world * row.numel(), dtype=torch.uint8)
        dist.all_gather_into_tensor(rows, row.cpu(), group=group)
        out.copy_(rows)
    else:
        dist.all_gather_into_tensor(out, row, group=group)
    return out


def issue_copy(copy_stream, data: torch.Tensor, at: int, host: torch.Tensor) -> torch.cuda.Event:
    """Host -> HBM copy of `host` to data[at ..) on the copy stream (asynchronous when the tensor is pinned); -> its completion event."""
    ev = torch.cuda.Event()
    with torch.cuda.stream(copy_stream):
        if host.numel():
            data[at: at + host.numel()].copy_(host, non_blocking=True)
        ev.record(copy_stream)
    return ev


# ---------------------------------------------------------------------------------------------------------------------------
# results of a global-L4 stream
# ---------------------------------------------------------------------------------------------------------------------------
def serve_chunks(uniq: torch.Tensor, cuts: torch.Tensor, data: torch.Tensor, slots: torch.Tensor):
    """Raw bytes of the stored chunks `slots` of a rank (what a peer's fetch of its dictionaries gets): (bytes, lens)."""
    cid = uniq[slots]
    ln = cuts[cid + 1] - cuts[cid]
    oc = torch.zeros(cid.numel() + 1, dtype=torch.int64, device=data.device)
    torch.cumsum(ln, 0, out=oc[1:])
    return (ops.read_assemble(oc, cid, cuts, data) if cid.numel() else torch.empty(0, dtype=torch.uint8, device=data.device)), ln


def remote_base_rows(bg: torch.Tensor, base: torch.Tensor, kind: torch.Tensor, g_owner: torch.Tensor, g_local: torch.Tensor):
    """(slot, owner rank, owner's slot) of every DELTA record whose dictionary another rank stores — the table manifest.build_manifest
    needs for a global-L4 stream's shard (the ranks' stored chunks interleave in the global numbering); None if there is none."""
    from .manifest import REMOTE_BASE_DTYPE
    slots = ((bg >= 0) & (base < 0) & (kind == 2)).nonzero().flatten()
    if not slots.numel():
        return None
    tab = np.zeros(int(slots.numel()), REMOTE_BASE_DTYPE)
    tab["slot"] = slots.cpu().numpy(); tab["shard"] = g_owner[bg[slots]].cpu().numpy(); tab["base_slot"] = g_local[bg[slots]].cpu().numpy()
    return tab


# ---------------------------------------------------------------------------------------------------------------------------
# this rank's side of a multi-rank stream: the feeder
# ---------------------------------------------------------------------------------------------------------------------------
class RankStream:
    """Buffers, index sizing and the feeder of one rank.  COLLECTIVE: every rank pushes ITS piece of every global batch, in the same
    order (a rank with no bytes in a batch pushes an empty tensor).  A subclass gives `_process(off, n, copied)` (one batch) and
    `_refuse(err) -> bool` (what happens to a piece push() cannot take)."""

    lockstep = False    # True: the ranks are driven in lock step inside ONE process (stream_shards_local*) — there are no collectives

    def __init__(self, cfg: IngestConfig, capacity_bytes: int, piece_bytes: int, device, world: int, rank: int, group,
                 max_chunks: int | None, max_chunks_global: int | None, ghost_bytes: int = 0, limit_pieces: bool = True):
        if cfg.layers != (LAYER_L1 | LAYER_L2 | LAYER_L3 | LAYER_L4):
            raise ValueError(f"{type(self).__name__} runs the full L1-L4 pipeline")
        if piece_bytes <= 0 or piece_bytes % cfg.seg_size:
            raise ValueError("piece_bytes (the nominal piece size) must be a positive multiple of seg_size")
        if not 0 <= rank < world <= 256:
            raise ValueError("0 <= rank < world <= 256")
        self.cfg, self.dev, self.world, self.rank, self.group = cfg, device, int(world), int(rank), group
        self.cap_bytes = int(piece_bytes) if limit_pieces else None     # a pushed piece may not be larger (None: any size)
        self.capacity = int(capacity_bytes)
        self.ghost_cap = int(ghost_bytes)
        self.data = torch.empty(self.capacity + self.ghost_cap, dtype=torch.uint8, device=device)   # [0, capacity): this rank's pieces; behind: fetched dictionaries
        self.n_bytes = 0
        self.copy_stream = torch.cuda.Stream(device=device)
        self.pending: list[tuple[int, int, torch.cuda.Event]] = []      # (offset, length, copy-done event)
        self.max_chunks = int(max_chunks or default_max_chunks(self.capacity, cfg))
        self.max_chunks_g = int(max_chunks_global or self.max_chunks * world)
        mc, mg = self.max_chunks, self.max_chunks_g
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        self._gidx = z(mc, torch.int64)                       # local chunk -> global chunk index
        # the global index: identical on every rank
        self._digests_g = torch.empty((mg, 32), dtype=torch.uint8, device=device)
        self._first_occ_g = z(mg, torch.int64)
        self._refcount_g = z(mg, torch.int32)
        self._l3_table = torch.empty(ops.l3_index_slots(mg), dtype=torch.int32, device=device)
        ops.l3_index_update(self._digests_g, 0, 0, self._first_occ_g, self._refcount_g, self._l3_table)     # clears the table
        self.n_batches = 0

    def push(self, host_piece: torch.Tensor) -> None:
        """Issue the host -> HBM copy of this rank's piece of the next global batch, then process the piece whose copy was
        issued by the previous push (its kernels overlap this copy)."""
        n = host_piece.numel()
        err = None
        if self.cap_bytes is not None and n > self.cap_bytes:
            err = "a piece may not exceed the stream's nominal piece size"
        elif self.n_bytes % self.cfg.seg_size:
            err = "only a rank's last piece may end inside a segment"
        elif self.n_bytes + n > self.capacity:
            err = "stream capacity exceeded"
        refused = self._refuse(err)
        if refused:
            n, host_piece = 0, host_piece[:0]
        ev = issue_copy(self.copy_stream, self.data, self.n_bytes, host_piece)
        self._drain()
        if refused:
            self._mark_refused()        # (behind the piece pushed before, which is still good)
        self.pending.append((self.n_bytes, n, ev))
        self.n_bytes += n

    def _drain(self) -> None:
        while self.pending:
            self._process(*self.pending.pop(0))

    def _result(self, n_done: int, n_chunks: int, n_global: int, uniq, sig, band_keys, base, streams, stream_off, kind, **gl4) -> ShardResult:
        gidx = self._gidx[:n_chunks]
        res = ShardResult(n_done, self._cuts[: n_chunks + 1], self._digests_g[gidx], 0, n_global, self._first_occ_g[gidx], self._refcount_g[gidx],
                          uniq, sig, band_keys, base, streams, stream_off, kind, gidx=gidx, **gl4)
        res.stats = shard_stats(res)
        return res


class CapturedRankStream(RankStream):
    """A rank whose batch is a chain of capturable phases over the device state block `_state` (no host read between them)."""

    def __init__(self, *args, stream_capacity: int | None, graph: bool, always_exchange: bool, extra_cuts: int = 0, before=None, **kw):
        super().__init__(*args, **kw)
        cfg, device = self.cfg, self.dev
        self.max_unique = max_stored(self.max_chunks)
        mc, mu = self.max_chunks, self.max_unique
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        # this rank's chunks (`extra_cuts`: room behind them that a subclass addresses itself) and the chunks it stores
        self._cuts = z(mc + 1 + extra_cuts, torch.int64)
        self._uniq = z(mu, torch.int64)                       # local ids of the chunks this rank stores, ascending
        self._sig = torch.empty((mu, cfg.n_hashes), dtype=torch.int32, device=device)
        self._band_keys = z((mu, cfg.bands), torch.int32)
        self._base = z(mu, torch.int64)                       # this rank's stored slot of the dictionary, -1: none (or remote)
        self._kind = z(mu, torch.uint8)
        self._stream_off = z(mu + 1, torch.int64)
        self._streams = torch.empty(int(stream_capacity or default_stream_capacity(self.capacity)), dtype=torch.uint8, device=device)
        self._lsh_tables = None                               # this rank's band tables, where a subclass keeps them per rank (stream_dist)
        self._state = z(SB_WORDS, torch.int64)
        self._arrays = None                                   # ops.StreamArrays, built at the first phase (_stream_arrays)
        self._host_error = None
        self._host_refused = False
        self._ws = ops.stream_workspace(self.cap_bytes, self.cfg, device)
        self.row_bytes = ops.stream_row_bytes(self.cap_bytes, self.cfg)
        self._row = torch.zeros(self.row_bytes, dtype=torch.uint8, device=device)
        self._rows = torch.zeros(self.world * self.row_bytes, dtype=torch.uint8, device=device)
        self.graph = bool(graph)
        self._graphs = PhaseGraphs(graph, lambda n: SizeEntry(ops.segment_offsets(n, self.cfg.seg_size, device) if n else None), before)
        self._always_exchange = bool(always_exchange)    # world size 1 still runs the collective (hardware rehearsal of the graph / RCCL interleaving)

    def _refuse(self, err) -> bool:
        # A rank that raised in push() alone would leave its peers blocked in this batch's all-gather.  Instead the piece
        # is refused THROUGH the chain: sticky status bit 6 on the device (phase A then reports 0 chunks, every later batch of
        # this rank is a no-op), the rank keeps taking part in the collectives with empty rows, and read_state()'s
        # all-reduce(MAX) of the status makes EVERY rank raise at finish() — this one with the reason.
        if err:
            self._host_error = self._host_error or err
        return bool(err)

    def _mark_refused(self) -> None:
        self._state[SB_STATUS: SB_STATUS + 1] |= ST_PUSH_REFUSED

    def _host_refuse(self, reason: str) -> None:
        """A rank-local failure BETWEEN two phases of a batch (the peers are at, or on their way to, the next collective): like
        _mark_refused, a sticky bit of the device's status word, set in stream order — so the phases enqueued after it drop the batch,
        every later batch is a no-op, the rank keeps taking part in every collective, and finish() raises on every rank."""
        self._host_error = self._host_error or reason
        self._host_refused = True
        self._state[SB_STATUS: SB_STATUS + 1] |= ST_HOST_REFUSED

    def _stream_arrays(self) -> ops.StreamArrays:
        """This rank's descriptor for the library, built at the first phase: a subclass may allocate band tables of its own after __init__."""
        if self._arrays is None:
            self._arrays = ops.StreamArrays(
                world=self.world, rank=self.rank, state=self._state, cuts=self._cuts, max_chunks=self.max_chunks, gidx=self._gidx,
                digests=self._digests_g, max_chunks_g=self.max_chunks_g, first_occ=self._first_occ_g, refcount=self._refcount_g,
                l3_table=self._l3_table, l3_slots=self._l3_table.numel(), uniq=self._uniq, max_unique=self.max_unique, sig=self._sig,
                band_keys=self._band_keys, base=self._base, lsh_tables=self._lsh_tables, lsh_slots=None if self._lsh_tables is None else self._lsh_tables.shape[1],
                kind=self._kind, stream_off=self._stream_off, out=self._streams, out_cap=self._streams.numel())
        return self._arrays

    def _gather(self, row: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        if self.world == 1 and not self._always_exchange:
            return row
        return all_gather_rows(row, self.world, self.group, out=out)

    def _stable(self, rows: torch.Tensor, mine: torch.Tensor, all_rows: torch.Tensor) -> torch.Tensor:
        """The rows of all ranks at an address that is the same in every batch (a captured phase reads them): `all_rows`, or with one
        rank this rank's own row."""
        if rows.data_ptr() != all_rows.data_ptr() and not (self.world == 1 and rows.data_ptr() == mine.data_ptr()):
            all_rows.copy_(rows.reshape(-1))
            rows = all_rows
        return rows

    def read_state(self, check: bool = True) -> list:
        st = self._state.tolist()
        status = agreed_status(st[SB_STATUS], self.world, self.group, self.dev, self.lockstep) if check else 0
        if status:
            raise chain_status_error(status, " on some rank", self._host_error)
        return st


# ---------------------------------------------------------------------------------------------------------------------------
# several ranks in lock step on one GPU
# ---------------------------------------------------------------------------------------------------------------------------
def lockstep_ranks(batches: list, cfg: IngestConfig, world: int, make, piece_bytes: int | None = None):
    """`batches`: host uint8 tensors (the global batches, whole segments except the last).  -> (ranks, steps): `make(capacity, nominal
    piece, rank)` built the ranks; `steps` yields, per global batch, the ranks' piece sizes once the pieces lie in the ranks' buffers,
    and advances the ranks' fill when the caller comes back for the next batch (after it ran the batch's phases)."""
    seg = cfg.seg_size
    bounds = [deal_batch(b.numel(), world, seg) for b in batches]
    pb = piece_bytes or max(max(bd[r + 1] - bd[r] for r in range(world)) for bd in bounds)
    pb = -(-pb // seg) * seg
    local_total = [sum(bd[r + 1] - bd[r] for bd in bounds) for r in range(world)]
    ranks = [make(max(local_total[r], 1), pb, r) for r in range(world)]
    for s in ranks:
        s.lockstep = True

    def steps():
        for b, bd in zip(batches, bounds):
            ns = [bd[r + 1] - bd[r] for r in range(world)]
            for r, (n, s) in enumerate(zip(ns, ranks)):
                if n:
                    s.data[s.n_bytes: s.n_bytes + n].copy_(b[bd[r]: bd[r + 1]])
            yield ns
            for n, s in zip(ns, ranks):
                s.n_bytes += n
    return ranks, steps()


def serve_requests(ranks: list, counts: list, slots: torch.Tensor):
    """What the routed fetch delivers to one requester: `counts[r]` of its `slots` (grouped by owner, rank order) are stored slots of
    rank r, served by that rank's `serve`.  -> (bytes, lens) in request order."""
    dev = slots.device
    parts, lens, o = [], [], 0
    for owner, cnt in enumerate(counts):
        if cnt:
            by, ln = ranks[owner].serve(slots[o: o + cnt])
            parts.append(by); lens.append(ln); o += cnt
    return (torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8, device=dev),
            torch.cat(lens) if lens else torch.empty(0, dtype=torch.int64, device=dev))
