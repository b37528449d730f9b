/*
 * hmse.h — C-ABI of the MI355X-native HMSE ingest hot path (L2 -> L3 -> L4 -> L1).
 *
 * This is the drop-in boundary.  The reference (1Jamie/HMSE, README.md) defines no
 * plugin/FFI interface: it has single-buffer C signatures with caller-owned output
 * and status-int returns.  Each entry point below is the batch form
 * of one of those signatures and cites the reference lines it replaces.
 *
 * Conventions (all entry points):
 *   - every pointer marked DEVICE is a HIP device pointer on the current device;
 *     the caller owns every buffer; the library never allocates and never syncs
 *     (hipGraph-capturable), work is stream-ordered on `stream` (a hipStream_t
 *     passed as void* so this header needs no HIP include);
 *   - return 0 = HMSE_OK, <0 = HMSE_E*;  counts that are only known on the device
 *     (n_cuts, overflow flags, stream lengths) are written to DEVICE memory;
 *   - one stream = one engine thread (README.md:148-153, "Core 1 HMSE engine").
 *   - integer/byte results are bit-exact against oracle/ (tests/).
 *
 * Memory (all entry points; pinned by tests/test_gpu_arguments_only.py):
 *   - a byte-typed pointer (const uint8_t* / uint8_t* / void* records: data, streams, out, raw_out, blob, digests, kind, ok, ...)
 *     may have ANY alignment; a typed pointer (u32 / u64 / i64 arrays) needs the natural alignment of its element, no more;
 *   - a workspace (`ws`) is 256-byte aligned: an entry point given another one returns HMSE_EINVAL before it clears or launches
 *     anything;
 *   - what a workspace or an output holds before the call never matters — the library clears what it needs cleared and writes
 *     every element the call declares valid (statuses, counts, and per-element outputs such as kind[], ok[], out_off[] in full):
 *     NO argument has to be cleared by the caller.  An output sized for a worst case is written up to the count the call returns
 *     and left as it was behind it (cuts beyond n_cuts, out beyond out_off[n_sel], the hmse_gc_plan arrays beyond counts[],
 *     ranges of hmse_scrub_attribute beyond counts[0] pairs): read the count, not the rest.  The two exceptions are state the
 *     caller carries from call to call and says so: the workspace of a stream between hmse_stream_workspace_init and its batches, and the persistent tables of hmse_l3_index_update / hmse_l4_lsh_update
 *     (cleared by the call with n_old == 0), with the arrays and the state block they index (of a stream's arrays, hmse_stream, the
 *     first batch reads cuts[0] and stream_off[0], the start of the first chunk and of the first record: 0);
 *   - nothing outside [p, p + declared size) is read with effect or written: the bytes behind n / streams_bytes / blob_bytes
 *     and around every output may be anything and are left as they are.
 */
#ifndef HMSE_H
#define HMSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: the streaming entry points (hmse_stream_batch, hmse_stream_piece_*) take a stream's persistent arrays as ONE descriptor
 * (hmse_stream) instead of some twenty positional pointers and capacities, of which two of one type in swapped order compiled, loaded
 * and ran; the words and status bits of the state block are named here (HMSE_SB_*, HMSE_STREAM_ST_*).  No layout or result changed.
 * 2 (round 4): contracts of existing entry points changed in round 3 — hmse_stream_batch / hmse_stream_piece_* need a workspace
 * prepared by hmse_stream_workspace_init (else HMSE_STREAM_ST_WS_INIT) and take the global chunk count from state[HMSE_SB_G_OLD] (one
 * rank: it must equal state[HMSE_SB_N_OLD]; a mismatch is HMSE_STREAM_ST_STATE); hmse_l1_deflate keeps ONE record per chunk in its
 * workspace (hmse_l1_deflate_record_bytes / _dict).  A caller built against another version must check hmse_abi_version() and refuse. */
#define HMSE_ABI_VERSION 3

enum {
  HMSE_OK      = 0,
  HMSE_EINVAL  = -1, /* bad argument / unsupported configuration              */
  HMSE_ENOSPC  = -2, /* a caller-provided buffer or workspace is too small     */
  HMSE_EHIP    = -3  /* a HIP runtime call failed (launch error)               */
};

/* stage ids for hmse_workspace_bytes() */
enum {
  /* export as gzip (hmse_crc32, hmse_gzip_members: no workspace, 0 bytes); profile slots of their own */
  HMSE_STAGE_EXPORT_CRC     = 0,
  HMSE_STAGE_EXPORT_MEMBERS = 1,
  HMSE_STAGE_L2_CDC     = 2,
  HMSE_STAGE_L3_SHA256  = 3,
  HMSE_STAGE_L3_DEDUP   = 4,
  HMSE_STAGE_L4_MINHASH = 5,
  HMSE_STAGE_L4_LSH     = 6,
  HMSE_STAGE_L1_DEFLATE = 7,
  /* read path; ids 8..15 are the DEFLATE kernels' profiling slots */
  HMSE_STAGE_L1_INFLATE    = 16,
  HMSE_STAGE_READ_ASSEMBLE = 17,
  HMSE_STAGE_MANIFEST_PACK = 18,
  /* replication (hmse_sync_match: no workspace, 0 bytes).  As a profile slot 19 is shared with the dictionary jobs of one DEFLATE
   * match-kernel class (see hmse_profile_read): reset it before timing a comparison */
  HMSE_STAGE_SYNC_MATCH    = 19,
  /* garbage collection of dropped segments (hmse_gc_plan; hmse_record_gather's profiling slot) */
  HMSE_STAGE_GC_PLAN       = 24,
  HMSE_STAGE_RECORD_GATHER = 25,
  /* near-duplicate search over the stored chunks' signatures (hmse_l4_index_build: n = stored chunks; hmse_l4_query: n = queries) */
  HMSE_STAGE_L4_INDEX      = 26,
  HMSE_STAGE_L4_QUERY      = 27,
  /* scrub of a store (hmse_scrub_records: no workspace, 0 bytes; hmse_scrub_attribute: n = max(records, chunks)) */
  HMSE_STAGE_SCRUB_RECORDS   = 28,
  HMSE_STAGE_SCRUB_ATTRIBUTE = 29,
  /* exact search (hmse_find_*: no workspace, 0 bytes).  As profile slots 30 and 31 are shared with the DELTA encode kernels of
   * hmse_l1_deflate (see hmse_profile_read): reset them before timing a search */
  HMSE_STAGE_FIND_SCAN       = 30,
  HMSE_STAGE_FIND_PLACE      = 31
};

/* layer-enable mask == the reference's ablation matrix / degradation modes
 * (VALIDATION_METHODS.md:458-464, README.md:745-770).                          */
enum {
  HMSE_LAYER_L1 = 1u, /* DEFLATE                */
  HMSE_LAYER_L2 = 2u, /* content-defined chunks */
  HMSE_LAYER_L3 = 4u, /* SHA-256 exact dedupe   */
  HMSE_LAYER_L4 = 8u  /* MinHash/LSH + delta    */
};

/* chunk kinds in the manifest (README.md:1635-1669) */
enum { HMSE_KIND_FULL = 0, HMSE_KIND_POINTER = 1, HMSE_KIND_DELTA = 2 };

/*
 * Configuration: mirrors the reference's compile-time constants
 * (README.md:2354-2355, 2444-2447, 2575-2576; SURVEY.md §5 "Config / flags").
 */
typedef struct hmse_cfg {
  uint32_t struct_size;  /* sizeof(hmse_cfg), ABI check                               */
  /* L2 — FASTCDC_MIN/AVG/MAX_SIZE (README.md:2444-2446), defaults 2048/8192/32768    */
  uint32_t min_size;     /* >= 64 (the Gear window)                                   */
  uint32_t avg_size;     /* power of two                                              */
  uint32_t max_size;     /* <= 32768 (uint16_t length in ChunkIndex, README.md:1267)  */
  uint32_t norm_level;   /* FastCDC normalisation: masks use log2(avg) +/- norm bits  */
  uint32_t seg_size;     /* resolve restarts every seg_size bytes (default 4 MiB)     */
  /* L4 — NUM_HASHES (README.md:2575), 4-byte shingles (README.md:2584-2586)          */
  uint32_t n_hashes;     /* 128                                                       */
  uint32_t shingle;      /* 4                                                         */
  uint32_t seed_base;    /* seeds are seed_base + 0..n_hashes-1 (README.md:2589-2591) */
  uint32_t bands;        /* b = 4  (README.md:1987-1996)                              */
  uint32_t rows;         /* r = 32, bands*rows == n_hashes                            */
  uint32_t band_bits;    /* 16 -> 65536 buckets per band (README.md:1937-1945)        */
  /* L1 — mz_deflateInit2(&s, 9, MZ_DEFLATED, 15, 9, ...) (README.md:2374)            */
  uint32_t level;        /* 1..9 profile; selects chain_depth when that is 0          */
  uint32_t chain_depth;  /* candidates examined per position (0 = from level)         */
  uint32_t layers;       /* HMSE_LAYER_* mask                                         */
  uint32_t delta_max_ratio_pct; /* optional gate: delta <= pct% of chunk (0 = off)    */
} hmse_cfg;

/* Fill *cfg with the defaults above. */
void hmse_cfg_default(hmse_cfg* cfg);
/* 0 if the configuration is supported by the device path, HMSE_EINVAL otherwise. */
int hmse_cfg_validate(const hmse_cfg* cfg);

int hmse_abi_version(void);
const char* hmse_strerror(int code);

/* The 256-entry Gear table (host copy), generated from a fixed seed. */
void hmse_gear_table(uint64_t table[256]);

/* Bytes of DEVICE workspace stage `stage` needs for an input of n bytes
 * (L2) or n chunks (all other stages). */
size_t hmse_workspace_bytes(int stage, uint64_t n, const hmse_cfg* cfg);

/*
 * L2 — content-defined chunking.  Replaces rabin_slide() + the cut loop of
 * benchmark_fastcdc() (README.md:2456-2464, 2475-2490): rolling state never reset at
 * a cut, cut iff size >= MIN && (hash hit || size >= MAX); Gear roll + two-mask
 * normalisation; resolution restarts at every segment boundary.
 *   data     DEVICE u8[n]
 *   seg_off  DEVICE u64[n_seg+1], ascending, seg_off[0]=0, seg_off[n_seg]=n
 *   cuts     DEVICE u64[cuts_cap]: receives cuts[0]=0 and then every chunk END offset
 *   n_cuts   DEVICE u64[1]: number of chunks (cuts holds n_cuts+1 entries).
 *            If the required count exceeds cuts_cap-1 nothing past cuts_cap is
 *            written and n_cuts still receives the required count.
 *   status   DEVICE u32[1]: 0 ok, bit0 = candidate workspace overflow,
 *            bit1 = cuts_cap overflow
 *   ws       hmse_workspace_bytes(HMSE_STAGE_L2_CDC, n, cfg) provisions a candidate list of 8x the expected density of
 *            easy-mask hits plus 65536 entries.  The list is sized from ws_bytes: whatever the caller passes beyond
 *            that goes to it, up to one entry per byte.  Ordinary bytes can be denser than provisioned (a run of two
 *            alternating bytes whose window hash passes the easy mask makes every second position a candidate): the
 *            call then reports bit0 and its cuts are not to be used; the same call with
 *            hmse_workspace_bytes(...) + 4 * n + 256 bytes cannot overflow and gives the cuts (hmse_amd/ops.py::l2_cdc
 *            does exactly this, once).  The default size does not grow.
 */
int hmse_l2_cdc(const uint8_t* data, uint64_t n, const uint64_t* seg_off, uint32_t n_seg,
                const hmse_cfg* cfg, uint64_t* cuts, uint64_t cuts_cap, uint64_t* n_cuts,
                uint32_t* status, void* ws, size_t ws_bytes, void* stream);

/*
 * L3 — SHA-256 of every chunk.  Replaces mbedtls_sha256(data, len, hash, 0)
 * (README.md:2543), applied to the raw chunk.
 *   cuts     DEVICE u64[n_chunks+1]
 *   digests  DEVICE u8[n_chunks][32]
 */
int hmse_l3_sha256(const uint8_t* data, uint64_t n, const uint64_t* cuts, uint64_t n_chunks,
                   uint8_t* digests, void* ws, size_t ws_bytes, void* stream);

/*
 * L3 — exact dedupe.  Replaces the hash-index probe/insert of README.md:1288-1292,
 * 1542-1551 on a table held whole in HBM.
 *   first_occ DEVICE u64[n_all]: index of the earliest chunk with an equal digest
 *   refcount  DEVICE u32[n_all]: at a first occurrence, number of chunks equal to it
 *             (ChunkIndex.refcount, README.md:1269); 0 elsewhere
 */
int hmse_l3_dedup(const uint8_t* digests_all, uint64_t n_all, uint64_t* first_occ,
                  uint32_t* refcount, void* ws, size_t ws_bytes, void* stream);

/*
 * L3 persistent index (README.md:1288-1292, 1542-1551: "lookup -> found: pointer, refcount++ / new: insert"; sizing
 * README.md:1850-1894).  The table (DEVICE u32[slots], slots = hmse_l3_index_slots(capacity in chunks)) outlives the
 * call: digests [n_old, n_old + n_new) of digests_all join a table that already holds [0, n_old) and are looked up;
 * first_occ[n_old ..) and refcount (running counts, DEVICE u32[>= n_old + n_new]) are updated.  Earlier first
 * occurrences never change, so a batch costs O(n_new) whatever the history.  n_old == 0 clears the table first.
 * Returns HMSE_ENOSPC when the table would exceed load factor 0.5.
 */
uint64_t hmse_l3_index_slots(uint64_t capacity_chunks);
int hmse_l3_index_update(const uint8_t* digests_all, uint64_t n_old, uint64_t n_new, uint64_t* first_occ,
                         uint32_t* refcount, uint32_t* table, uint64_t slots, void* stream);

/*
 * L4a — MinHash signatures.  Replaces minhash_compute(const uint8_t*, size_t,
 * uint32_t*) (README.md:2578-2598): sig[h] = min over 4-byte shingles of
 * MurmurHash3_x86_32(shingle, 4, seed_base + h).
 *   chunk_ids DEVICE u64[n_sel]: chunks to sign (indices into cuts), or NULL = all
 *   sig       DEVICE u32[n_sel][n_hashes]
 *   ws        hmse_workspace_bytes(HMSE_STAGE_L4_MINHASH, n_sel, cfg) bytes hold the call's memo table (per shingle: which
 *             of its 128 hashes are small enough to matter; cleared at the start of every call, so a call depends on
 *             nothing but its arguments).  With a smaller workspace (>= 0 bytes) every hash is computed; the signatures
 *             are the same either way.
 * The table makes the call's TIME data-dependent: it pays where 4-byte shingles repeat across chunks (text: 90 % of the
 * lookups hit, 1.6x faster than without it); on data without repeating shingles (random bytes) the lookups are overhead and
 * a wavefront gives up after 256 of them per pass — measured 6 % slower than a call without workspace.
 * A caller that knows its data is incompressible passes ws_bytes = 0.
 */
int hmse_l4_minhash(const uint8_t* data, uint64_t n, const uint64_t* cuts,
                    const uint64_t* chunk_ids, uint64_t n_sel, const hmse_cfg* cfg,
                    uint32_t* sig, void* ws, size_t ws_bytes, void* stream);

/*
 * L4b — LSH banding (README.md:1375-1383, 1987-1996).  band key = MurmurHash3_x86_32
 * over the band's rows*4 bytes, seed = band index (bucket = key & (2^band_bits - 1));
 * base[i] = earliest j < i sharing a whole band with i, or -1.
 *   band_keys DEVICE u32[n_sel][bands]
 *   base      DEVICE i64[n_sel]  (indices into the selection)
 */
int hmse_l4_lsh(const uint32_t* sig, uint64_t n_sel, const hmse_cfg* cfg, uint32_t* band_keys,
                int64_t* base, void* ws, size_t ws_bytes, void* stream);

/*
 * L4b persistent band tables (README.md:1554-1576 "probe LSH ... none: insert signature", 1937-1945): tables DEVICE
 * u32[bands][slots], slots = hmse_l4_lsh_slots(capacity in stored chunks), outlive the call.  Signatures
 * [n_old, n_old + n_new) of sig_all join tables that already hold [0, n_old); band_keys[n_old ..) are written (or, with
 * keys_given != 0, taken as loaded from a stored band table) and base[n_old ..) = earliest chunk, old or new, sharing a
 * whole band (base may be NULL: insert only).  n_old == 0 clears the tables first.
 */
uint64_t hmse_l4_lsh_slots(uint64_t capacity_chunks);
int hmse_l4_lsh_update(const uint32_t* sig_all, uint64_t n_old, uint64_t n_new, const hmse_cfg* cfg, uint32_t* band_keys,
                       int64_t* base, uint32_t* tables, uint64_t slots, uint32_t keys_given, void* stream);

/*
 * L1 — per-chunk DEFLATE (RFC 1951 raw stream) with the LSH base chunk as preset
 * dictionary.  Replaces mz_deflateInit2(&s, 9, MZ_DEFLATED, 15, 9, ...) +
 * mz_deflate(&s, MZ_FINISH) (README.md:2374, 2378) and the delta rule of
 * README.md:1328, 2175.
 *   chunk_ids DEVICE u64[n_sel] or NULL = all;  base DEVICE i64[n_sel] or NULL
 *             (index into the selection of the dictionary chunk, -1 = none)
 *   out       DEVICE u8[out_cap]; chunk k's stream is out[out_off[k] .. out_off[k+1])
 *   out_off   DEVICE u64[n_sel+1]
 *   kind      DEVICE u8[n_sel]: HMSE_KIND_FULL or HMSE_KIND_DELTA
 *   status    DEVICE u32[1]: bit0 = out_cap overflow (out_off still exact), bit1 = workspace too small,
 *             bit2 = a selected chunk is longer than 32768 bytes and was not encoded: it gets an EMPTY record
 *             (out_off[k+1] == out_off[k], kind FULL) while every other chunk's record is complete and exact,
 *             bit3 = a chunk was never encoded (internal error)
 *   ws        hmse_workspace_bytes(HMSE_STAGE_L1_DEFLATE, n_sel, cfg) is the FIXED part; after it the call needs
 *             one record per chunk: hmse_l1_deflate_record_bytes(len) bytes (about 4*len + 1.4 KiB: histograms and a
 *             token list sized for the all-literal case, which the FULL stream later overwrites), or
 *             hmse_l1_deflate_record_bytes_dict(len) where base >= 0 (len + 21 more: the DELTA stream's own slot)
 */
int hmse_l1_deflate(const uint8_t* data, uint64_t n, const uint64_t* cuts,
                    const uint64_t* chunk_ids, const int64_t* base, uint64_t n_sel,
                    const hmse_cfg* cfg, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                    uint8_t* kind, uint32_t* status, void* ws, size_t ws_bytes, void* stream);

/* Bytes of workspace the record of a chunk of `chunk_len` bytes needs behind the fixed part — without / with a dictionary
 * (0 if chunk_len > 32768: such a chunk cannot be encoded — `uint16_t length`, README.md:1267). */
uint64_t hmse_l1_deflate_record_bytes(uint32_t chunk_len);
uint64_t hmse_l1_deflate_record_bytes_dict(uint32_t chunk_len);

/*
 * L1 with options (the streaming front end): as hmse_l1_deflate, plus
 *   flags  HMSE_DEFLATE_BASE_IS_CHUNK_ID: base[k] is a chunk index into `cuts` (any chunk of the resident data, e.g. one
 *          stored by an earlier batch) instead of an index into the selection.
 */
enum { HMSE_DEFLATE_BASE_IS_CHUNK_ID = 1u };
int hmse_l1_deflate_ex(const uint8_t* data, uint64_t n, const uint64_t* cuts, const uint64_t* chunk_ids,
                       const int64_t* base, uint64_t n_sel, const hmse_cfg* cfg, uint32_t flags, uint8_t* out,
                       uint64_t out_cap, uint64_t* out_off, uint8_t* kind, uint32_t* status, void* ws,
                       size_t ws_bytes, void* stream);

/*
 * Read path, L1 — raw DEFLATE decode of stored chunks.  Replaces mz_inflateInit2(&s, 15) + mz_inflate(&s, MZ_FINISH)
 * (README.md:2397-2400) and the FULL / DELTA branches of the read path (README.md:1635-1669, 2191-2198): a DELTA
 * record inflates with the raw bytes of its base chunk as preset dictionary (the last 32 KiB of them).
 *   streams    DEVICE u8[streams_bytes]
 *   stream_off DEVICE u64[n_sel+1] (dense: stream k = [off[k], off[k+1]))  or, with stream_len != NULL,
 *              DEVICE u64[n_sel] starts + stream_len DEVICE u32[n_sel] (records inside a manifest blob)
 *   kind       DEVICE u8[n_sel]  HMSE_KIND_FULL / HMSE_KIND_DELTA;  base DEVICE i64[n_sel] or NULL: slot of the
 *              dictionary chunk, must be < k (the writer only ever picks earlier chunks)
 *   raw_off    DEVICE u64[n_sel+1]: where each chunk's raw bytes go in raw_out (exclusive prefix sum of raw lengths)
 *   ok         DEVICE u8[n_sel] or NULL: 1 where chunk k decoded, 0 where its record is corrupt
 *   status     DEVICE u32[1]: bit0 = at least one record is corrupt (the streams stock zlib rejects: bad block type or
 *              code set, undefined code, distance beyond the window, stored LEN/NLEN mismatch; plus: decoded size !=
 *              recorded raw length, stream not ending in its last byte, DELTA with a missing/corrupt base) — that
 *              chunk's bytes are undefined, every other chunk is still decoded
 *   ws         hmse_workspace_bytes(HMSE_STAGE_L1_INFLATE, n_sel, cfg)
 */
int hmse_l1_inflate(const uint8_t* streams, uint64_t streams_bytes, const uint64_t* stream_off,
                    const uint32_t* stream_len, const uint8_t* kind, const int64_t* base, uint64_t n_sel,
                    const uint64_t* raw_off, uint8_t* raw_out, uint64_t raw_cap, uint8_t* ok,
                    uint32_t* status, void* ws, size_t ws_bytes, void* stream);

/*
 * Which decoder hmse_l1_inflate launches.  0 (default): by stream count — one stream per wavefront below 49152 streams
 * (a call lasts about as long as its longest stream), one stream per LANE from there on (four times the throughput
 * once the chip's 65 536 lanes are fed).  1 / 2 force the first / second.  Results are identical; process-wide.
 * No reference counterpart: mz_inflate (README.md:2397-2400) decodes one stream per call on one core.
 */
int hmse_l1_inflate_mode(int mode);

/*
 * Read path — POINTER branch and final layout (README.md:1635-1669): chunk i of the original data is the raw
 * bytes of stored slot slot_of_chunk[i] (its own slot for FULL/DELTA, the target's for POINTER).
 *   cuts DEVICE u64[n_chunks+1]; slot_of_chunk DEVICE u64[n_chunks]; raw_off DEVICE u64[n_slots+1]; raw DEVICE u8[]
 *   data_out DEVICE u8[n];  status DEVICE u32[1]: bit0 = a map entry disagrees with the stored lengths
 */
int hmse_read_assemble(const uint64_t* cuts, uint64_t n_chunks, const uint64_t* slot_of_chunk, uint64_t n_slots,
                       const uint64_t* raw_off, const uint8_t* raw, uint8_t* data_out, uint64_t n,
                       uint32_t* status, void* stream);

/*
 * The streaming front end: one batch as a single enqueue with NO host read (BASELINE.json configs[4]
 * "hipGraph-captured per-batch pipeline"; the reference's batch loop README.md:1519-1580: request block -> L2 -> per chunk
 * L3 lookup/insert -> L4 probe -> delta or full).
 *
 * The state block: DEVICE u64[HMSE_SB_WORDS], read by every stage of the chain instead of host-side counts and advanced by the chain
 * itself, so a batch can be captured into a hipGraph once per batch size and replayed for every batch.  The caller writes it whole
 * before the first batch (a fresh stream: zeros) and reads it when it wants the counts.
 */
enum {
  HMSE_SB_OFF    = 0,   /* byte offset of this batch in the resident data (= bytes ingested before it) */
  HMSE_SB_N_OLD  = 1,   /* this rank's chunks before this batch */
  HMSE_SB_N_NEW  = 2,   /* ... of this batch (out) */
  HMSE_SB_U_OLD  = 3,   /* this rank's stored chunks before this batch (a gstate block: of ALL ranks) */
  HMSE_SB_U_NEW  = 4,   /* ... of this batch (out) */
  HMSE_SB_S_OLD  = 5,   /* stream bytes before this batch */
  HMSE_SB_S_NEW  = 6,   /* ... of this batch (out) */
  HMSE_SB_STATUS = 7,   /* sticky HMSE_STREAM_ST_* bits */
  /* the global chunk order of a multi-rank stream (batch, rank, local index); with one rank these mirror N_OLD / N_NEW */
  HMSE_SB_G_OLD  = 8,   /* chunks of ALL ranks before this batch (one rank: must equal [HMSE_SB_N_OLD]) */
  HMSE_SB_G_NEW  = 9,   /* ... in this batch (out) */
  HMSE_SB_G_BASE = 10,  /* global index of this rank's first chunk of this batch (out; a gstate block: global STORED index of its first new chunk) */
  HMSE_SB_WORDS  = 16
};
/*
 * state[HMSE_SB_STATUS].  Once it is non-zero the failing batch has been dropped and every later call is a no-op (counters frozen at
 * the last good batch): nothing is ever appended to an index that is no longer consistent.
 */
#define HMSE_STREAM_ST_CHUNK_CAP    1ull    /* chunk capacity (max_chunks, max_chunks_g, or more chunks than the batch's cut list holds) */
#define HMSE_STREAM_ST_STORED_CAP   2ull    /* stored-chunk capacity (max_unique, g->max_stored_g) */
#define HMSE_STREAM_ST_L2           4ull    /* L2 status: the chain cannot run a batch twice, so a batch with more cut candidates than its fixed
                                               list holds (see hmse_l2_cdc) is refused, no cut of it is published; such bytes go through hmse_l2_cdc
                                               with the larger workspace */
#define HMSE_STREAM_ST_ROW          8ull    /* malformed exchange row (a count beyond the row's capacity) */
#define HMSE_STREAM_ST_WS_INIT      16ull   /* workspace not initialised (hmse_stream_workspace_init) */
#define HMSE_STREAM_ST_STATE        32ull   /* state block inconsistent: one rank and [HMSE_SB_G_OLD] != [HMSE_SB_N_OLD], e.g. a stream resumed with
                                               the version-1 state layout, whose word 8 is 0 */
#define HMSE_STREAM_ST_PUSH_REFUSED 64ull   /* set by the CALLER: a piece refused by its feeder */
#define HMSE_STREAM_ST_SIG_ROW      128ull  /* more new stored chunks than a signature row holds */
#define HMSE_STREAM_ST_DEFLATE_SHIFT 8      /* bits 8..: the status word of hmse_l1_deflate, shifted */
#define HMSE_STREAM_ST_HOST_REFUSED (1ull << 16)  /* set by the CALLER: a refusal on the host between two phases of a batch */

/*
 * What is fixed for a stream's life: its persistent arrays and their capacities.  The struct is read on the HOST, during the call only;
 * its pointers are copied into kernel arguments, so a captured graph keeps them.  The arrays must outlive the stream (and every graph
 * captured from it), the struct need not.  Each entry point names the fields it requires; a required field that is NULL, a struct_size
 * other than sizeof(hmse_stream), a world outside 1..256 or rank >= world is HMSE_EINVAL before anything is enqueued.
 * With several ranks (hmse_stream_piece_*), cuts / uniq / sig / band_keys / base / lsh_tables / kind / stream_off / out are THIS RANK's
 * arrays (chunk ids are local) and digests / first_occ / refcount / l3_table the GLOBAL ones, identical on every rank.  Of the arrays
 * the first batch reads cuts[0] and stream_off[0], the start of the first chunk and of the first record: 0.
 */
typedef struct hmse_stream {
  uint32_t struct_size, world, rank, reserved;   /* one-rank stream: world 1, rank 0 */
  uint64_t* state;                               /* u64[HMSE_SB_WORDS] */
  uint64_t* cuts;        uint64_t max_chunks;    /* u64[max_chunks + 1]: chunk bounds (stream offsets) */
  uint64_t* gidx;                                /* local -> global chunk index; may be NULL when world == 1 */
  uint8_t*  digests;     uint64_t max_chunks_g;  /* u8[max_chunks_g][32], global chunk order; one rank: == max_chunks */
  uint64_t* first_occ;   uint32_t* refcount;     /* [max_chunks_g], as hmse_l3_index_update */
  uint32_t* l3_table;    uint64_t l3_slots;      /* hmse_l3_index_slots(max_chunks_g), cleared by hmse_l3_index_update(n_old = n_new = 0) */
  uint64_t* uniq;        uint64_t max_unique;    /* u64[max_unique]: chunk ids of the stored chunks, ascending */
  uint32_t* sig;         uint32_t* band_keys;    int64_t* base;   /* [max_unique][128], [max_unique][bands], [max_unique]: stored slot of the dictionary, -1 none */
  uint32_t* lsh_tables;  uint64_t lsh_slots;     /* u32[bands][lsh_slots], hmse_l4_lsh_slots(max_unique), cleared by hmse_l4_lsh_update(n_old = n_new = 0) */
  uint8_t*  kind;        uint64_t* stream_off;   /* u8[max_unique], u64[max_unique + 1] */
  uint8_t*  out;         uint64_t out_cap;       /* the DEFLATE streams, record k at out[stream_off[k] ..) */
} hmse_stream;

/*
 * hmse_stream_batch: one batch of a ONE-RANK stream (s->world must be 1; requires every field of *s but gidx).  The batch's bytes are
 * already at data[state[HMSE_SB_OFF] .. + batch_bytes); grids and workspace are sized for batch_bytes / min_size chunks, and the call
 * ends by advancing the OFF, N_OLD, U_OLD, S_OLD and G_OLD words.  Appends to the per-chunk arrays of the stream, to the persistent L3
 * table / L4 band tables, and writes the batch's DEFLATE streams to out[state[HMSE_SB_S_OLD] ..).
 * seg_off DEVICE u64[n_seg+1]: batch-local segment offsets.  ws: hmse_stream_batch_workspace_bytes(batch_bytes, cfg), prepared ONCE
 * with hmse_stream_workspace_init() and then handed to every batch of the stream unchanged: it holds the MinHash memo table, which
 * persists across the batches (a cache of a pure function of (shingle, cfg->seed_base); cleared per batch it cost every 1 GiB batch
 * its warm-up again).  A chain that finds the workspace untagged drops the batch with HMSE_STREAM_ST_WS_INIT.
 */
uint64_t hmse_stream_batch_workspace_bytes(uint64_t batch_bytes, const hmse_cfg* cfg);
int hmse_stream_workspace_init(void* ws, size_t ws_bytes, uint64_t batch_bytes, const hmse_cfg* cfg, void* stream);
int hmse_stream_batch(uint8_t* data, uint64_t data_cap, uint64_t batch_bytes, const uint64_t* seg_off, uint32_t n_seg,
                      const hmse_cfg* cfg, const hmse_stream* s, void* ws, size_t ws_bytes, void* stream);

/*
 * The same chain for a stream that is sharded over several ranks (one process per GPU; BASELINE.json configs[4] "4 x 10 GB
 * streamed, 8 x MI355X, hipGraph-captured per-batch pipeline").  A global batch is dealt to the ranks as contiguous runs of
 * whole segments ("pieces", rank order = stream order inside the batch), so the GLOBAL CHUNK ORDER is (batch, rank, local
 * index) and equals the natural order of the concatenated stream.  The reference's per-chunk "L3 lookup -> found: pointer /
 * new: insert" (README.md:1538-1551) against ONE index becomes, per batch: phase A on every rank, ONE all-gather of the ranks'
 * exchange rows (RCCL over xGMI; the caller's job — this library never communicates), phase B on every rank.  Every rank
 * keeps a replica of the global digest array and of the L3 table and applies the same order-independent first-occurrence rule
 * to the same rows, so dedupe is that of the one-rank stream; L4 bases and dictionaries are scoped to the rank (the bytes
 * must be resident), exactly as in the sharded one-shot ingest.
 *   cap_bytes    the NOMINAL piece size of the stream (>= every piece_bytes): it alone sizes rows, grids and the workspace, so
 *                that every rank's row has the same layout whatever its piece holds (a rank may get 0 bytes in the last batch)
 *   row          DEVICE u8[hmse_stream_row_bytes(cap_bytes)]: {u64 n_chunks, 24 B zero, n_chunks x 32 B digests, unused tail}
 *   rows         DEVICE u8[world][row bytes]: the all-gathered rows in rank order (world == 1: rows == row)
 *   s            hmse_stream_piece_hash requires state and cuts; hmse_stream_piece_encode every field (gidx when world > 1).
 *                state: N_OLD .. S_NEW count this rank's chunks / stored chunks / stream bytes, G_OLD .. G_BASE the global ones
 *   ws           hmse_stream_batch_workspace_bytes(cap_bytes, cfg); both phases of a batch take the SAME workspace
 * Both calls are stream-ordered and capturable; hmse_stream_batch == hash + encode with world 1 on the row in its workspace.
 */
uint64_t hmse_stream_row_bytes(uint64_t cap_bytes, const hmse_cfg* cfg);
int hmse_stream_piece_hash(uint8_t* data, uint64_t data_cap, uint64_t piece_bytes, uint64_t cap_bytes, const uint64_t* seg_off,
                           uint32_t n_seg, const hmse_cfg* cfg, const hmse_stream* s, uint8_t* row, void* ws, size_t ws_bytes,
                           void* stream);
int hmse_stream_piece_encode(uint8_t* data, uint64_t data_cap, uint64_t piece_bytes, uint64_t cap_bytes, const hmse_cfg* cfg,
                             const hmse_stream* s, const uint8_t* rows, void* ws, size_t ws_bytes, void* stream);

/*
 * Global L4 for a multi-rank stream as captured phases (round 4; SURVEY.md §8f-3: "cross-GPU base-chunk fetch over xGMI P2P for global L4
 * (config 5)"; the reference keeps ONE set of band tables, README.md:1375-1383).  The stored chunks of all ranks are numbered in global
 * stored order (batch, rank, local); every rank holds the same signature array, band tables and owner map of that numbering and therefore
 * finds, for each of its chunks, the dictionary that ONE rank ingesting the whole stream would find.  Phase B of a batch becomes three
 * enqueue-only calls around two more exchange steps:
 *   hmse_stream_piece_sign      rows of all ranks (as for hmse_stream_piece_encode) -> global index -> this rank's new stored chunks ->
 *                               MinHash -> sig_row {u64 count, u64 first local stored slot, 16 B pad, sig_cap x 512 B}, sig_cap = the row's chunk capacity
 *                               (hmse_stream_sig_cap: the worst-case chunk count of a piece, as in the digest row)
 *   -- all-gather of the signature rows (fixed size: hmse_stream_sig_row_bytes) --
 *   hmse_stream_piece_bases     sig rows -> global signature array + owner map -> global band tables -> for every new stored chunk of
 *                               this rank its dictionary: a chunk of this rank, or a REMOTE one -> request (owner, owner's stored slot);
 *                               g->req_counts[q] requests to rank q, then two more words (HMSE_GL4_REQ_*), g->req_slots grouped by owner
 *   -- the requested chunks are fetched (all-to-all; the caller writes the bytes behind its data and their bounds into
 *      s->cuts[g->ghost_chunk0 ..]: request j is chunk ghost_chunk0 + j) --
 *   hmse_stream_piece_encode_g  DEFLATE of the new stored chunks with those dictionaries, tails, both state blocks advanced
 * Required fields of *s: sign — state, cuts, digests, first_occ, refcount, l3_table, uniq, sig (gidx when world > 1); bases — state, uniq,
 * band_keys, base (and s->world == g->world, s->rank == g->rank); encode_g — state, cuts, kind, stream_off, out.
 * gstate: DEVICE u64[HMSE_SB_WORDS], word [HMSE_SB_U_OLD] = stored chunks of ALL ranks before this batch, [HMSE_SB_U_NEW] = of this batch
 * (out), [HMSE_SB_G_BASE] = global stored index of this rank's first new chunk (out).  Status bits as hmse_stream_batch; HMSE_STREAM_ST_SIG_ROW
 * is a defence against a row that another build wrote (sig_cap is the worst-case chunk count of a piece, cap_bytes / min_size + segments
 * + 2, so phase A's own bound fires first).  HMSE_STREAM_ST_PUSH_REFUSED (a piece refused by the caller's feeder) and
 * HMSE_STREAM_ST_HOST_REFUSED (a refusal on the host between the phases of a batch: the fetch of the remote dictionaries, the ghost area,
 * a phase's return code) are set by the CALLER, before the next phase is enqueued, to drop the batch through the chain instead of
 * leaving the collectives alone.
 * All arrays are the caller's; sizes in the struct.
 */
enum {                       /* g->req_counts[world + ...], behind the per-rank counts */
  HMSE_GL4_REQ_TOTAL  = 0,   /* requests of this batch to all ranks */
  HMSE_GL4_REQ_STORED = 1,   /* this rank's stored chunks INCLUDING this batch's: the bound of the slots a peer may ask of it now */
  HMSE_GL4_REQ_EXTRA  = 2
};
typedef struct hmse_gl4 {
  uint32_t struct_size, world, rank, reserved;
  uint64_t sig_cap;        /* hmse_stream_sig_cap(cap_bytes, cfg) */
  uint64_t max_stored_g;   /* capacity of the global stored-chunk arrays */
  uint64_t* gstate;
  uint32_t* sig_g;         /* [max_stored_g][128] */
  uint32_t* band_keys_g;   /* [max_stored_g][bands] */
  int64_t*  base_g;        /* [max_stored_g] global stored index of the dictionary, -1 none */
  uint32_t* lsh_tables_g;  /* [bands][lsh_slots_g], cleared by hmse_l4_lsh_update(n_old = n_new = 0) */
  uint64_t  lsh_slots_g;
  uint32_t* g_owner;       /* [max_stored_g] owning rank */
  uint64_t* g_local;       /* [max_stored_g] the owner's stored slot */
  uint64_t* ug;            /* [max_unique] this rank's stored chunks: global stored index (out, appended) */
  int64_t*  base_global;   /* [max_unique] this rank's stored chunks: base_g (out, appended) */
  uint64_t* req_counts;    /* DEVICE u64[world + HMSE_GL4_REQ_EXTRA] (out) */
  uint64_t* req_slots;     /* DEVICE u64[cap chunks of a piece] (out) */
  uint64_t  ghost_chunk0;  /* chunk id of the batch's first fetched dictionary */
} hmse_gl4;
uint64_t hmse_stream_sig_cap(uint64_t cap_bytes, const hmse_cfg* cfg);
uint64_t hmse_stream_sig_row_bytes(uint64_t cap_bytes, const hmse_cfg* cfg);
int hmse_stream_piece_sign(uint8_t* data, uint64_t data_cap, uint64_t piece_bytes, uint64_t cap_bytes, const hmse_cfg* cfg, const hmse_stream* s,
                           const uint8_t* rows, uint8_t* sig_row, void* ws, size_t ws_bytes, void* stream);
int hmse_stream_piece_bases(uint64_t cap_bytes, const hmse_cfg* cfg, const hmse_stream* s, const uint8_t* sig_rows, const hmse_gl4* g,
                            void* ws, size_t ws_bytes, void* stream);
int hmse_stream_piece_encode_g(uint8_t* data, uint64_t data_cap, uint64_t piece_bytes, uint64_t cap_bytes, const hmse_cfg* cfg,
                               const hmse_stream* s, uint64_t* gstate, void* ws, size_t ws_bytes, void* stream);

/*
 * Chunk manifest — the packed on-disk records, written on the GPU (README.md:1263-1270 ChunkIndex 40 B, 2182-2189
 * DeltaChunk 8-byte header + delta data, 1312 pointer 8 B, 1448 per-chunk map, 1635-1669 chunk types).  Replaces the
 * reference's per-chunk "write chunk, insert (sha -> lba, len)" / "pointer record, refcount++" steps of the batch loop
 * (README.md:1542-1551) by one pass over a whole shard; the host only write()s the four arrays.
 *   streams/stream_off/kind/base/uniq_ids   the L1 outputs of the shard's n_unique stored chunks (base: slot index of the dictionary,
 *             -1 none, -2 = a dictionary stored on ANOTHER shard (global L4): the DeltaChunk header is packed unresolved, base_lba
 *             0xFFFFFFFF, and filled in when the shards' manifests are merged; base may be NULL when no record is a DELTA)
 *   digests DEVICE u8[n_chunks][32] or NULL, refcount DEVICE u32[n_chunks] or NULL, cuts DEVICE u64[n_chunks+1]
 *   first_occ DEVICE u64[n_chunks] GLOBAL index of each chunk's first occurrence (NULL: every chunk is its own);
 *             chunk_base = global index of this shard's chunk 0; shard / n_shards (<= 256); shard_bases DEVICE u64[n_shards]
 *             = chunk_base of every shard (NULL when n_shards == 1)
 *   rec_off   DEVICE u64[n_unique+1]: byte offset of each record in the blob (multiples of lba_unit, a power of two; the
 *             record = 8-byte DeltaChunk header for DELTA + the stream); ptr_index DEVICE u64[n_chunks]: number of
 *             POINTER chunks before chunk i
 *   blob      DEVICE u8[blob_bytes]; index DEVICE 40 B x n_unique; chunk_map DEVICE 8 B x n_chunks
 *             {slot u32, raw_length u16, kind u8, shard u8}; pointers DEVICE 8 B x n_pointers
 *             {target_lba u32, target_length u16, flags u16 = HMSE_KIND_POINTER | shard << 4 | 0x8000 if unresolved}.
 *             A chunk whose first occurrence lives on another shard gets slot = that shard's LOCAL chunk index and an
 *             unresolved pointer record (target_lba 0xFFFFFFFF): the merge of the per-shard manifests fills them in.
 *   status    DEVICE u32[1]: bit0 record does not fit (slot, 32-bit lba or 16-bit length), bit1 DELTA without an earlier
 *             base, bit2 first occurrence is not a stored chunk, bit3 forward / unknown cross-shard target, bit4 pointer overflow,
 *             bit5 a stored-chunk id (uniq_ids) outside the shard
 *   ws        hmse_workspace_bytes(HMSE_STAGE_MANIFEST_PACK, n_chunks, cfg)
 */
int hmse_manifest_pack(const uint8_t* streams, const uint64_t* stream_off, const uint8_t* kind, const int64_t* base,
                       const uint64_t* uniq_ids, uint64_t n_unique, const uint8_t* digests, const uint32_t* refcount,
                       const uint64_t* cuts, uint64_t n_chunks, const uint64_t* first_occ, uint64_t chunk_base,
                       uint32_t shard, const uint64_t* shard_bases, uint32_t n_shards, const uint64_t* rec_off,
                       uint32_t lba_unit, const uint64_t* ptr_index, uint8_t* blob, uint64_t blob_bytes, void* index,
                       void* chunk_map, void* pointers, uint64_t n_pointers, uint32_t* status, void* ws, size_t ws_bytes,
                       void* stream);
/* With options: HMSE_MANIFEST_ANY_SHARD_TARGET — a chunk's first occurrence may live on ANY other shard, also a later one.  The
 * shards of a multi-rank stream interleave in stream order (hmse_stream_piece_encode), so the rank that met a chunk first is not
 * always the lower-numbered one; the caller passes first_occ / chunk_base / shard_bases in the STORE numbering (shard, local
 * index) — hmse_amd/stream_dist.py::store_results.  Without the flag a forward target is an error (status bit3), as in a
 * one-shot sharded ingest, where dedupe only ever points backwards. */
enum { HMSE_MANIFEST_ANY_SHARD_TARGET = 1u };
int hmse_manifest_pack_ex(const uint8_t* streams, const uint64_t* stream_off, const uint8_t* kind, const int64_t* base,
                          const uint64_t* uniq_ids, uint64_t n_unique, const uint8_t* digests, const uint32_t* refcount,
                          const uint64_t* cuts, uint64_t n_chunks, const uint64_t* first_occ, uint64_t chunk_base,
                          uint32_t shard, const uint64_t* shard_bases, uint32_t n_shards, uint32_t flags,
                          const uint64_t* rec_off, uint32_t lba_unit, const uint64_t* ptr_index, uint8_t* blob,
                          uint64_t blob_bytes, void* index, void* chunk_map, void* pointers, uint64_t n_pointers,
                          uint32_t* status, void* ws, size_t ws_bytes, void* stream);

/*
 * Garbage collection, plan (the ChunkIndex refcount is kept "for garbage collection", README.md:1268, 1886): the chunk map of a
 * one-shard store and a set of dropped segments -> the L3 arrays of the store that holds only the surviving segments, numbered
 * as a fresh ingest of that remainder numbers them (a segment boundary is always a cut, so the surviving chunks keep their cuts).
 *   cuts        DEVICE u64[n_chunks+1] old chunk ends;  slot DEVICE u32[n_chunks] the old chunk map's index slot of each chunk
 *   seg_off     DEVICE u64[n_seg+1] the store's segment table (seg_off[n_seg] == cuts[n_chunks]); drop DEVICE u8[n_seg], 1 = dropped
 *   digests_old DEVICE u8[n_slots][32] the old ChunkIndex digests
 *   counts      DEVICE u64[2] out: {surviving chunks n_new, surviving slots u_new}
 *   old_chunk   DEVICE i64[n_chunks]: [k < n_new] old index of new chunk k
 *   first_occ   DEVICE i64[n_chunks], refcount DEVICE u32[n_chunks], digests DEVICE u8[n_chunks][32]: [k < n_new] as hmse_l3_dedup
 *               over the surviving digests (refcount counts the surviving references in the map, never the packed u16)
 *   uniq_ids    DEVICE i64[n_slots]: [j < u_new] new chunk index of new slot j (its first surviving reference, ascending)
 *   old_slot    DEVICE i64[n_slots]: [j < u_new] old slot of new slot j;  new_slot_of_old DEVICE i64[n_slots]: inverse, -1 = gone
 *   status      DEVICE u32[1]: bit0 = a map slot >= n_slots
 *   ws          hmse_workspace_bytes(HMSE_STAGE_GC_PLAN, n_chunks, cfg)
 */
int hmse_gc_plan(const uint64_t* cuts, uint64_t n_chunks, const uint32_t* slot, uint64_t n_slots, const uint64_t* seg_off,
                 uint32_t n_seg, const uint8_t* drop, const uint8_t* digests_old, uint64_t* counts, int64_t* old_chunk,
                 int64_t* first_occ, uint32_t* refcount, uint8_t* digests, int64_t* uniq_ids, int64_t* old_slot,
                 int64_t* new_slot_of_old, uint32_t* status, void* ws, size_t ws_bytes, void* stream);

/*
 * Garbage collection, records: the dense DEFLATE streams of the collected store from two sources in one launch (one wavefront
 * per record).  Record k is src_sel[k] ? src1 : src0, bytes [src_off[k], src_off[k] + dst_off[k+1] - dst_off[k]), copied to
 * dst[dst_off[k] ..).  src0 is typically the old blob (a reused record's stream, behind its DeltaChunk header; any byte
 * offset: lba_unit may be 1), src1 the hmse_l1_deflate output of the re-encoded records.
 *   src_off DEVICE u64[n]; src_sel DEVICE u8[n]; dst_off DEVICE u64[n+1]; dst DEVICE u8[dst_bytes]
 *   status  DEVICE u32[1]: bit0 = a record outside its source or the destination (that record is not copied)
 */
int hmse_record_gather(const uint8_t* src0, uint64_t src0_bytes, const uint8_t* src1, uint64_t src1_bytes, const uint64_t* src_off,
                       const uint8_t* src_sel, const uint64_t* dst_off, uint64_t n, uint8_t* dst, uint64_t dst_bytes,
                       uint32_t* status, void* stream);

/*
 * L4 band-table sidecar (hmse_amd/bandtable.py write_band_tables, byte for byte): file header, per band the header count, the
 * {band_hash u16, count u16} bucket headers in ascending band_hash order (a bucket of more than 65535 ids continues in further
 * headers) and the 3-byte ids, ascending inside a bucket; with n_hashes > 0 the "HMSESIGS" section (band keys, signatures).
 *   band_keys DEVICE u32[n][bands]; sig DEVICE u32[n][n_hashes] (may be NULL when n == 0 or n_hashes == 0)
 *   out       DEVICE u8[out_cap], out_cap >= hmse_band_tables_bound(n, bands, band_bits, n_hashes)
 *   out_bytes DEVICE u64[1] out: the exact size written
 *   status    DEVICE u32[1]: bit0 = n >= 2^24 (3-byte ids), bit1 = band_bits outside 1..16, bit2 = out_cap too small
 *   ws        hmse_band_tables_workspace_bytes(n) bytes
 * Buckets are built by a stable LSD radix sort per band: the bytes do not depend on the order of any atomic operation.
 */
uint64_t hmse_band_tables_bound(uint64_t n, uint32_t bands, uint32_t band_bits, uint32_t n_hashes);
size_t hmse_band_tables_workspace_bytes(uint64_t n);
int hmse_band_tables_write(const uint32_t* band_keys, uint64_t n, uint32_t bands, uint32_t band_bits, const uint32_t* sig,
                           uint32_t n_hashes, uint8_t* out, uint64_t out_cap, uint64_t* out_bytes, uint32_t* status, void* ws,
                           size_t ws_bytes, void* stream);

/*
 * Near-duplicate search (hmse_amd/similarity.py) over the MinHash signatures of the stored chunks.  A search banding is any cfg
 * that hmse_cfg_validate accepts (bands x rows == 128, bands in {1, 2, 4, 8, 16}); band b of a signature is hashes
 * [b rows, (b+1) rows).  Stored ids and query ids are row numbers of sig_s and sig_q.
 *
 * Index: per band, the stored ids sorted stably by their 32-bit band key (ids ascending inside equal keys), by the LSD radix sort
 * of hmse_band_tables_write (four 8-bit passes).
 *   keys        DEVICE u32[n][bands] the stored chunks' band keys under the search banding (hmse_l4_lsh)
 *   sorted_keys DEVICE u32[bands][n], sorted_ids DEVICE u32[bands][n] out
 *   status      DEVICE u32[1] out: 0 (no device-side failure exists; kept for the calling convention)
 *   ws          hmse_workspace_bytes(HMSE_STAGE_L4_INDEX, n, cfg) bytes
 * HMSE_EINVAL before any launch: bands not a power of two <= 16, n >= 2^32, a NULL pointer (keys / sorted_* may be NULL when n == 0).
 */
int hmse_l4_index_build(const uint32_t* keys, uint64_t n, uint32_t bands, uint32_t* sorted_keys, uint32_t* sorted_ids,
                        uint32_t* status, void* ws, size_t ws_bytes, void* stream);

/*
 * Query: stored id c is a CANDIDATE of query i iff some band of sig_q[i] equals the same band of sig_s[c], word by word (a band
 * key only routes the search: equal keys with different rows are no candidate).  score(i, c) = number of equal hashes (of 128;
 * the Jaccard estimate is score / 128).  Result of query i: its candidates with score >= min_score, by score descending, then
 * id ascending, the first top_k.
 *   sig_q   DEVICE u32[n_q][128];  keys_q DEVICE u32[n_q][bands] (hmse_l4_lsh under cfg)
 *   sig_s   DEVICE u32[n_s][128];  sorted_keys / sorted_ids from hmse_l4_index_build under the same banding
 *   cfg     the search banding (bands, rows)
 *   top_k   1..64;  min_score 0..128;  flags HMSE_QUERY_EXCLUDE_SELF: stored id i is no candidate of query i (self-join, sig_q == sig_s)
 *   out_ids DEVICE i64[n_q][top_k] (-1 padding);  out_scores DEVICE i32[n_q][top_k] (0 padding)
 *   n_hits  DEVICE u32[n_q] ids returned;  n_candidates DEVICE u64[n_q] candidates before min_score and top_k
 *   status  DEVICE u32[1] out: bit0 = an index entry names an id >= n_s (it is skipped)
 *   ws      hmse_workspace_bytes(HMSE_STAGE_L4_QUERY, n_q, cfg) bytes
 * HMSE_EINVAL before any launch: top_k or min_score out of range, an unsupported banding, unknown flags, n_q or n_s >= 2^32,
 * a NULL pointer (the query-side pointers may be NULL when n_q == 0, the stored-side ones when n_s == 0).
 */
enum { HMSE_QUERY_EXCLUDE_SELF = 1u };
int hmse_l4_query(const uint32_t* sig_q, const uint32_t* keys_q, uint64_t n_q, const uint32_t* sig_s, uint64_t n_s,
                  const uint32_t* sorted_keys, const uint32_t* sorted_ids, const hmse_cfg* cfg, uint32_t top_k, uint32_t min_score,
                  uint32_t flags, int64_t* out_ids, int32_t* out_scores, uint32_t* n_hits, uint64_t* n_candidates, uint32_t* status,
                  void* ws, size_t ws_bytes, void* stream);

/*
 * Scrub (hmse_amd/scrub.py): which records of a store are intact, and how far each damaged one reaches.  Records are numbered by
 * their GLOBAL slot: shard order, then index slot order.  Per-record flags (0 = good):
 *   STRUCTURE   the record is not inside its shard's blob, a DELTA record is shorter than its 8-byte header, its base_lba is not
 *               the LBA of an index entry of the shard its dictionary must be on (its own; remote_bases': exactly that entry),
 *               or a local dictionary does not come before it.  No dictionary is attributed.
 *   STREAM      structure fine, dictionary good, the decoder rejects the record (hmse_l1_inflate ok == 0)
 *   DIGEST      the record decodes, its SHA-256 is not the ChunkIndex sha256
 *   DICTIONARY  the record's dictionary is damaged (its own state is unknown)
 *   HEADER      base_length is not the dictionary's index length or delta_length is not the record length - 8 (loses nothing)
 *   METADATA    an inconsistency of the (trusted but checked) metadata touches the record
 */
enum {
  HMSE_SCRUB_STRUCTURE = 1u, HMSE_SCRUB_STREAM = 2u, HMSE_SCRUB_DIGEST = 4u, HMSE_SCRUB_DICTIONARY = 8u,
  HMSE_SCRUB_HEADER = 16u, HMSE_SCRUB_METADATA = 32u
};

/*
 * Scrub, records pass: one thread per record.  STRUCTURE / HEADER flags, the resolved dictionary, the non-zero padding bytes.
 *   blob        DEVICE u8[blob_bytes]: the shards' blobs back to back;  shard_blob DEVICE u64[n_shards+1] their offsets in it
 *   shard_slot  DEVICE u64[n_shards+1]: global slot of every shard's slot 0;  rec_shard DEVICE u32[n]: shard of every record
 *   lba_unit    DEVICE u32[n_shards];  lba DEVICE u32[n], rec_len DEVICE u32[n]: the ChunkIndex lba / length of every record
 *   kind        DEVICE u8[n] HMSE_KIND_* of every record (from the chunk map)
 *   remote      DEVICE i64[n]: -1, or the global slot remote_bases names as the record's dictionary
 *   sorted_lba  DEVICE u32[n], sorted_slot DEVICE u32[n]: per shard (the same segments as the slots) its LBAs ascending and the
 *               local slot of each;  steps = iterations of the binary search (bit length of the largest shard's record count)
 *   meta        DEVICE u8[n] flags found on the host (METADATA), OR-ed into status
 *   status      DEVICE u8[n] out;  dict DEVICE i64[n] out: global slot of the dictionary, -1 none / unresolved
 *   padding     DEVICE u64[1] out: non-zero bytes outside every record, the whole blob of a shard without records included (the
 *               packer writes zeros)
 * Shard bounds are clamped to blob_bytes.  Every value read from the blob is only compared, never used as an index.  No workspace
 * (hmse_workspace_bytes(HMSE_STAGE_SCRUB_RECORDS, ...) is 0).  n may be 0 with blob_bytes > 0: only the padding is counted.
 */
int hmse_scrub_records(const uint8_t* blob, uint64_t blob_bytes, uint64_t n, uint32_t n_shards, const uint32_t* rec_shard,
                       const uint64_t* shard_blob, const uint64_t* shard_slot, const uint32_t* lba_unit, const uint32_t* lba,
                       const uint32_t* rec_len, const uint8_t* kind, const int64_t* remote, const uint32_t* sorted_lba,
                       const uint32_t* sorted_slot, uint32_t steps, const uint8_t* meta, uint8_t* status, int64_t* dict,
                       uint64_t* padding, void* stream);

/*
 * Scrub, attribution: from the records pass's status / dict, the decoder's ok flags and the digests of the decoded records ->
 * final flags and roots.  root(k) = the furthest ancestor on k's dictionary chain (k included) whose own state is faulty, found by
 * pointer doubling in max_depth_log2 + 1 rounds (the caller cuts cycles and longer chains as METADATA); -1 for a good record.
 *   ok          DEVICE u8[n] (hmse_l1_inflate, in slot order);  got_sha / want_sha DEVICE u8[n][32] (check_digest == 0: no DIGEST)
 *   chunk_slot  DEVICE i64[n_chunks]: global slot of every chunk in corpus (stream) order, -1 = an inconsistent map entry
 *   cuts        DEVICE u64[n_chunks+1]: byte offset of every chunk
 *   status_out  DEVICE u8[n]; root DEVICE i64[n]; chunk_root DEVICE i64[n_chunks] (-1 good, -2 map entry inconsistent)
 *   root_records / root_chunks / root_bytes DEVICE u64[n]: per root (index = its slot) records, chunks and bytes lost
 *   ranges      DEVICE u64[2 (n_chunks / 2 + 1)]: the maximal runs of damaged chunks, (offset, length) pairs
 *   counts      DEVICE u64[8] out: ranges, damaged records, damaged chunks, damaged bytes, METADATA chunks, METADATA bytes,
 *               HEADER records, 0
 *   ws          hmse_workspace_bytes(HMSE_STAGE_SCRUB_ATTRIBUTE, max(n, n_chunks), cfg)
 */
int hmse_scrub_attribute(uint64_t n, const uint8_t* status, const int64_t* dict, const uint8_t* ok, const uint8_t* got_sha,
                         const uint8_t* want_sha, uint32_t check_digest, uint32_t max_depth_log2, uint64_t n_chunks,
                         const int64_t* chunk_slot, const uint64_t* cuts, uint8_t* status_out, int64_t* root, int64_t* chunk_root,
                         uint64_t* root_records, uint64_t* root_chunks, uint64_t* root_bytes, uint64_t* ranges, uint64_t* counts,
                         void* ws, size_t ws_bytes, void* stream);

/*
 * Exact search (hmse_amd/find.py): where does a byte string occur in a store?  Replaces what the reference layout leaves a user to do:
 * read the store back (README.md:1621-1675 per chunk), move the corpus to the host and loop over bytes.find() — which decodes and scans
 * every duplicate chunk once per occurrence.  Here a pattern is looked for once per stored RECORD (hmse_find_scan over the decoded
 * records of hmse_l1_inflate), every hit then belongs to every chunk that maps to that record (hmse_find_place), and only the
 * max(m) - 1 bytes in front of each chunk boundary are looked at through the chunk map (hmse_find_seams).
 *
 * Patterns: pat DEVICE u8[pat_off[n_pat]], pattern j = pat[pat_off[j] .. pat_off[j+1]); pat_off is a HOST u32[n_pat+1], read during
 * the call only (as the hmse_stream descriptor is): the lengths size the launch and are refused on the host.  1 <= n_pat <=
 * HMSE_FIND_MAX_PATTERNS, 1 <= length <= HMSE_FIND_MAX_LEN; equal patterns may repeat, each is answered on its own.  flags:
 * HMSE_FIND_IGNORE_CASE compares after folding the ASCII letters A-Z to a-z on both sides (every other value, >= 0x80 included,
 * compares exactly).  Overlapping occurrences all count.  HMSE_EINVAL before anything is cleared or launched: n_pat of 0 or above 32,
 * a pattern length of 0 or above 256, unknown flag bits, a NULL pointer to a non-empty array.
 * A hit is one u64: position << 8 | pattern index.
 *   hits    DEVICE u64[hits_cap] or NULL (hits == NULL or hits_cap == 0: count only); written in any order, up to min(n_hits, hits_cap)
 *   n_hits  DEVICE u64[1]: the exact number of hits, also when it exceeds hits_cap
 *   counts  DEVICE u64[n_pat]
 *   status  DEVICE u32[1]: bit0 = the hit list ran out (hits_cap > 0 and n_hits > hits_cap; n_hits and counts are still exact),
 *           bit1 = inconsistent tables: raw_off, cuts or chunk_out descending, raw_off[n_rec] > raw_bytes, slot[k] >= n_rec, a chunk
 *           whose length is not its record's.  With bit1 nothing is read through the tables, no hit is written, n_hits and counts are 0.
 * No workspace.  The three calls are stream-ordered, allocate nothing and never sync.
 */
#define HMSE_FIND_MAX_PATTERNS 32
#define HMSE_FIND_MAX_LEN 256
#define HMSE_FIND_IGNORE_CASE 1u

/*
 * Scan: every match lying wholly inside ONE record [raw_off[r], raw_off[r+1]).  Records that are neighbours in raw are not neighbours
 * in the corpus: a match across raw_off[r+1] is no hit.  A record may have any length (the position in raw carries it).
 *   raw     DEVICE u8[raw_bytes], any alignment;  raw_off DEVICE u64[n_rec+1] ascending, raw_off[n_rec] <= raw_bytes
 *   mult    DEVICE u32[n_rec] or NULL: counts[j] = sum over the hits of pattern j of mult[record] (NULL: 1 each) — with the number of
 *           chunks that map to each record, the in-record occurrences in the corpus
 *   hits    position = offset in raw
 */
int hmse_find_scan(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint32_t* mult,
                   const uint8_t* pat, const uint32_t* pat_off, uint32_t n_pat, uint32_t flags, uint64_t* hits,
                   uint64_t hits_cap, uint64_t* n_hits, uint64_t* counts, uint32_t* status, void* stream);

/*
 * Seams: chunk k covers corpus bytes [cuts[k], cuts[k+1]); corpus byte p of chunk c is raw[raw_off[slot[c]] + p - cuts[c]].  An
 * occurrence (o, m) that starts in chunk k is a seam hit of k iff o + m > cuts[k+1]; it may run over any number of following chunks
 * (tiny and empty ones) and must end at or before N = cuts[n_chunks].  In-record hits of all chunks plus seam hits of all chunks are
 * every occurrence exactly once.
 *   cuts    DEVICE u64[n_chunks+1];  slot DEVICE u64[n_chunks]: the record of every chunk (a POINTER's: its target's)
 *   hits    position = corpus offset;  counts[j] = seam hits of pattern j
 */
int hmse_find_seams(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                    const uint64_t* slot, uint64_t n_chunks, const uint8_t* pat, const uint32_t* pat_off, uint32_t n_pat,
                    uint32_t flags, uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits, uint64_t* counts, uint32_t* status,
                    void* stream);

/*
 * Place: the scan's hits, sorted ascending, laid out in the corpus.  For every chunk k in corpus order and every hit h of record
 * slot[k] in ascending order: (cuts[k] + pos(h) - raw_off[slot[k]]) << 8 | pat(h) — ascending by corpus offset, then pattern.
 *   hits      DEVICE u64[n_hits] ascending
 *   chunk_out DEVICE u64[n_chunks+1]: exclusive prefix sum of the chunks' hit counts (the number of hits of record slot[k]);
 *             chunk k's hits go to out[chunk_out[k] ..)
 *   out       DEVICE u64[out_cap], written up to chunk_out[n_chunks]
 *   status    DEVICE u32[1]: bit0 = chunk_out[n_chunks] > out_cap, bit1 = inconsistent tables (as above, or chunk_out is not the
 *             count of its records' hits in the list)
 */
int hmse_find_place(const uint64_t* hits, uint64_t n_hits, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                    const uint64_t* slot, uint64_t n_chunks, const uint64_t* chunk_out, uint64_t* out, uint64_t out_cap,
                    uint32_t* status, void* stream);

/*
 * Dictionary search (hmse_amd/find.py PatternSet): the question of hmse_find_* for a whole SET of patterns in one pass — up to
 * HMSE_FINDSET_MAX_PATTERNS of HMSE_FINDSET_MIN_LEN..HMSE_FIND_MAX_LEN bytes each.  hmse_find_scan's work per position grows with the
 * patterns and its ABI ends at 32 of them; here the set is compiled ONCE into the structure below and a position whose four-byte
 * window no pattern starts with costs one hash and one bit lookup, whatever the size of the set.  (Patterns of 1..3 bytes have no
 * four-byte key: they are not part of a set and go through hmse_find_*.)
 *
 * The compiled set is plain device arrays, so any caller can build it (hmse_amd/find.py does, on the host, with sorts only):
 *   key(p)  = the first four bytes of pattern p as a little-endian u32;  h(key) = key * HMSE_FINDSET_HASH mod 2^32
 *   entries = the n_entries patterns sorted by (h(key), key, length, bytes); entry i is upat[uoff[i] .. uoff[i+1]), ukey[i] = its key,
 *             uid[i] < n_ids = the id reported for it (any map: several entries may not share an id unless the caller wants their
 *             hits and counts merged)
 *   dir     = u32[2^dir_bits + 1]: the entries whose h has the top dir_bits bits c are dir[c] .. dir[c+1]; dir[0] = 0,
 *             dir[2^dir_bits] = n_entries.  1 <= dir_bits <= 21; 2^dir_bits >= 2 * n_entries keeps a cell at half an entry on average
 *   bitmap  = u32[2^(HMSE_FINDSET_BITMAP_BITS - 5)] (64 KiB): bit (h(key) >> 13) is set for every entry (the scan keeps it in LDS)
 *   flags   = HMSE_FIND_IGNORE_CASE iff the patterns were folded (A-Z -> a-z) before they were keyed and sorted; a call's flags
 *             must equal the set's
 *   max_len >= every entry's length (it sizes the seam launch)
 * Nothing has a capacity: any number of entries may share a key or a cell — the walk gets longer, no pattern is dropped.
 * The kernels do not trust the set: a validate kernel runs first in every call and sets status bit 1 (nothing is then read through the
 * set or the tables, no hit is written, n_hits and counts are 0) for a directory that descends or does not cover [0, n_entries), an
 * id >= n_ids, a byte range that descends, leaves upat or is not MIN_LEN..max_len long, a key that is not the first four bytes of its
 * pattern (or not folded in a folded set), an entry outside its directory cell or without its bit in the bitmap.  The header (a HOST
 * struct, read during the call only) is checked on the host: HMSE_EINVAL, before anything is cleared or launched, for struct_size,
 * unknown flag bits, flags that differ from the call's, n_entries or n_ids above HMSE_FINDSET_MAX_PATTERNS, and with n_entries > 0:
 * n_ids == 0, dir_bits outside 1..21, max_len outside 4..256, pat_bytes outside 4 .. 256 bytes per entry, a NULL array.
 * n_entries == 0 is a legal, empty set (the arrays may be NULL): the outputs are cleared, nothing is launched.
 *
 * A hit is one u64: position << HMSE_FINDSET_ID_BITS | id.  Ids are below 2^20, positions below 2^40: raw_bytes >= 2^40 is
 * HMSE_EINVAL; cuts lives on the device, so cuts[n_chunks] >= 2^40 is status bit 1 (the calls never sync).
 *   hits, hits_cap, n_hits, status as for hmse_find_*;  counts DEVICE u64[n_ids] (NULL only with n_ids == 0)
 * The three calls mirror hmse_find_scan / _seams / _place argument by argument, with (set, flags) in the place of
 * (pat, pat_off, n_pat, flags); scan and seams, in-record and seam hits, mult and the chunk map mean what they mean there.
 * hmse_findset_place is hmse_find_place for this hit word (hits sorted ascending; out = corpus offset << 24 | id).
 * No workspace; stream-ordered, allocate nothing, never sync.  Profile slots: hmse_findset_scan reports in 30, hmse_findset_seams
 * and hmse_findset_place in 31 — the slots hmse_find_* and the DELTA encode kernels already share (see Diagnostics below).
 */
#define HMSE_FINDSET_MAX_PATTERNS (1u << 20)
#define HMSE_FINDSET_MIN_LEN 4
#define HMSE_FINDSET_ID_BITS 24
#define HMSE_FINDSET_BITMAP_BITS 19
#define HMSE_FINDSET_HASH 0x9E3779B1u

typedef struct hmse_findset {
  uint32_t struct_size;   /* sizeof(hmse_findset) */
  uint32_t flags;         /* HMSE_FIND_IGNORE_CASE: the patterns are folded */
  uint32_t n_entries;
  uint32_t n_ids;
  uint32_t dir_bits;
  uint32_t max_len;
  uint64_t pat_bytes;     /* bytes of upat */
  const uint8_t* upat;    /* DEVICE u8[pat_bytes] */
  const uint32_t* uoff;   /* DEVICE u32[n_entries + 1] */
  const uint32_t* ukey;   /* DEVICE u32[n_entries] */
  const uint32_t* uid;    /* DEVICE u32[n_entries] */
  const uint32_t* dir;    /* DEVICE u32[2^dir_bits + 1] */
  const uint32_t* bitmap; /* DEVICE u32[16384] */
} hmse_findset;

int hmse_findset_scan(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint32_t* mult,
                      const hmse_findset* set, uint32_t flags, uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits,
                      uint64_t* counts, uint32_t* status, void* stream);
int hmse_findset_seams(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                       const uint64_t* slot, uint64_t n_chunks, const hmse_findset* set, uint32_t flags, uint64_t* hits,
                       uint64_t hits_cap, uint64_t* n_hits, uint64_t* counts, uint32_t* status, void* stream);
int hmse_findset_place(const uint64_t* hits, uint64_t n_hits, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                       const uint64_t* slot, uint64_t n_chunks, const uint64_t* chunk_out, uint64_t* out, uint64_t out_cap,
                       uint32_t* status, void* stream);

/*
 * Replication (hmse_amd/sync.py): the byte proof behind a digest join of two stores.  Record k of store a (the wanted one) has the
 * stored stream a[a_off[k] .. a_off[k] + a_len[k]) and the candidate cand[k], a record of store b (the one the replica holds) with the
 * stream b[b_off[c] .. b_off[c] + b_len[c]).  Equal digests say the decoded chunks are equal, not the streams: the same chunk may be
 * FULL in one store and DELTA in the other, or DELTA against another dictionary.
 *   same[k] = 1 iff 0 <= cand[k] < n_b, a_len[k] == b_len[cand[k]] and the two byte ranges are equal (length 0 on both sides: 1).
 *   same[k] is WRITTEN FOR EVERY k < n: the caller clears nothing.
 *   cand[k] < 0: no candidate — same[k] = 0, no status bit, record k's range is not looked at.
 *   cand[k] >= n_b, or a range of either side that reaches outside its blob (off > bytes or len > bytes - off): same[k] = 0 and
 *   status bit 0; nothing outside a[0 .. a_bytes) and b[0 .. b_bytes) is read.  Ranges are checked before lengths are compared;
 *   unequal lengths give 0 without reading a stream byte.
 *   a, b    DEVICE u8, any alignment (lba_unit may be 1: the two sides are misaligned independently); NULL only with 0 bytes
 *   a_off   DEVICE u64[n];  a_len DEVICE u32[n];  b_off DEVICE u64[n_b];  b_len DEVICE u32[n_b] (NULL only with n_b == 0)
 *   cand    DEVICE i64[n];  same DEVICE u8[n];  status DEVICE u32[1]
 * n == 0 clears the status word and returns HMSE_OK.  HMSE_EINVAL before anything is cleared or launched: status NULL, n >= 2^33,
 * with n > 0 a NULL pointer to a non-empty array.  No workspace (hmse_workspace_bytes(HMSE_STAGE_SYNC_MATCH, ...) is 0);
 * stream-ordered, allocates nothing, never syncs.  One wavefront per record, 16 bytes per lane and side and trip; the record is left
 * at the first 1 KiB trip that differs.  Reads at most 2 x the compared bytes.
 */
int hmse_sync_match(const uint8_t* a, uint64_t a_bytes, const uint64_t* a_off, const uint32_t* a_len, uint64_t n, const uint8_t* b,
                    uint64_t b_bytes, const uint64_t* b_off, const uint32_t* b_len, uint64_t n_b, const int64_t* cand, uint8_t* same,
                    uint32_t* status, void* stream);

/*
 * Lines (hmse_amd/find.py lines / text / grep): from a hit to the line — the delimited record — it lies in, with context, and its text.
 * Replaces the detour a user of hmse_find_* is left with today: read the store back, move the corpus to the host and run bytes.rfind /
 * bytes.find per hit.  The tables (raw, raw_off, cuts, slot) mean what they mean for hmse_find_seams: corpus byte p of chunk c is
 * raw[raw_off[slot[c]] + p - cuts[c]], C is the N = cuts[n_chunks] bytes of the corpus.  A line does not stop at a chunk boundary, a
 * record that several chunks map to has other neighbours at each of its places, and chunks may be 0, 1 or 2 bytes long.
 *
 * Definitions, for a corpus offset o < N, the delimiter d = delim (one byte value), before = b, after = a, reach = R:
 *   start  look at positions o-1, o-2, ..., max(o-R, 0) in that order: start = 1 + the position of the (b+1)-th byte equal to d met
 *          on the way.  Fewer are met: start = max(o-R, 0), and HMSE_LINES_START_CUT is set iff o-R > 0 (reaching the corpus's first
 *          byte is no cut).
 *   end    look at positions o, o+1, ..., min(o+R, N)-1: end = the position of the (a+1)-th byte equal to d.  Fewer are met:
 *          end = min(o+R, N), and HMSE_LINES_END_CUT is set iff o+R < N.
 * The extent is C[start .. end): it never holds the closing delimiter, it holds b + a inner delimiters when nothing was cut, and a
 * delimiter AT o closes o's own line (end = o when a = 0).  With no cut this is what splitting C at d gives: start of line
 * max(i-b, 0), end of line i+a (N if there is none), i the line with L_i <= o <= R_i — the trailing empty line of a corpus that ends
 * in d included.  Out of scope: delimiters of more than one byte, CR stripping, merging the overlapping context of neighbouring
 * hits (grep's "--" groups).
 *
 * A validate kernel runs first in each call: status bit 1 = inconsistent tables, by hmse_find_*'s rules (raw_off or cuts descending,
 * raw_off[n_rec] > raw_bytes, slot[k] >= n_rec, a chunk whose length is not its record's) and for cuts[0] != 0 (the positions come
 * from the caller here).  With bit 1 nothing is read through the tables.
 * No workspace, no stage id of their own; both calls report in profile slot 31 (see Diagnostics below).  Stream-ordered, allocate
 * nothing, never sync.  HMSE_EINVAL before anything is cleared or launched: status NULL, n >= 2^33, with n > 0 a NULL pointer to a
 * non-empty array (raw: raw_bytes > 0; raw_off: n_rec or n_chunks > 0; cuts, slot: n_chunks > 0).  n == 0 clears the status word and
 * returns HMSE_OK.
 *
 * hmse_lines_extent — one wavefront per position; per trip it looks at 64 bytes (one per lane), clipped to the chunk and to reach:
 *   pos     DEVICE u64[n]: corpus offsets, any order, equal ones allowed
 *   start, end DEVICE u64[n];  flags DEVICE u8[n]: WRITTEN FOR EVERY i < n, the caller clears nothing
 *   pos[i] >= N (N == 0, n_chunks == 0: every position): start = end = 0, flags = HMSE_LINES_BAD, status bit 0; the others are answered
 *   status bit 1: every i gets 0 / 0 / HMSE_LINES_BAD
 *   delim <= 255, 1 <= reach <= HMSE_LINES_MAX_REACH (else HMSE_EINVAL); before and after are any u32 — reach bounds the work: at
 *   most 2 * reach bytes are looked at per position.
 * hmse_lines_gather — one wavefront per range; 16 bytes per lane between the ends of every chunk piece:
 *   start, end DEVICE u64[n]: ranges of the corpus, start[i] <= end[i] <= N, empty ones are legal, they may overlap
 *   out_off DEVICE u64[n+1]: the caller's exclusive prefix sum of end[i] - start[i];  out DEVICE u8[out_cap], any alignment, NULL only
 *           with out_cap == 0 (else HMSE_EINVAL)
 *   out[out_off[i] .. out_off[i] + end[i] - start[i]) = C[start[i] .. end[i]) for every i
 *   status bit 0: out_off[n] > out_cap.  bit 1: inconsistent tables, some start[i] > end[i], some end[i] > N, or
 *   out_off[i+1] - out_off[i] != end[i] - start[i].  With either bit NOTHING is written to out.
 */
#define HMSE_LINES_START_CUT 1u
#define HMSE_LINES_END_CUT   2u
#define HMSE_LINES_BAD       128u
#define HMSE_LINES_MAX_REACH (1u << 24)

int hmse_lines_extent(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec,
                      const uint64_t* cuts, const uint64_t* slot, uint64_t n_chunks,
                      const uint64_t* pos, uint64_t n, uint32_t delim, uint32_t before, uint32_t after, uint32_t reach,
                      uint64_t* start, uint64_t* end, uint8_t* flags, uint32_t* status, void* stream);

int hmse_lines_gather(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec,
                      const uint64_t* cuts, const uint64_t* slot, uint64_t n_chunks,
                      const uint64_t* start, const uint64_t* end, const uint64_t* out_off, uint64_t n,
                      uint8_t* out, uint64_t out_cap, uint32_t* status, void* stream);

/*
 * Regular-expression search (hmse_amd/regex.py compiles, hmse_amd/find.py StoreFinder.find_regex runs): the question of hmse_find_*
 * for a regular expression — every ISO date, every IPv4 address, `(error|warn)[a-z ]*id=`.  Replaces read_store -> host -> re.finditer.
 * The matcher is a DFA compiled on the host; the kernels walk its transition table.
 *
 * Definitions.  C is the N bytes of the corpus, L(r) the byte strings the regex denotes, R = reach (below).  Start o is an OCCURRENCE
 * iff some l with 1 <= l <= min(R, N - o) has C[o .. o + l) in L(r); its LENGTH is the largest such l.  Empty matches are never
 * reported; every start counts, overlapping ones included (`a+` has four occurrences in `aaaa`, of 4, 3, 2 and 1 bytes).  A match is
 * at most HMSE_REGEX_MAX_LEN bytes: `x.*y` reports the longest match within 256 bytes — this is the definition, not a defect.
 *
 * The compiled form is plain device arrays, so any caller can build it:
 *   state 0 is the dead state (its row is all 0), state 1 the start; n_states <= 32767
 *   classmap = u8[256]: the class of every byte value, < n_classes
 *   table    = u16[n_states * n_classes]: table[s * n_classes + c] = the next state, OR-ed with HMSE_REGEX_ACCEPT iff that state accepts
 *   reach    = 1..256: no match is longer (the longest path through the live states if they hold no cycle, else 256)
 *   n_states * n_classes <= HMSE_REGEX_MAX_TABLE (32 KiB: the kernels keep the table in LDS beside a tile of data)
 * The header is a HOST struct, read during the call only.  HMSE_EINVAL before anything is cleared or launched: struct_size,
 * n_states < 2 or > 32767, n_classes outside 1..256, a table over the cap, reach outside 1..256, a NULL pointer to a non-empty array,
 * raw_bytes >= 2^56.
 *
 * Partition by START (a longest match may or may not cross a boundary): start p of record r is a SCAN start iff
 * raw_off[r+1] - p >= reach — its answer depends on the record only and holds for every chunk that maps to r (hmse_regex_scan, laid
 * out by hmse_find_place, which passes the low byte through); start o of chunk k is a SEAM start iff cuts[k+1] - o < reach — the
 * last min(reach - 1, chunk length) positions of the chunk, walked through the chunk map over any number of tiny or empty chunks and
 * clipped to N (hmse_regex_seams).  Scan starts placed plus seam starts of all chunks are every occurrence exactly once.
 *
 * A hit is one u64: position << 8 | (length - 1); position = offset in raw (scan), corpus offset (seams).
 *   hits, hits_cap, n_hits as for hmse_find_*;  count DEVICE u64[1]: scan = the sum of mult[record] over the hits, seams = the hits
 *   status  DEVICE u32[1]: bit0 = the hit list ran out (n_hits and count stay exact), bit1 = inconsistent tables (hmse_find_*'s rules),
 *           bit2 = bad automaton: a table entry whose low 15 bits are >= n_states, a non-zero dead row, a classmap value >= n_classes.
 *           With bit1 or bit2 nothing is read through the tables or the automaton, no hit is written, n_hits and count are 0.
 * The other arguments mean what they mean for hmse_find_scan / hmse_find_seams.  No workspace; stream-ordered, allocate nothing, never
 * sync.  Profile slots: hmse_regex_scan reports in 30, hmse_regex_seams in 31 (see Diagnostics below).
 * Out of scope here: anchors and \b (include/hmse_regexa.h has them: hmse_regexa_scan / hmse_regexa_seams, a library of its own),
 * captures, lazy matching, matches over 256 bytes, Unicode classes, several regexes in one automaton.
 */
#define HMSE_REGEX_MAX_LEN   256
#define HMSE_REGEX_MAX_TABLE 16384
#define HMSE_REGEX_ACCEPT    0x8000u

typedef struct hmse_regex {
  uint32_t struct_size;      /* sizeof(hmse_regex) */
  uint32_t n_states;
  uint32_t n_classes;
  uint32_t reach;
  const uint16_t* table;     /* DEVICE u16[n_states * n_classes] */
  const uint8_t* classmap;   /* DEVICE u8[256] */
} hmse_regex;

int hmse_regex_scan(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint32_t* mult,
                    const hmse_regex* rx, uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits, uint64_t* count, uint32_t* status,
                    void* stream);
int hmse_regex_seams(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                     const uint64_t* slot, uint64_t n_chunks, const hmse_regex* rx, uint64_t* hits, uint64_t hits_cap,
                     uint64_t* n_hits, uint64_t* count, uint32_t* status, void* stream);

/*
 * Approximate search (hmse_amd/find.py StoreFinder.find_approx): where does something within k edits of this byte string occur?  —
 * agrep's question, at byte granularity.  Replaces read_store -> host -> a dynamic programme over every duplicate chunk.  The matcher is
 * Myers' bit-vector algorithm: one 64-bit column per pattern, a fixed number of integer operations per byte.
 *
 * Definitions (tests/approx_ref.py restates them in plain Python, with Sellers' DP).  C is the N bytes of the corpus.  Patterns are byte
 * strings of 1..HMSE_APPROX_MAX_LEN bytes, pattern j with an error bound k_j, 0 <= k_j <= HMSE_APPROX_MAX_K and k_j < m_j (with
 * k >= m every position would match); at most HMSE_APPROX_MAX_PATTERNS per call.  The distance ed is Levenshtein's: insertion,
 * deletion and substitution cost 1 each.  HMSE_FIND_IGNORE_CASE folds A-Z to a-z on both sides, bytes >= 0x80 compare as they are.
 *   d_j(e) = min over 0 <= s <= e of ed(pat_j, C[s .. e))   for an END e, 1 <= e <= N
 *   e is an OCCURRENCE of pattern j iff d_j(e) <= k_j; its errors are d_j(e); its reported position is e - 1, the match's LAST byte
 *   (below N).  Every end counts: the neighbouring ends of one fuzzy match are each reported.  With k = 0 the occurrences are
 *   hmse_find_*'s offsets + m - 1.
 * Window.  W_j = m_j + k_j.  A start in front of e - W_j never gives a distance <= k_j (the text would be more than k_j bytes longer
 * than the pattern), so a column started fresh (D[i] = i) anywhere at or in front of e - W_j gives d_j(e) whenever that is <= k_j and
 * some value > k_j otherwise, whatever bytes lie in front of the window.
 * Partition by END (hmse_regex_*'s rule mirrored): end e lies in chunk c if byte e - 1 does.  It is a SCAN end iff e - cuts[c] >= W_j —
 * the answer depends on the record only (hmse_approx_scan, laid out by hmse_find_place, which passes the low byte through) — and a
 * SEAM end otherwise: the first min(W_j - 1, chunk length) ends of every chunk, walked through the chunk map from
 * max(cuts[c] + 1 - W_j, 0) on, over any number of tiny or empty chunks (hmse_approx_seams: at most 2 W_j - 2 steps per chunk and
 * pattern).  Scan ends placed plus seam ends of all chunks are every occurrence exactly once.
 * Span.  The start of an occurrence is the largest s with ed(pat_j, C[s .. e)) == d_j(e): the shortest best match, of m - d .. m + d
 * bytes.  hmse_approx_spans finds it with the anchored column (D[0][t] = t) of the reversed pattern over C[e-1], C[e-2], ...
 *
 * A hit is one u64: position << 8 | errors << 3 | pattern index; position = offset in raw (scan), corpus offset (seams) of the
 * match's last byte.
 *   pat      DEVICE u8: the patterns back to back;  pat_off HOST u32[n_pat + 1], k HOST u8[n_pat]: read during the call
 *   flags    HMSE_FIND_IGNORE_CASE or 0
 *   hits, hits_cap, n_hits as for hmse_find_*: hits_cap == 0 counts only; n_hits and counts stay exact when the list runs out
 *   counts   DEVICE u64[n_pat]: scan = per pattern the sum of mult[record] over its hits (mult NULL: 1 each), seams = its hits
 *   status   DEVICE u32[1]: bit0 = the hit list ran out, bit1 = inconsistent tables (hmse_find_*'s rules): nothing is read through
 *            them, no hit is written, n_hits and counts are 0
 * hmse_approx_spans: hits DEVICE u64[n] = hit words with CORPUS offsets, any order; start DEVICE u64[n], written for every i < n.
 *   status bit0: some hit has an offset >= N, a pattern index >= n_pat or errors that no window of m_j + errors bytes ending there
 *   attains — such a hit gets start = offset + 1, an empty span.  bit1 as above (nothing is written).  n == 0 clears the status word.
 * The other arguments mean what they mean for hmse_find_scan / hmse_find_seams.  HMSE_EINVAL before anything is cleared or launched:
 * n_pat of 0 or above HMSE_APPROX_MAX_PATTERNS, a pattern length of 0 or above HMSE_APPROX_MAX_LEN, k[j] >= its length or above
 * HMSE_APPROX_MAX_K, unknown flag bits, raw_bytes >= 2^56, a NULL pointer to a non-empty array.  No workspace; stream-ordered,
 * allocate nothing, never sync.  Profile slots: hmse_approx_scan reports in 30, hmse_approx_seams and hmse_approx_spans in 31.
 * Out of scope: patterns over 64 bytes, Hamming-only and transposition distances, weighted costs, errors inside a regex, a
 * dictionary of approximate patterns.
 */
#define HMSE_APPROX_MAX_PATTERNS 8
#define HMSE_APPROX_MAX_LEN      64
#define HMSE_APPROX_MAX_K        16

int hmse_approx_scan(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint32_t* mult,
                     const uint8_t* pat, const uint32_t* pat_off, const uint8_t* k, uint32_t n_pat, uint32_t flags, uint64_t* hits,
                     uint64_t hits_cap, uint64_t* n_hits, uint64_t* counts, uint32_t* status, void* stream);
int hmse_approx_seams(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                      const uint64_t* slot, uint64_t n_chunks, const uint8_t* pat, const uint32_t* pat_off, const uint8_t* k,
                      uint32_t n_pat, uint32_t flags, uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits, uint64_t* counts,
                      uint32_t* status, void* stream);
int hmse_approx_spans(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                      const uint64_t* slot, uint64_t n_chunks, const uint8_t* pat, const uint32_t* pat_off, uint32_t n_pat,
                      uint32_t flags, const uint64_t* hits, uint64_t n, uint64_t* start, uint32_t* status, void* stream);

/*
 * Export (hmse_amd/export.py): a store as multi-member gzip (RFC 1952) or BGZF.  A stored FULL record is a complete raw DEFLATE stream,
 * so its member is header + the stream as stored + CRC-32 + raw length; a DELTA record is encoded again without its dictionary first
 * (hmse_l1_deflate), gzip has none.  One member per chunk of the corpus, in corpus order, POINTER chunks included.
 *
 * Definitions (tests/export_ref.py restates them in plain Python).  The CRC-32 is zlib's and gzip's: polynomial 0xEDB88320 (reflected),
 * initial value and final xor 0xFFFFFFFF; an empty range gives 0.  With x^k the polynomial x^k modulo that one, in the register's bit
 * order, and * the product modulo it:  crc(A | B) = crc(A) * x^(8 |B|) ^ crc(B).
 *
 * hmse_crc32: crc_out[k] = CRC-32 of data[cuts[k], cuts[k + 1]) for the n_chunks ranges of cuts (DEVICE u64[n_chunks + 1], ascending;
 *   ranges may be empty, start at any byte and have any length).  status DEVICE u32[1]: bit0 = cuts descends somewhere or
 *   cuts[n_chunks] > n — nothing is read through cuts, crc_out is left as it was.  n_chunks == 0 clears the status word.
 * hmse_crc32_combine: out[0] = CRC-32 of the concatenation of n ranges given their CRCs (DEVICE u32[n]) and lengths (DEVICE u64[n], any
 *   values whose sum stays below 2^61: they are exponents only).  n == 0 gives 0.  status is cleared; no bit is defined.
 * hmse_gzip_members: member i (0 <= i < n_chunks) = header + stream of record r = slot[i] + crc[r] (u32 LE) + raw_off[r + 1] - raw_off[r]
 *   (u32 LE) at dst + member_off[i]; the stream is stream_len[r] bytes at src_off[r] of src1 if src_sel[r] else of src0 (as for
 *   hmse_record_gather: the store's blob and the streams encoded again).  All tables DEVICE: src_off, stream_len u64[n_rec], src_sel
 *   u8[n_rec], crc u32[n_rec], raw_off u64[n_rec + 1], slot u64[n_chunks], member_off u64[n_chunks + 1] (the caller's prefix sum).
 *   flags 0: the 10-byte header 1f 8b 08 00 | MTIME 0 | XFL 0 | OS ff.  HMSE_GZIP_BGZF: the 18-byte header 1f 8b 08 04 00 00 00 00 00 ff
 *   06 00 42 43 02 00 + BSIZE (u16 LE) = the member's size - 1; the caller appends the 28-byte EOF block.
 *   status DEVICE u32[1]: bit0 = slot[i] >= n_rec, a stream outside its source, a member outside dst_bytes, member_off descending or
 *   member_off[i + 1] - member_off[i] != header + stream_len[r] + 8, a raw length above 2^32 - 1; bit1 = a BGZF member above 65536 bytes
 *   (a chunk of at most 32768 bytes never gives one).  With either bit nothing is written to dst.
 * HMSE_EINVAL before anything is cleared or launched: status NULL, unknown flag bits, a NULL pointer to a non-empty array, n_chunks
 * above 2^40 (hmse_crc32), n above 2^32 (hmse_crc32_combine), n_chunks >= 2^33 (hmse_gzip_members).  No workspace; stream-ordered,
 * allocate nothing, never sync.  Profile slots: hmse_crc32 reports in 0, hmse_gzip_members in 1.
 * Out of scope: byte ranges or single documents, containers, other codecs, one member for the whole corpus; importing gzip: hmse_gunzip.h.
 */
#define HMSE_GZIP_BGZF 1u

int hmse_crc32(const uint8_t* data, uint64_t n, const uint64_t* cuts, uint64_t n_chunks, uint32_t* crc_out, uint32_t* status, void* stream);
int hmse_crc32_combine(const uint32_t* crc, const uint64_t* len, uint64_t n, uint32_t* out, uint32_t* status, void* stream);
int hmse_gzip_members(const uint8_t* src0, uint64_t src0_bytes, const uint8_t* src1, uint64_t src1_bytes, const uint64_t* src_off,
                      const uint64_t* stream_len, const uint8_t* src_sel, const uint32_t* crc, const uint64_t* raw_off, uint64_t n_rec,
                      const uint64_t* slot, uint64_t n_chunks, const uint64_t* member_off, uint32_t flags, uint8_t* dst, uint64_t dst_bytes,
                      uint32_t* status, void* stream);

/*
 * Diagnostics (bench.py's roofline leg): when enabled, every entry point brackets its DOMINANT
 * kernel launch with a HIP event pair on the caller's stream.  hmse_profile_read() waits for the
 * recorded events (a host sync — never call it inside a capture), adds their durations to the
 * stage's running total and returns it.  Off by default; not part of the data path.
 * Slots: the HMSE_STAGE_* ids (0..31); the six DEFLATE match-kernel size classes report in slots 8..13
 * (S, SG2, SG3, B, S2, SG), their dictionary jobs in 18..23, and the two encode-kernel instantiations in 14 and 15 (FULL
 * records) and 30 and 31 (DELTA records) (hmse_amd/csrc/l1_deflate.hip); hmse_find_scan also reports in 30, hmse_find_seams and
 * hmse_find_place in 31, hmse_sync_match in 19; hmse_findset_scan reports in 30 as well, hmse_findset_seams and hmse_findset_place in 31.
 * hmse_lines_extent and hmse_lines_gather report in 31 as well (reset the slot before reading one of them: it is shared).
 * hmse_regex_scan reports in 30 and hmse_regex_seams in 31, too; so do hmse_approx_scan (30), hmse_approx_seams and hmse_approx_spans (31).
 * hmse_crc32 reports in 0 and hmse_gzip_members in 1 (HMSE_STAGE_EXPORT_*): slots of their own.
 * hmse_profile_counter(): work counted on the device while profiling is on — the DEFLATE match kernels add the TOKENS they
 * write to their slot (8..13, 18..23), the encode kernels the tokens they read (14, 15, 30, 31):
 * bench.py's algorithmic bytes come from these counts, not from an assumed token density.  A host sync; diagnostics only.
 */
void hmse_profile_enable(int on);
int hmse_profile_read(int stage, double* total_ms, uint64_t* launches, int reset);
int hmse_profile_counter(int slot, uint64_t* value, int reset);

#ifdef __cplusplus
}
#endif
#endif /* HMSE_H */
