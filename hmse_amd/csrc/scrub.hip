// scrub.hip — which of a store's records are intact, and how far each damaged one reaches (hmse_amd/scrub.py, include/hmse.h).
//
// A scrub decodes every record of a store once, like read_store, but never stops at a damaged byte.  Two passes bracket the
// existing decode (hmse_l1_inflate with per-record ok flags, then hmse_l3_sha256 of the decoded records):
//   hmse_scrub_records    one thread per record: is the record inside its shard's blob; for a DELTA record its 8-byte
//                         DeltaChunk header is read and base_lba is looked up by binary search in that shard's sorted LBAs
//                         (the shard the dictionary must be on: its own, or the one remote_bases names) -> STRUCTURE and
//                         HEADER flags and the resolved global dictionary slot.  The same thread counts the non-zero padding
//                         bytes in front of its record in LBA order (and behind the last record of its shard); thread s also
//                         counts the whole blob of shard s when that shard holds no record.
//   hmse_scrub_attribute  own fault per record (STRUCTURE / METADATA / decoder reject / digest mismatch) -> by POINTER
//                         DOUBLING over the dictionary forest the furthest faulty ancestor of every record, which is its root
//                         (a record below a damaged dictionary is DICTIONARY, its own state unknown); then per chunk of the
//                         chunk map its root, per root the records, chunks and logical bytes lost (atomics: sums do not depend
//                         on order), and the maximal runs of damaged chunks as (offset, length) by a count-then-write scan.
// No value read from the blob indexes memory: base_lba is only ever compared with the index's LBAs.  Every loop bound is
// wave-uniform and scalar (a kernel argument, or the wave maximum taken before the loop), as in l4_query.hip.
#include "common.h"
#include "blockops.h"

constexpr int SC_NT = 256;
constexpr int SC_SCAN_NT = 1024;
constexpr uint32_t SC_NONE = 0xFFFFFFFFu;

size_t hmse_scrub_attribute_workspace_bytes_impl(uint64_t n_records, uint64_t n_chunks) {
  // anc / far ping-pong (u32 x 4 per record), the live flag, block counts of the boundary scan
  return 4 * hmse_align_up(4 * (n_records + 1), 256) + 256 + hmse_align_up(4 * (hmse_blocks(n_chunks + 1, SC_NT) + 1), 256);
}

// ---- records ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_NT) void sc_records_kernel(const uint8_t* __restrict__ blob, uint64_t n, const uint32_t* __restrict__ rec_shard,
                                                          const uint64_t* __restrict__ shard_blob, const uint64_t* __restrict__ shard_slot,
                                                          const uint32_t* __restrict__ lba_unit, const uint32_t* __restrict__ lba,
                                                          const uint32_t* __restrict__ rec_len, const uint8_t* __restrict__ kind,
                                                          const int64_t* __restrict__ remote, const uint32_t* __restrict__ sorted_lba,
                                                          const uint32_t* __restrict__ sorted_slot, uint32_t steps,
                                                          const uint8_t* __restrict__ meta, uint8_t* __restrict__ status,
                                                          int64_t* __restrict__ dict, uint64_t blob_bytes, uint32_t n_shards,
                                                          unsigned long long* padding) {
  const uint64_t k = (uint64_t)blockIdx.x * SC_NT + threadIdx.x;
  const bool valid = k < n;
  // shard bounds from the caller's table, clamped to the blob it passed
  auto bound = [&](uint32_t s) -> uint64_t { const uint64_t b = shard_blob[s]; return b < blob_bytes ? b : blob_bytes; };
  uint32_t gf = 0, gt = 0, ge = 0;   // padding in front of sorted record k, behind a shard's last record, and of a shard without records
  uint64_t f0 = 0, t0 = 0, e0 = 0;
  if (k < n_shards && shard_slot[k] == shard_slot[k + 1]) {                 // thread k also covers shard k when it holds no record
    const uint64_t b0 = bound((uint32_t)k), b1 = bound((uint32_t)k + 1);
    if (b1 > b0) { e0 = b0; ge = (uint32_t)((b1 - b0) > 0x7FFFFFFFull ? 0x7FFFFFFFull : b1 - b0); }
  }
  if (valid) {
    const uint32_t s = rec_shard[k];
    const uint64_t b0 = bound(s), b1 = bound(s + 1), slot0 = shard_slot[s], slot1 = shard_slot[s + 1];
    const uint32_t L = rec_len[k];
    const uint64_t o0 = b0 + (uint64_t)lba[k] * lba_unit[s];
    uint32_t st = meta[k];
    int64_t d = -1;
    const int64_t r = remote[k];
    if (r >= (int64_t)n) st |= HMSE_SCRUB_METADATA;
    if (o0 + L > b1) st |= HMSE_SCRUB_STRUCTURE;                         // outside the shard's blob
    else if (kind[k] == HMSE_KIND_DELTA && !(st & HMSE_SCRUB_METADATA)) {
      if (L < 8) st |= HMSE_SCRUB_STRUCTURE;
      else {
        uint32_t w0 = 0, w1 = 0;
        for (int i = 0; i < 4; i++) { w0 |= (uint32_t)blob[o0 + i] << (8 * i); w1 |= (uint32_t)blob[o0 + 4 + i] << (8 * i); }
        // the shard the dictionary must be on: remote_bases' shard (r = the global slot it names), else the record's own
        const uint32_t ds = r >= 0 ? rec_shard[r] : s;
        const uint64_t lo = shard_slot[ds], cnt0 = shard_slot[ds + 1] - lo;
        uint64_t first = 0, count = cnt0;                                // lower bound of base_lba in the shard's sorted LBAs
        for (uint32_t i = 0; i < steps; i++) {
          const uint64_t step = count >> 1, mid = first + step;
          const uint32_t v = count ? sorted_lba[lo + mid] : 0xFFFFFFFFu;
          const bool less = count != 0 && v < w0;
          first = less ? mid + 1 : first;
          count = count == 0 ? 0 : (less ? count - step - 1 : step);
        }
        const bool found = first < cnt0 && sorted_lba[lo + first] == w0;
        const uint64_t j = found ? lo + sorted_slot[lo + first] : 0;     // global slot of the named record
        if (!found) st |= HMSE_SCRUB_STRUCTURE;
        else if (r >= 0 ? (int64_t)j != r : j >= k) st |= HMSE_SCRUB_STRUCTURE;   // remote: the table's record; local: an earlier one
        else {
          d = (int64_t)j;
          if ((w1 & 0xFFFFu) != (rec_len[j] & 0xFFFFu)) st |= HMSE_SCRUB_HEADER;
        }
        if ((w1 >> 16) != ((L - 8) & 0xFFFFu)) st |= HMSE_SCRUB_HEADER;
      }
    }
    status[k] = (uint8_t)st;
    dict[k] = d;
    // padding: between the previous record in LBA order (sorted position k - 1 of the shard) and sorted record k
    const uint64_t q = slot0 + sorted_slot[k];
    const uint64_t qs = b0 + (uint64_t)lba[q] * lba_unit[s];
    uint64_t prev_end = b0;
    if (k > slot0) {
      const uint64_t p = slot0 + sorted_slot[k - 1];
      prev_end = b0 + (uint64_t)lba[p] * lba_unit[s] + rec_len[p];
    }
    const uint64_t hi = qs < b1 ? qs : b1;
    if (hi > prev_end) { f0 = prev_end; gf = (uint32_t)((hi - prev_end) > 0x7FFFFFFFull ? 0x7FFFFFFFull : hi - prev_end); }
    const uint64_t e = qs + rec_len[q];
    if (k + 1 == slot1 && e < b1) { t0 = e; gt = (uint32_t)((b1 - e) > 0x7FFFFFFFull ? 0x7FFFFFFFull : b1 - e); }
  }
  const uint32_t g = gf + gt + ge;
  const uint32_t gmax = wave_max(g);                                       // every lane is active here: no early return above
  uint32_t c = 0;
  for (uint32_t i = 0; i < gmax; i++) {
    if (i < g) c += blob[i < gf ? f0 + i : i < gf + gt ? t0 + (i - gf) : e0 + (i - gf - gt)] != 0 ? 1u : 0u;
  }
  if (c) atomicAdd(padding, (unsigned long long)c);
}

extern "C" int hmse_scrub_records(const uint8_t* blob, uint64_t blob_bytes, uint64_t n, uint32_t n_shards, const uint32_t* rec_shard,
                                  const uint64_t* shard_blob, const uint64_t* shard_slot, const uint32_t* lba_unit, const uint32_t* lba,
                                  const uint32_t* rec_len, const uint8_t* kind, const int64_t* remote, const uint32_t* sorted_lba,
                                  const uint32_t* sorted_slot, uint32_t steps, const uint8_t* meta, uint8_t* status, int64_t* dict,
                                  uint64_t* padding, void* stream_) {
  if (!padding || n_shards == 0 || n >= 0x7FFFFFFFull || steps > 64) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(padding, 0, 8, stream);
  if (n == 0 && blob_bytes == 0) return HMSE_OK;
  if (!blob || !blob_bytes || !shard_blob || !shard_slot) return HMSE_EINVAL;
  if (n && (!rec_shard || !lba_unit || !lba || !rec_len || !kind || !remote || !sorted_lba || !sorted_slot || !meta || !status || !dict))
    return HMSE_EINVAL;
  const uint64_t threads = n > n_shards ? n : n_shards;                    // (a shard without records is covered by thread `shard`)
  PROF_BEGIN(HMSE_STAGE_SCRUB_RECORDS, stream);
  sc_records_kernel<<<dim3((uint32_t)hmse_blocks(threads, SC_NT)), dim3(SC_NT), 0, stream>>>(blob, n, rec_shard, shard_blob, shard_slot, lba_unit, lba,
                                                                                    rec_len, kind, remote, sorted_lba, sorted_slot, steps, meta,
                                                                                    status, dict, blob_bytes, n_shards,
                                                                                    (unsigned long long*)padding);
  PROF_END(HMSE_STAGE_SCRUB_RECORDS, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

// ---- attribution -----------------------------------------------------------------------------------------------------------
// own fault of every record and the first doubling state: anc = its dictionary (SC_NONE: a top), far = itself if faulty
__global__ __launch_bounds__(SC_NT) void sc_init_kernel(uint64_t n, const uint8_t* __restrict__ status, const int64_t* __restrict__ dict,
                                                       const uint8_t* __restrict__ ok, const uint8_t* __restrict__ got,
                                                       const uint8_t* __restrict__ want, uint32_t check_digest, uint8_t* __restrict__ own,
                                                       uint32_t* __restrict__ anc, uint32_t* __restrict__ far) {
  const uint64_t k = (uint64_t)blockIdx.x * SC_NT + threadIdx.x;
  if (k >= n) return;
  const uint32_t st = status[k];
  uint32_t f = 0;
  if (st & (HMSE_SCRUB_STRUCTURE | HMSE_SCRUB_METADATA)) f = st & (HMSE_SCRUB_STRUCTURE | HMSE_SCRUB_METADATA);
  else if (!ok[k]) f = HMSE_SCRUB_STREAM;
  else if (check_digest) {
    const uint4* a = (const uint4*)(got + 32 * k);
    const uint4* b = (const uint4*)(want + 32 * k);
    const uint4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
    if (a0.x != b0.x || a0.y != b0.y || a0.z != b0.z || a0.w != b0.w || a1.x != b1.x || a1.y != b1.y || a1.z != b1.z || a1.w != b1.w)
      f = HMSE_SCRUB_DIGEST;
  }
  own[k] = (uint8_t)f;
  const int64_t d = dict[k];
  anc[k] = (st & (HMSE_SCRUB_STRUCTURE | HMSE_SCRUB_METADATA)) || d < 0 || (uint64_t)d >= n ? SC_NONE : (uint32_t)d;
  far[k] = f ? (uint32_t)k : SC_NONE;
}

// one doubling round r: far = the furthest faulty record on the chain [k, anc), anc = the 2^r-th ancestor.  live[r] (set by round
// r - 1; live[0] by the caller) lets the rounds after convergence copy through; a record that still has an ancestor sets live[r + 1].
__global__ __launch_bounds__(SC_NT) void sc_double_kernel(uint64_t n, const uint32_t* __restrict__ anc_in, const uint32_t* __restrict__ far_in,
                                                         uint32_t* __restrict__ anc_out, uint32_t* __restrict__ far_out,
                                                         const uint32_t* live_in, uint32_t* live_out) {
  const uint64_t k = (uint64_t)blockIdx.x * SC_NT + threadIdx.x;
  if (k >= n) return;
  const uint32_t a = anc_in[k];
  if (*live_in == 0u || a == SC_NONE) { anc_out[k] = a; far_out[k] = far_in[k]; return; }
  const uint32_t fa = far_in[a];
  far_out[k] = fa != SC_NONE ? fa : far_in[k];
  const uint32_t aa = anc_in[a];
  anc_out[k] = aa;
  if (aa != SC_NONE) atomicOr(live_out, 1u);
}

__device__ __forceinline__ bool sc_damaged(uint32_t st) {
  return (st & (HMSE_SCRUB_STRUCTURE | HMSE_SCRUB_STREAM | HMSE_SCRUB_DIGEST | HMSE_SCRUB_DICTIONARY | HMSE_SCRUB_METADATA)) != 0;
}

// final record flags and roots (own flags are read from status_out and replaced in place by the same thread); records lost per root
__global__ __launch_bounds__(SC_NT) void sc_final_kernel(uint64_t n, const uint8_t* __restrict__ status, const uint32_t* __restrict__ far,
                                                        uint8_t* status_out, int64_t* __restrict__ root,
                                                        unsigned long long* __restrict__ root_records, unsigned long long* __restrict__ counts) {
  const uint64_t k = (uint64_t)blockIdx.x * SC_NT + threadIdx.x;
  if (k >= n) return;
  const uint32_t st = status[k], r = far[k], own = status_out[k];
  uint32_t out = st & HMSE_SCRUB_HEADER;
  if (r == (uint32_t)k) out |= own;
  else if (r != SC_NONE) out |= HMSE_SCRUB_DICTIONARY;
  status_out[k] = (uint8_t)out;
  root[k] = r == SC_NONE ? -1 : (int64_t)r;
  if (r != SC_NONE) { atomicAdd(&root_records[r], 1ull); atomicAdd(&counts[1], 1ull); }
  if (out & HMSE_SCRUB_HEADER) atomicAdd(&counts[6], 1ull);
}

// per chunk: root (-2: an inconsistent map entry), counters, block counts of the run boundaries (chunk i is a boundary when its
// damage differs from chunk i-1's; chunk -1 and chunk n are good)
__global__ __launch_bounds__(SC_NT) void sc_chunks_kernel(uint64_t n_chunks, const int64_t* __restrict__ slot, uint64_t n,
                                                         const uint64_t* __restrict__ cuts, const int64_t* __restrict__ root,
                                                         int64_t* __restrict__ chunk_root, unsigned long long* __restrict__ root_chunks,
                                                         unsigned long long* __restrict__ root_bytes, unsigned long long* __restrict__ counts,
                                                         uint32_t* __restrict__ bsum) {
  const uint64_t i = (uint64_t)blockIdx.x * SC_NT + threadIdx.x;
  auto root_of = [&](uint64_t c) -> int64_t {
    const int64_t s = slot[c];
    return (s < 0 || (uint64_t)s >= n) ? -2 : root[s];
  };
  int bnd = 0;
  if (i < n_chunks) {
    const int64_t r = root_of(i);
    chunk_root[i] = r;
    if (r != -1) {
      const unsigned long long len = cuts[i + 1] - cuts[i];
      if (r >= 0) { atomicAdd(&root_chunks[r], 1ull); atomicAdd(&root_bytes[r], len); }
      else { atomicAdd(&counts[4], 1ull); atomicAdd(&counts[5], len); }
      atomicAdd(&counts[2], 1ull); atomicAdd(&counts[3], len);
    }
    const bool prev = i > 0 && root_of(i - 1) != -1;
    bnd = (r != -1) != prev;
  } else if (i == n_chunks) {
    bnd = n_chunks > 0 && root_of(i - 1) != -1;
  }
  const int c = __syncthreads_count(bnd);
  if (threadIdx.x == 0) bsum[blockIdx.x] = (uint32_t)c;
}

// boundary j at chunk i -> ranges[j] = cuts[i] (an even j starts a run, an odd one ends it)
__global__ __launch_bounds__(SC_NT) void sc_emit_kernel(uint64_t n_chunks, const int64_t* __restrict__ chunk_root, const uint64_t* __restrict__ cuts,
                                                       const uint32_t* __restrict__ bsum, uint64_t* __restrict__ ranges) {
  __shared__ uint32_t red[SC_NT / 64 + 1];
  const uint64_t i = (uint64_t)blockIdx.x * SC_NT + threadIdx.x;
  uint32_t bnd = 0;
  if (i < n_chunks) {
    const bool prev = i > 0 && chunk_root[i - 1] != -1;
    bnd = (chunk_root[i] != -1) != prev;
  } else if (i == n_chunks) {
    bnd = n_chunks > 0 && chunk_root[i - 1] != -1;
  }
  uint32_t tot;
  const uint32_t j = bsum[blockIdx.x] + block_exclusive_scan<SC_NT>(bnd, red, &tot);
  if (bnd) ranges[j] = cuts[i];
}

// (start, end) -> (offset, length)
__global__ __launch_bounds__(SC_NT) void sc_lengths_kernel(uint64_t cap, const unsigned long long* __restrict__ counts, uint64_t* __restrict__ ranges) {
  const uint64_t r = (uint64_t)blockIdx.x * SC_NT + threadIdx.x;
  if (r < cap && r < counts[0]) ranges[2 * r + 1] -= ranges[2 * r];
}

extern "C" int hmse_scrub_attribute(uint64_t n, const uint8_t* status, const int64_t* dict, const uint8_t* ok, const uint8_t* got_sha,
                                    const uint8_t* want_sha, uint32_t check_digest, uint32_t max_depth_log2, uint64_t n_chunks,
                                    const int64_t* chunk_slot, const uint64_t* cuts, uint8_t* status_out, int64_t* root, int64_t* chunk_root,
                                    uint64_t* root_records, uint64_t* root_chunks, uint64_t* root_bytes, uint64_t* ranges, uint64_t* counts,
                                    void* ws, size_t ws_bytes, void* stream_) {
  HMSE_WS_ALIGNED(ws);
  if (!counts || n >= 0x7FFFFFFFull || n_chunks >= 0x7FFFFFFFull || max_depth_log2 > 30) return HMSE_EINVAL;
  if (n && (!status || !dict || !ok || !status_out || !root || !root_records || !root_chunks || !root_bytes)) return HMSE_EINVAL;
  if (n && check_digest && (!got_sha || !want_sha)) return HMSE_EINVAL;
  if (n_chunks && (!chunk_slot || !cuts || !chunk_root || !ranges)) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(counts, 0, 64, stream);
  if (n == 0 && n_chunks == 0) return HMSE_OK;
  if (!ws || ws_bytes < hmse_scrub_attribute_workspace_bytes_impl(n, n_chunks)) return HMSE_ENOSPC;
  WsCarver c(ws, ws_bytes);
  uint32_t* anc[2] = {c.take<uint32_t>(n + 1), c.take<uint32_t>(n + 1)};
  uint32_t* far[2] = {c.take<uint32_t>(n + 1), c.take<uint32_t>(n + 1)};
  uint32_t* live = c.take<uint32_t>(64);
  const uint64_t nbc = hmse_blocks(n_chunks + 1, SC_NT);
  uint32_t* bsum = c.take<uint32_t>(nbc + 1);
  if (!c.ok()) return HMSE_ENOSPC;
  unsigned long long* cnt = (unsigned long long*)counts;
  PROF_BEGIN(HMSE_STAGE_SCRUB_ATTRIBUTE, stream);
  if (n) {
    const uint32_t rounds = max_depth_log2 + 1;          // a chain of up to 2^rounds records (the caller cuts longer ones and cycles)
    HMSE_FILL(root_records, 0, 8 * n, stream);
    HMSE_FILL(root_chunks, 0, 8 * n, stream);
    HMSE_FILL(root_bytes, 0, 8 * n, stream);
    HMSE_FILL(live, 0, 4 * 64, stream);
    HMSE_FILL(live, 0x01, 4, stream);                    // round 0 runs
    const uint32_t nb = (uint32_t)hmse_blocks(n, SC_NT);
    sc_init_kernel<<<dim3(nb), dim3(SC_NT), 0, stream>>>(n, status, dict, ok, got_sha, want_sha, check_digest, status_out, anc[0], far[0]);
    HMSE_LAUNCH_CHECK();
    int cur = 0;
    for (uint32_t r = 0; r < rounds; r++) {
      sc_double_kernel<<<dim3(nb), dim3(SC_NT), 0, stream>>>(n, anc[cur], far[cur], anc[cur ^ 1], far[cur ^ 1], live + r, live + r + 1);
      HMSE_LAUNCH_CHECK();
      cur ^= 1;
    }
    sc_final_kernel<<<dim3(nb), dim3(SC_NT), 0, stream>>>(n, status, far[cur], status_out, root, (unsigned long long*)root_records, cnt);
    HMSE_LAUNCH_CHECK();
  }
  if (n_chunks) {
    const uint32_t nb = (uint32_t)nbc;
    sc_chunks_kernel<<<dim3(nb), dim3(SC_NT), 0, stream>>>(n_chunks, chunk_slot, n, cuts, root, chunk_root, (unsigned long long*)root_chunks,
                                                           (unsigned long long*)root_bytes, cnt, bsum);
    HMSE_LAUNCH_CHECK();
    // boundaries come in pairs, (start, end) of every damaged run: counts[0] = half their number
    block_sums_scan_kernel<SC_SCAN_NT, 1><<<dim3(1), dim3(SC_SCAN_NT), 0, stream>>>(bsum, nbc, counts, nullptr);
    HMSE_LAUNCH_CHECK();
    sc_emit_kernel<<<dim3(nb), dim3(SC_NT), 0, stream>>>(n_chunks, chunk_root, cuts, bsum, ranges);
    HMSE_LAUNCH_CHECK();
    const uint64_t cap = n_chunks / 2 + 1;
    sc_lengths_kernel<<<dim3((uint32_t)hmse_blocks(cap, SC_NT)), dim3(SC_NT), 0, stream>>>(cap, cnt, ranges);
    HMSE_LAUNCH_CHECK();
  }
  PROF_END(HMSE_STAGE_SCRUB_ATTRIBUTE, stream);
  return HMSE_OK;
}
