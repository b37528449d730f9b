// gc.hip — garbage collection of a store's dropped segments (hmse_amd/gc.py; refcount "for garbage collection", README.md:1268, 1886).
//
// hmse_gc_plan: the old chunk map + the dropped segments -> the L3 arrays of the surviving store, in the numbering a fresh ingest
// of the remainder would give it.  Six launches, no sort:
//   survive  per old chunk: its segment (binary search of its start in seg_off), alive or not, references per slot (atomicAdd);
//            block counts of the survivors (__syncthreads_count)
//   scan     one workgroup: exclusive scan of the block counts -> new chunk index of every block's first survivor; the total
//   rank     per old chunk: new chunk index (block scan + block base); first surviving reference per slot (atomicMin)
//   scatter  per old slot: slot id at its first surviving reference's position
//   count    per new chunk: block counts of the positions that hold a slot id; scan again -> new slot numbers in the order of
//            the first surviving references (a fresh ingest's stored-chunk order)
//   emit     per new chunk: first_occ, refcount (surviving references, counted from the map: the packed u16 may saturate),
//            digest; per new slot: uniq_ids, the old slot it came from and the inverse map
// hmse_record_gather: the dense DEFLATE streams of the surviving store from two sources (records reused from the old blob,
// records re-encoded by hmse_l1_deflate), one wavefront per record, 16-byte stores at 16-byte aligned destinations.
#include "common.h"
#include "blockops.h"

constexpr uint32_t GC_EMPTY = 0xFFFFFFFFu;
constexpr int GC_NT = 256;
constexpr int GC_SCAN_NT = 1024;

size_t hmse_gc_plan_workspace_bytes_impl(uint64_t n_chunks) {
  const uint64_t nb = hmse_blocks(n_chunks, GC_NT) + 1;
  // cnt u32[n_slots] + first u32[n_slots] + slot_at u32[n] + alive u8[n] + two block-sum arrays (n_slots <= n_chunks)
  return hmse_align_up(4 * n_chunks, 256) * 3 + hmse_align_up(n_chunks, 256) + 2 * hmse_align_up(4 * nb, 256) + 256;
}

__global__ __launch_bounds__(GC_NT) void gc_survive_kernel(const uint64_t* __restrict__ cuts, uint64_t n, const uint32_t* __restrict__ slot,
                                                          uint64_t n_slots, const uint64_t* __restrict__ seg_off, uint32_t n_seg,
                                                          const uint8_t* __restrict__ drop, uint8_t* __restrict__ alive, uint32_t* cnt,
                                                          uint32_t* __restrict__ bsum, uint32_t* status) {
  const uint64_t i = (uint64_t)blockIdx.x * GC_NT + threadIdx.x;
  int a = 0;
  if (i < n) {
    const uint64_t start = cuts[i];
    uint32_t lo = 0, hi = n_seg;                       // last segment whose start is <= the chunk's start
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (seg_off[mid] <= start) lo = mid; else hi = mid;
    }
    const uint32_t s = slot[i];
    if (s >= n_slots) atomicOr(status, 1u);
    else if (!drop[lo]) { a = 1; atomicAdd(&cnt[s], 1u); }
    alive[i] = (uint8_t)a;
  }
  const int c = __syncthreads_count(a);
  if (threadIdx.x == 0) bsum[blockIdx.x] = (uint32_t)c;
}

__global__ __launch_bounds__(GC_NT) void gc_rank_kernel(uint64_t n, const uint32_t* __restrict__ slot, const uint8_t* __restrict__ alive,
                                                       const uint32_t* __restrict__ bsum, uint32_t* first, int64_t* __restrict__ old_chunk) {
  __shared__ uint32_t red[GC_NT / 64 + 1];
  const uint64_t i = (uint64_t)blockIdx.x * GC_NT + threadIdx.x;
  const uint32_t a = i < n ? alive[i] : 0u;
  uint32_t tot;
  const uint32_t k = bsum[blockIdx.x] + block_exclusive_scan<GC_NT>(a, red, &tot);
  if (a) {
    old_chunk[k] = (int64_t)i;
    atomicMin(&first[slot[i]], k);
  }
}

__global__ __launch_bounds__(GC_NT) void gc_scatter_kernel(uint64_t n_slots, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ first,
                                                          uint32_t* __restrict__ slot_at) {
  const uint64_t s = (uint64_t)blockIdx.x * GC_NT + threadIdx.x;
  if (s < n_slots && cnt[s]) slot_at[first[s]] = (uint32_t)s;
}

__global__ __launch_bounds__(GC_NT) void gc_count_kernel(const uint64_t* __restrict__ counts, const uint32_t* __restrict__ slot_at,
                                                        uint32_t* __restrict__ bsum) {
  const uint64_t k = (uint64_t)blockIdx.x * GC_NT + threadIdx.x;
  const int m = k < counts[0] && slot_at[k] != GC_EMPTY;
  const int c = __syncthreads_count(m);
  if (threadIdx.x == 0) bsum[blockIdx.x] = (uint32_t)c;
}

__global__ __launch_bounds__(GC_NT) void gc_emit_kernel(const uint64_t* __restrict__ counts, const uint32_t* __restrict__ slot,
                                                       const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ first,
                                                       const uint32_t* __restrict__ slot_at, const uint32_t* __restrict__ bsum,
                                                       const int64_t* __restrict__ old_chunk, const uint8_t* __restrict__ digests_old,
                                                       int64_t* __restrict__ first_occ, uint32_t* __restrict__ refcount,
                                                       uint8_t* __restrict__ digests, int64_t* __restrict__ uniq_ids,
                                                       int64_t* __restrict__ old_slot, int64_t* __restrict__ new_slot_of_old) {
  __shared__ uint32_t red[GC_NT / 64 + 1];
  const uint64_t k = (uint64_t)blockIdx.x * GC_NT + threadIdx.x;
  const bool valid = k < counts[0];
  const uint32_t sa = valid ? slot_at[k] : GC_EMPTY;
  const uint32_t m = sa != GC_EMPTY;
  uint32_t tot;
  const uint32_t j = bsum[blockIdx.x] + block_exclusive_scan<GC_NT>(m, red, &tot);
  if (valid) {
    const uint32_t s = slot[old_chunk[k]];
    const uint32_t fo = first[s];
    first_occ[k] = (int64_t)fo;
    refcount[k] = fo == (uint32_t)k ? cnt[s] : 0u;
    const uint4* src = (const uint4*)(digests_old + 32 * (size_t)s);
    uint4* dst = (uint4*)(digests + 32 * (size_t)k);
    dst[0] = src[0];
    dst[1] = src[1];
  }
  if (m) {
    uniq_ids[j] = (int64_t)k;
    old_slot[j] = (int64_t)sa;
    new_slot_of_old[sa] = (int64_t)j;
  }
}

extern "C" int hmse_gc_plan(const uint64_t* cuts, uint64_t n_chunks, const uint32_t* slot, uint64_t n_slots, const uint64_t* seg_off,
                            uint32_t n_seg, const uint8_t* drop, const uint8_t* digests_old, uint64_t* counts, int64_t* old_chunk,
                            int64_t* first_occ, uint32_t* refcount, uint8_t* digests, int64_t* uniq_ids, int64_t* old_slot,
                            int64_t* new_slot_of_old, uint32_t* status, void* ws, size_t ws_bytes, void* stream_) {
  HMSE_WS_ALIGNED(ws);
  if (!counts || !status || n_seg == 0 || !seg_off || !drop) return HMSE_EINVAL;
  if (n_chunks >= 0x7FFFFFFFull || n_slots > n_chunks) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(counts, 0, 16, stream);
  HMSE_FILL(status, 0, 4, stream);
  if (n_chunks == 0) return HMSE_OK;
  if (!cuts || !slot || !digests_old || !old_chunk || !first_occ || !refcount || !digests || !uniq_ids || !old_slot || !new_slot_of_old)
    return HMSE_EINVAL;
  if (!ws || ws_bytes < hmse_gc_plan_workspace_bytes_impl(n_chunks)) return HMSE_ENOSPC;
  const uint64_t nb = hmse_blocks(n_chunks, GC_NT), nbs = hmse_blocks(n_slots, GC_NT);
  WsCarver c(ws, ws_bytes);
  uint32_t* cnt = c.take<uint32_t>(n_chunks);
  uint32_t* first = c.take<uint32_t>(n_chunks);
  uint32_t* slot_at = c.take<uint32_t>(n_chunks);
  uint8_t* alive = c.take<uint8_t>(n_chunks);
  uint32_t* bsum_a = c.take<uint32_t>(nb + 1);
  uint32_t* bsum_b = c.take<uint32_t>(nb + 1);
  if (!c.ok()) return HMSE_ENOSPC;
  HMSE_FILL(cnt, 0, hmse_align_up(4 * n_slots, 4), stream);
  HMSE_FILL(first, 0xFF, hmse_align_up(4 * n_slots, 4), stream);
  HMSE_FILL(slot_at, 0xFF, 4 * n_chunks, stream);
  if (n_slots) HMSE_FILL(new_slot_of_old, 0xFF, 8 * n_slots, stream);
  gc_survive_kernel<<<dim3((uint32_t)nb), dim3(GC_NT), 0, stream>>>(cuts, n_chunks, slot, n_slots, seg_off, n_seg, drop, alive, cnt, bsum_a, status);
  HMSE_LAUNCH_CHECK();
  block_sums_scan_kernel<GC_SCAN_NT><<<dim3(1), dim3(GC_SCAN_NT), 0, stream>>>(bsum_a, nb, counts, nullptr);
  HMSE_LAUNCH_CHECK();
  gc_rank_kernel<<<dim3((uint32_t)nb), dim3(GC_NT), 0, stream>>>(n_chunks, slot, alive, bsum_a, first, old_chunk);
  HMSE_LAUNCH_CHECK();
  if (n_slots) {
    gc_scatter_kernel<<<dim3((uint32_t)nbs), dim3(GC_NT), 0, stream>>>(n_slots, cnt, first, slot_at);
    HMSE_LAUNCH_CHECK();
  }
  gc_count_kernel<<<dim3((uint32_t)nb), dim3(GC_NT), 0, stream>>>(counts, slot_at, bsum_b);
  HMSE_LAUNCH_CHECK();
  block_sums_scan_kernel<GC_SCAN_NT><<<dim3(1), dim3(GC_SCAN_NT), 0, stream>>>(bsum_b, nb, counts + 1, nullptr);
  HMSE_LAUNCH_CHECK();
  gc_emit_kernel<<<dim3((uint32_t)nb), dim3(GC_NT), 0, stream>>>(counts, slot, cnt, first, slot_at, bsum_b, old_chunk, digests_old, first_occ,
                                                                 refcount, digests, uniq_ids, old_slot, new_slot_of_old);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

// ---- record gather: one wavefront per record ------------------------------------------------------------------------------
// wave_copy (blockops.h): 16-byte stores at aligned destinations, loads from wherever the source record starts (lba_unit may be 1).
__global__ __launch_bounds__(GC_NT) void gc_gather_kernel(const uint8_t* __restrict__ src0, uint64_t src0_bytes, const uint8_t* __restrict__ src1,
                                                         uint64_t src1_bytes, const uint64_t* __restrict__ src_off, const uint8_t* __restrict__ src_sel,
                                                         const uint64_t* __restrict__ dst_off, uint64_t n, uint8_t* __restrict__ dst,
                                                         uint64_t dst_bytes, uint32_t* status) {
  const uint64_t r = (uint64_t)blockIdx.x * (GC_NT / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (r >= n) return;
  const uint32_t lane = lane_id();
  const uint64_t d0 = dst_off[r], len = dst_off[r + 1] - d0, s0 = src_off[r];
  const bool one = src_sel[r] != 0;
  const uint8_t* src = one ? src1 : src0;
  const uint64_t cap = one ? src1_bytes : src0_bytes;
  if (d0 > dst_bytes || len > dst_bytes - d0 || s0 > cap || len > cap - s0) {
    if (lane == 0) atomicOr(status, 1u);
    return;
  }
  const uint8_t* s = src + s0;
  wave_copy(dst + d0, s, len, lane);
}

extern "C" int hmse_record_gather(const uint8_t* src0, uint64_t src0_bytes, const uint8_t* src1, uint64_t src1_bytes, const uint64_t* src_off,
                                  const uint8_t* src_sel, const uint64_t* dst_off, uint64_t n, uint8_t* dst, uint64_t dst_bytes,
                                  uint32_t* status, void* stream_) {
  if (!status) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n == 0) return HMSE_OK;
  if (!src_off || !src_sel || !dst_off || (!dst && dst_bytes) || (!src0 && src0_bytes) || (!src1 && src1_bytes)) return HMSE_EINVAL;
  if (n >= (1ull << 33)) return HMSE_EINVAL;
  const uint64_t blocks = (n + GC_NT / 64 - 1) / (GC_NT / 64);
  PROF_BEGIN(HMSE_STAGE_RECORD_GATHER, stream);
  gc_gather_kernel<<<dim3((uint32_t)blocks), dim3(GC_NT), 0, stream>>>(src0, src0_bytes, src1, src1_bytes, src_off, src_sel, dst_off, n, dst,
                                                                       dst_bytes, status);
  PROF_END(HMSE_STAGE_RECORD_GATHER, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
