// order.hip — the ranges of a search in the lexicographic order of the texts they cover (hmse_amd/find.py sort / sort_regex / order_ranges;
// include/hmse_order.h hmse_order_*; a library of its own, libhmse_order.so, beside libhmse_hip.so).
//
// tally answers which values an expression took and how often, most frequent first.  `grep -o RX | sort`, `sort -u`, `sort | uniq -c`, a
// rank, a median and a join ask for the values in ORDER, and the route to that used to leave the GPU (text(), .cpu(), one Python bytes
// object per occurrence into sorted()).  Ordering ranges by the bytes they cover is a most-significant-bytes-first radix sort whose
// digits the device reads through the chunk map, as lines_gather_kernel reads (a range does not stop at a chunk boundary, chunks may be
// 0, 1 or 2 bytes long, a deduplicated record lies at several places):
//   (1) order_keys_kernel — one THREAD per range: seven (folded) bytes of the text from depth[i] on and the state of its end in one
//       integer that sorts like the texts, defined bit for bit in the header.  One last_le search in cuts and at most seven bytes behind
//       it: a wavefront per range would keep 57 lanes idle for the whole search, and nothing here is shared between lanes, so the
//       divergent loops (the search, the seven bytes) hold loads and integer work only (tools/isa_audit.py).
//   (2) order_lcp_kernel — one WAVEFRONT per range: how many bytes do range i and range rep[i] share from text index from[i] on?  What
//       the keys could not split agrees in at least seven more bytes, often in hundreds (duplicated lines): the rounds skip them in one
//       call.  Both ranges are walked in lockstep from from[i] (the bytes in front of it are promised equal and not read), a trip covers
//       what is contiguous in raw for both, one ballot per trip, the first set bit of the mismatch mask is the answer.
// order_ranges_kernel proves every range, depth, rep and from first, tables_validate_kernel the tables: a refused call reads nothing
// through them and writes 0 everywhere.  In the LCP kernel the range index is wave-uniform (readfirstlane), so its two last_le searches
// and every table entry are scalar, and its loop has a scalar counter and exit.  No LDS, no workspace, no scratch; every launch covers
// its n directly.
#include "common.h"
#include "../../include/hmse_order.h"
#include "chunkmap.h"
#include "blockops.h"

constexpr int ORDER_NT = 256;                // the checks and the keys: a range per thread; the LCP: four wavefronts = four ranges per workgroup
constexpr uint32_t ORDER_TRIP = 64;          // bytes one trip of the LCP walk looks at: one per lane
constexpr uint64_t ORDER_VALIDATE_BLOCKS = 2048;   // of tables_validate_kernel (chunkmap.h), which strides over the rest itself

// the smaller of two lengths
__device__ __forceinline__ uint64_t order_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- ranges -------------------------------------------------------------------------------------------------------------------
// One thread per range: status bit 1 for a range that descends or leaves the corpus, a depth[i] > L_i (the keys call; depth == nullptr:
// the LCP call has none), a rep[i] outside [0, n) and a from[i] > min(L_i, L_rep[i]) (the LCP call).  Reads cuts only when the tables
// are consistent.  A partner's own range is proved by its own thread: a descending one gives a huge L_rep here and is caught there.
__global__ __launch_bounds__(ORDER_NT) void order_ranges_kernel(const uint64_t* __restrict__ cuts, uint64_t n_chunks, const uint64_t* __restrict__ start,
                                                                const uint64_t* __restrict__ end, const uint64_t* __restrict__ depth,
                                                                const uint64_t* __restrict__ rep, const uint64_t* __restrict__ from, uint64_t n,
                                                                uint32_t* status) {
  if (*status & 2u) return;
  const uint64_t i = (uint64_t)blockIdx.x * ORDER_NT + threadIdx.x;
  if (i >= n) return;
  const uint64_t N = n_chunks ? cuts[n_chunks] : 0;
  const uint64_t s = start[i], e = end[i];
  bool bad = s > e || e > N;
  if (!bad && depth) bad = depth[i] > e - s;
  if (!bad && rep) {
    const uint64_t r = rep[i];
    bad = r >= n;
    if (!bad) bad = from[i] > order_min(e - s, end[r] - start[r]);
  }
  if (bad) atomicOr(status, 2u);
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ORDER_NT) void order_keys_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                              const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                              uint64_t n_chunks, const uint64_t* __restrict__ start, const uint64_t* __restrict__ end,
                                                              const uint64_t* __restrict__ depth, uint64_t n, uint32_t fold,
                                                              uint64_t* __restrict__ key, const uint32_t* status) {
  const uint64_t i = (uint64_t)blockIdx.x * ORDER_NT + threadIdx.x;
  if (i >= n) return;
  if (*status) {                                       // refused (tables_validate_kernel, order_ranges_kernel): nothing is read through the tables
    key[i] = 0;
    return;
  }
  const uint64_t p = start[i] + depth[i], left = end[i] - p;             // depth[i] <= L_i: proved
  const uint32_t m = (uint32_t)order_min(left, HMSE_ORDER_KEY_BYTES);
  uint64_t k = 0;
  if (m) {
    uint64_t c = last_le(cuts, 0, n_chunks, p);        // p < end[i] <= N: p lies in a chunk, and so does every byte read below
    for (uint32_t j = 0; j < m; j++) {
      uint32_t b = corpus_byte(raw, raw_off, cuts, slot, p + j, c);
      if (fold) b = fold_byte(b);
      k |= (uint64_t)b << (8u * (HMSE_ORDER_KEY_BYTES - 1u - j));
    }
  }
  key[i] = (k << 4) | order_min(left, HMSE_ORDER_R_MORE);
}

// ---- lcp ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ORDER_NT) void order_lcp_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                             const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                             uint64_t n_chunks, const uint64_t* __restrict__ start, const uint64_t* __restrict__ end,
                                                             const uint64_t* __restrict__ rep, const uint64_t* __restrict__ from, uint64_t n,
                                                             uint32_t fold, uint64_t* __restrict__ lcp, const uint32_t* status) {
  const uint64_t i = (uint64_t)blockIdx.x * (ORDER_NT / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= n) return;
  const uint32_t lane = lane_id();
  if (__builtin_amdgcn_readfirstlane((int)*status)) {
    if (lane == 0) lcp[i] = 0;
    return;
  }
  const uint64_t r = rep[i];
  const uint64_t si = start[i], sr = start[r];
  uint64_t t = end[i] - si;                            // rep[i] == i: L_i, and no byte is read
  if (r != i) {
    const uint64_t f = from[i];                        // f <= min(L_i, L_rep): proved
    uint64_t left = order_min(t, end[r] - sr) - f;
    t = f;
    if (left) {
      uint64_t pi = si + f, pr = sr + f;               // the walk starts at from[i]: the searches land there, not on the ranges' starts
      uint64_t ci = last_le(cuts, 0, n_chunks, pi), cr = last_le(cuts, 0, n_chunks, pr);
      while (left) {
        const uint64_t i1 = cuts[ci + 1], r1 = cuts[cr + 1];
        if (pi == i1) { ci++; continue; }              // pi + left <= N with left > 0: a chunk follows (and likewise for pr)
        if (pr == r1) { cr++; continue; }
        const uint64_t w = order_min(order_min(i1 - pi, r1 - pr), order_min(left, ORDER_TRIP));      // contiguous in raw for both ranges
        bool differ = false;
        if (lane < w) {
          uint32_t x = raw[raw_off[slot[ci]] + (pi - cuts[ci]) + lane], y = raw[raw_off[slot[cr]] + (pr - cuts[cr]) + lane];
          if (fold) { x = fold_byte(x); y = fold_byte(y); }
          differ = x != y;
        }
        const unsigned long long mask = __ballot(differ);                // wave-uniform: every lane sees the same mask
        if (mask) { t += (uint64_t)__builtin_ctzll(mask); break; }
        pi += w; pr += w; left -= w; t += w;
      }
    }
  }
  if (lane == 0) lcp[i] = t;
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
// The table rules of chunkmap.h (status bit 1) and cuts[0] != 0, as tally.hip checks them: cuts goes in as the chunk_out as well.
static bool order_args_bad(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                           const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, uint64_t n, uint32_t flags,
                           const uint32_t* status) {
  if (!status || n >= (1ull << 31) || (flags & ~(uint32_t)HMSE_FIND_IGNORE_CASE)) return true;
  if ((raw_bytes && !raw) || ((n_rec || n_chunks) && !raw_off) || (n_chunks && (!cuts || !slot))) return true;
  return n && (!start || !end);
}

// tables, then ranges: every launch covers its n directly (n < 2^31 keeps ceil(n / ORDER_NT) in range)
static int order_check(const uint64_t* raw_off, uint64_t n_rec, uint64_t raw_bytes, const uint64_t* cuts, const uint64_t* slot,
                       uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* depth, const uint64_t* rep,
                       const uint64_t* from, uint64_t n, uint32_t* status, hipStream_t stream) {
  int rc = tables_validate<ORDER_NT>(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, /*chunk_out=*/cuts, status, ORDER_VALIDATE_BLOCKS, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t blocks = (n + ORDER_NT - 1) / ORDER_NT;
  order_ranges_kernel<<<dim3((uint32_t)blocks), dim3(ORDER_NT), 0, stream>>>(cuts, n_chunks, start, end, depth, rep, from, n, status);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_order_keys(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                               const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* depth,
                               uint64_t n, uint32_t flags, uint64_t* key, uint32_t* status, void* stream_) {
  if (order_args_bad(raw, raw_bytes, raw_off, n_rec, cuts, slot, n_chunks, start, end, n, flags, status)) return HMSE_EINVAL;
  if (n && (!depth || !key)) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n == 0) return HMSE_OK;
  int rc = order_check(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, start, end, depth, nullptr, nullptr, n, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t blocks = (n + ORDER_NT - 1) / ORDER_NT;
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  order_keys_kernel<<<dim3((uint32_t)blocks), dim3(ORDER_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, start, end, depth, n,
                                                                           flags & HMSE_FIND_IGNORE_CASE, key, status);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_order_lcp(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                              const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* rep,
                              const uint64_t* from, uint64_t n, uint32_t flags, uint64_t* lcp, uint32_t* status, void* stream_) {
  if (order_args_bad(raw, raw_bytes, raw_off, n_rec, cuts, slot, n_chunks, start, end, n, flags, status)) return HMSE_EINVAL;
  if (n && (!rep || !from || !lcp)) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n == 0) return HMSE_OK;
  int rc = order_check(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, start, end, nullptr, rep, from, n, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t blocks = (n + ORDER_NT / 64 - 1) / (ORDER_NT / 64);
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  order_lcp_kernel<<<dim3((uint32_t)blocks), dim3(ORDER_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, start, end, rep, from, n,
                                                                          flags & HMSE_FIND_IGNORE_CASE, lcp, status);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
