// tally.hip — which texts did the ranges of a search cover, and how often each (hmse_amd/find.py tally / tally_regex;
// include/hmse_tally.h hmse_tally_*; a library of its own, libhmse_tally.so, beside libhmse_hip.so).
//
// find / find_regex / lines answer where something occurs and which lines it lies in.  `grep -o RX | sort | uniq -c | sort -rn` asks which
// values the expression took and how often; the route to that used to leave the GPU (text(), .cpu(), one Python bytes object per
// occurrence into a Counter).  Grouping ranges by the bytes they cover needs two things from the device, both read through the chunk map
// as lines_gather_kernel reads (a range does not stop at a chunk boundary, chunks may be 0, 1 or 2 bytes long):
//   (1) tally_keys_kernel — one wavefront per range: a 64-bit key of the (folded) text, defined bit for bit in the header.  The two 32-bit
//       sums a = sum (f(b_t) + 1) M^t are linear, so lane l owns the text indices t = l (mod 64), keeps M^t for its next t and adds
//       privately: no cross-lane operation inside any loop, two wave_sums after the walk, lane 0 mixes and stores.
//   (2) tally_same_kernel — one wavefront per range: is range i byte for byte the range rep[i]?  The key only buckets; this decides.  Both
//       ranges are walked in lockstep, a trip covers what is contiguous in raw for both, one ballot per trip ends the walk at the first
//       difference.
// tally_ranges_kernel proves every range (and rep) first, tables_validate_kernel the tables: a refused call reads nothing through them and
// writes 0 everywhere.  The range index is wave-uniform (readfirstlane), so the one last_le search in cuts and every table entry are
// scalar, and every loop has a scalar counter and exit (tools/isa_audit.py).  No LDS, no workspace.
#include "common.h"
#include "../../include/hmse_tally.h"
#include "chunkmap.h"
#include "blockops.h"

constexpr int TALLY_NT = 256;                // four wavefronts = four ranges per workgroup
constexpr uint32_t TALLY_TRIP = 64;          // bytes one trip looks at: one per lane
constexpr uint32_t TALLY_MAX_BLOCKS = 2048;  // of the two checking kernels; the rest by the grid stride

constexpr uint32_t tally_pow(uint32_t m, uint32_t e) {
  uint32_t r = 1;
  for (; e; e >>= 1, m *= m) if (e & 1) r *= m;
  return r;
}
constexpr uint32_t TALLY_M1_64 = tally_pow(HMSE_TALLY_M1, 64), TALLY_M2_64 = tally_pow(HMSE_TALLY_M2, 64);

// ---- ranges -------------------------------------------------------------------------------------------------------------------
// One thread per range: status bit 1 for a range that descends or leaves the corpus and for a rep[i] outside [0, n) (rep == nullptr:
// the keys call has none).  Reads cuts only when the tables are consistent.
__global__ __launch_bounds__(TALLY_NT) void tally_ranges_kernel(const uint64_t* __restrict__ cuts, uint64_t n_chunks, const uint64_t* __restrict__ start,
                                                                const uint64_t* __restrict__ end, const uint64_t* __restrict__ rep, uint64_t n,
                                                                uint32_t* status) {
  if (*status & 2u) return;
  const uint64_t N = n_chunks ? cuts[n_chunks] : 0;
  const uint64_t stride = (uint64_t)gridDim.x * TALLY_NT;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * TALLY_NT + threadIdx.x; i < n; i += stride) {
    const uint64_t s = start[i], e = end[i];
    bad |= s > e || e > N;
    if (rep) bad |= rep[i] >= n;
  }
  if (bad) atomicOr(status, 2u);
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TALLY_NT) void tally_keys_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                              const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                              uint64_t n_chunks, const uint64_t* __restrict__ start, const uint64_t* __restrict__ end,
                                                              uint64_t n, uint32_t fold, uint64_t seed, uint32_t key_bits,
                                                              uint64_t* __restrict__ key, const uint32_t* status) {
  const uint64_t i = (uint64_t)blockIdx.x * (TALLY_NT / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= n) return;
  const uint32_t lane = lane_id();
  if (__builtin_amdgcn_readfirstlane((int)*status)) {  // refused (tables_validate_kernel, tally_ranges_kernel): nothing is read through the tables
    if (lane == 0) key[i] = 0;
    return;
  }
  const uint64_t s = start[i], e = end[i];
  uint32_t pw1 = 1, pw2 = 1;                           // M^lane: six squarings, driven by the lane's bits
  {
    uint32_t b1 = HMSE_TALLY_M1, b2 = HMSE_TALLY_M2;
#pragma unroll
    for (int bit = 0; bit < 6; bit++) {
      if ((lane >> bit) & 1u) { pw1 *= b1; pw2 *= b2; }
      b1 *= b1; b2 *= b2;
    }
  }
  uint32_t a1 = 0, a2 = 0;
  uint64_t c = s < e ? last_le(cuts, 0, n_chunks, s) : 0, p = s;
  while (p < e) {
    const uint64_t c0 = cuts[c], c1 = cuts[c + 1];
    if (p == c1) { c++; continue; }                    // p < e <= N: a chunk follows
    const uint64_t q = c1 < e ? c1 : e;                // the piece [p, q) of chunk c
    const uint8_t* src = raw + raw_off[slot[c]] + (p - c0);
    for (uint64_t o = 0; o < q - p; o += TALLY_TRIP) {
      const uint64_t left = q - p - o;
      const uint32_t w = left < TALLY_TRIP ? (uint32_t)left : TALLY_TRIP;
      const uint32_t rot = (uint32_t)(p - s + o) & 63u;                  // the text index of the trip's first byte, mod 64: its owner
      const uint32_t j = (lane - rot) & 63u;                            // this lane's byte of the window: one contiguous load, rotated
      if (j < w) {
        uint32_t b = src[o + j];
        if (fold) b = fold_byte(b);
        a1 += (b + 1u) * pw1; a2 += (b + 1u) * pw2;
        pw1 *= TALLY_M1_64; pw2 *= TALLY_M2_64;
      }
    }
    p = q;
  }
  const uint32_t s1 = wave_sum(a1), s2 = wave_sum(a2);
  if (lane == 0) {
    uint64_t x = ((uint64_t)s1 | ((uint64_t)s2 << 32)) ^ ((e - s) * HMSE_TALLY_LEN) ^ (seed * HMSE_TALLY_SEED);
    x ^= x >> 33; x *= HMSE_TALLY_MIX1; x ^= x >> 33; x *= HMSE_TALLY_MIX2; x ^= x >> 33;
    key[i] = key_bits >= 64 ? x : x & ((1ull << key_bits) - 1ull);
  }
}

// ---- same ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TALLY_NT) void tally_same_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                              const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                              uint64_t n_chunks, const uint64_t* __restrict__ start, const uint64_t* __restrict__ end,
                                                              const uint64_t* __restrict__ rep, uint64_t n, uint32_t fold,
                                                              uint8_t* __restrict__ same, const uint32_t* status) {
  const uint64_t i = (uint64_t)blockIdx.x * (TALLY_NT / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= n) return;
  const uint32_t lane = lane_id();
  if (__builtin_amdgcn_readfirstlane((int)*status)) {
    if (lane == 0) same[i] = 0;
    return;
  }
  const uint64_t r = rep[i];
  const uint64_t si = start[i], sr = start[r];
  uint64_t left = end[i] - si;
  bool eq = left == end[r] - sr;
  if (eq && r != i && left) {                          // rep[i] == i, a length mismatch and two empty texts: no byte is read
    uint64_t ci = last_le(cuts, 0, n_chunks, si), cr = last_le(cuts, 0, n_chunks, sr), pi = si, pr = sr;
    while (left) {
      const uint64_t i1 = cuts[ci + 1], r1 = cuts[cr + 1];
      if (pi == i1) { ci++; continue; }                // pi + left <= N with left > 0: a chunk follows (and likewise for pr)
      if (pr == r1) { cr++; continue; }
      uint64_t w = i1 - pi < r1 - pr ? i1 - pi : r1 - pr;                // contiguous in raw for both ranges
      if (w > left) w = left;
      if (w > TALLY_TRIP) w = TALLY_TRIP;
      bool differ = false;
      if (lane < w) {
        uint32_t x = raw[raw_off[slot[ci]] + (pi - cuts[ci]) + lane], y = raw[raw_off[slot[cr]] + (pr - cuts[cr]) + lane];
        if (fold) { x = fold_byte(x); y = fold_byte(y); }
        differ = x != y;
      }
      if (__ballot(differ)) { eq = false; break; }     // wave-uniform: every lane sees the same mask
      pi += w; pr += w; left -= w;
    }
  }
  if (lane == 0) same[i] = eq ? 1 : 0;
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
// The table rules of chunkmap.h (status bit 1) and cuts[0] != 0, as lines.hip checks them: the ranges come from the caller, and a
// position below cuts[0] would lie in no chunk.  cuts goes in as the chunk_out as well.
static int tally_validate(const uint64_t* raw_off, uint64_t n_rec, uint64_t raw_bytes, const uint64_t* cuts, const uint64_t* slot,
                          uint64_t n_chunks, uint32_t* status, hipStream_t stream) {
  return tables_validate<TALLY_NT>(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, /*chunk_out=*/cuts, status, TALLY_MAX_BLOCKS, stream);
}

static bool tally_args_bad(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                           const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, uint64_t n, uint32_t flags,
                           const uint32_t* status) {
  if (!status || n >= (1ull << 33) || (flags & ~(uint32_t)HMSE_FIND_IGNORE_CASE)) return true;
  if ((raw_bytes && !raw) || ((n_rec || n_chunks) && !raw_off) || (n_chunks && (!cuts || !slot))) return true;
  return n && (!start || !end);
}

static int tally_check(const uint64_t* raw_off, uint64_t n_rec, uint64_t raw_bytes, const uint64_t* cuts, const uint64_t* slot,
                       uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* rep, uint64_t n, uint32_t* status,
                       hipStream_t stream) {
  int rc = tally_validate(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, status, stream);
  if (rc != HMSE_OK) return rc;
  uint64_t nb = (n + TALLY_NT - 1) / TALLY_NT;
  if (nb > TALLY_MAX_BLOCKS) nb = TALLY_MAX_BLOCKS;
  tally_ranges_kernel<<<dim3((uint32_t)nb), dim3(TALLY_NT), 0, stream>>>(cuts, n_chunks, start, end, rep, n, status);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_tally_keys(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                               const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, uint64_t n, uint32_t flags,
                               uint64_t seed, uint32_t key_bits, uint64_t* key, uint32_t* status, void* stream_) {
  if (tally_args_bad(raw, raw_bytes, raw_off, n_rec, cuts, slot, n_chunks, start, end, n, flags, status)) return HMSE_EINVAL;
  if (key_bits < 1 || key_bits > 64 || (n && !key)) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n == 0) return HMSE_OK;
  int rc = tally_check(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, start, end, nullptr, n, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t blocks = (n + TALLY_NT / 64 - 1) / (TALLY_NT / 64);
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  tally_keys_kernel<<<dim3((uint32_t)blocks), dim3(TALLY_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, start, end, n,
                                                                           flags & HMSE_FIND_IGNORE_CASE, seed, key_bits, key, status);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_tally_same(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                               const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* rep,
                               uint64_t n, uint32_t flags, uint8_t* same, uint32_t* status, void* stream_) {
  if (tally_args_bad(raw, raw_bytes, raw_off, n_rec, cuts, slot, n_chunks, start, end, n, flags, status)) return HMSE_EINVAL;
  if (n && (!rep || !same)) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n == 0) return HMSE_OK;
  int rc = tally_check(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, start, end, rep, n, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t blocks = (n + TALLY_NT / 64 - 1) / (TALLY_NT / 64);
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  tally_same_kernel<<<dim3((uint32_t)blocks), dim3(TALLY_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, start, end, rep, n,
                                                                           flags & HMSE_FIND_IGNORE_CASE, same, status);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
