// lines.hip — from a search hit to the line it lies in (hmse_amd/find.py lines / text / grep; include/hmse.h hmse_lines_*).
//
// find.hip and findset.hip answer "at which corpus offsets does this byte string occur".  What a user wants is the line (the delimited
// record) around the offset, how many lines match, a few lines of context and the text.  The route from an offset to its line used to
// leave the GPU: read_store decodes the whole corpus, .cpu() moves it, the host runs bytes.rfind / bytes.find per hit.  Here the walk
// stays where the finder already holds every unique record decoded, and goes through the chunk map as find_seams_kernel does: corpus
// byte p of chunk c is raw[raw_off[slot[c]] + p - cuts[c]].  A line does not stop at a chunk boundary, a deduplicated record has other
// neighbours at each of its places, and chunks may be 0, 1 or 2 bytes long.
//   (1) lines_extent_kernel — one wavefront per hit.  The hit index is wave-uniform, so the hit's chunk is ONE binary search in cuts on
//       scalar values.  Backward from o - 1 and forward from o the wavefront looks at LINES_TRIP bytes per trip, one per lane, clipped to
//       the chunk and to `reach`; one ballot gives the trip's delimiter mask, the count still needed lives in an SGPR, and the trip that
//       holds the wanted delimiter picks it by rank (the popcount of the mask above the lane going backward, below it going forward)
//       with one more ballot.  Every loop — trips inside a chunk, chunks with the empty ones skipped — has a scalar counter and exit.
//   (2) lines_gather_kernel — one wavefront per range [start, end): per chunk piece one wave_copy (blockops.h: aligned 16-byte stores,
//       loads from wherever the piece starts in raw).  lines_ranges_kernel proves every range and the prefix sum first: a refused call writes nothing.
// No kernel holds an atomic or a cross-lane operation inside a loop that lanes leave at different times (tools/isa_audit.py).
#include "common.h"
#include "chunkmap.h"
#include "blockops.h"

constexpr int LINES_NT = 256;                // four wavefronts = four hits (or ranges) per workgroup
constexpr uint32_t LINES_TRIP = 64;          // bytes one trip looks at: one per lane
constexpr uint32_t LINES_MAX_BLOCKS = 2048;  // of the two checking kernels; the rest by the grid stride

// ---- extent -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LINES_NT) void lines_extent_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                                const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                                uint64_t n_chunks, const uint64_t* __restrict__ pos, uint64_t n, uint32_t delim,
                                                                uint32_t before, uint32_t after, uint32_t reach, uint64_t* __restrict__ start,
                                                                uint64_t* __restrict__ end, uint8_t* __restrict__ flags, uint32_t* status) {
  const uint64_t i = (uint64_t)blockIdx.x * (LINES_NT / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= n) return;
  const uint32_t lane = lane_id();
  const bool tables = ((uint32_t)__builtin_amdgcn_readfirstlane((int)*status) & 2u) == 0;       // tables_validate_kernel ran before this one
  const uint64_t N = tables && n_chunks ? cuts[n_chunks] : 0;
  const uint64_t o = pos[i];
  if (!tables || o >= N) {
    if (lane == 0) {
      start[i] = 0; end[i] = 0; flags[i] = (uint8_t)HMSE_LINES_BAD;
      if (tables) atomicOr(status, 1u);
    }
    return;
  }
  const uint64_t R = reach;
  const uint64_t lo = o > R ? o - R : 0, hi = R < N - o ? o + R : N;      // what may be looked at: [lo, o) and [o, hi)
  const uint64_t c_o = last_le(cuts, 0, n_chunks, o);
  uint32_t fl = 0;

  // ---- backward: the (before + 1)-th delimiter met below o.  More than `reach` cannot be met: the count is clipped, not the answer ----
  uint64_t st = lo;
  {
    uint32_t need = (before < HMSE_LINES_MAX_REACH ? before : HMSE_LINES_MAX_REACH) + 1u;
    uint64_t c = c_o, p = o;                           // [lo, p) is still to be looked at; p lies in chunk c or at its end
    bool found = false;
    while (p > lo && !found) {
      const uint64_t c0 = cuts[c];
      if (p == c0) { c--; continue; }                  // chunk c is used up (or empty): p > lo >= 0, so there is one below
      const uint64_t floor = c0 > lo ? c0 : lo;
      const uint8_t* src = raw + raw_off[slot[c]] + (floor - c0);
      while (p > floor) {
        const uint32_t w = p - floor < LINES_TRIP ? (uint32_t)(p - floor) : LINES_TRIP;
        const uint64_t q = p - w;                      // lane l looks at corpus byte q + l
        const bool is = lane < w && src[(q - floor) + lane] == delim;
        const uint64_t m = __ballot(is);
        const uint32_t cnt = (uint32_t)__builtin_popcountll(m);
        if (cnt >= need) {
          const uint32_t above = cnt - mbcnt64(m) - (is ? 1u : 0u);      // delimiters of this trip nearer to o than this lane's
          const uint64_t sel = __ballot(is && above == need - 1u);
          st = q + (uint32_t)__builtin_ctzll(sel) + 1;
          found = true;
          break;
        }
        need -= cnt;
        p = q;
      }
    }
    if (!found && o > R) fl |= HMSE_LINES_START_CUT;   // stopped by reach in front of the corpus's first byte
  }

  // ---- forward: the (after + 1)-th delimiter met at or behind o ----
  uint64_t en = hi;
  {
    uint32_t need = (after < HMSE_LINES_MAX_REACH ? after : HMSE_LINES_MAX_REACH) + 1u;
    uint64_t c = c_o, p = o;                           // [p, hi) is still to be looked at
    bool found = false;
    while (p < hi && !found) {
      const uint64_t c0 = cuts[c], c1 = cuts[c + 1];
      if (p == c1) { c++; continue; }                  // p < hi <= N: a chunk follows
      const uint64_t ceil = c1 < hi ? c1 : hi;
      const uint8_t* src = raw + raw_off[slot[c]];
      while (p < ceil) {
        const uint32_t w = ceil - p < LINES_TRIP ? (uint32_t)(ceil - p) : LINES_TRIP;
        const bool is = lane < w && src[(p - c0) + lane] == delim;
        const uint64_t m = __ballot(is);
        const uint32_t cnt = (uint32_t)__builtin_popcountll(m);
        if (cnt >= need) {
          const uint64_t sel = __ballot(is && mbcnt64(m) == need - 1u);
          en = p + (uint32_t)__builtin_ctzll(sel);
          found = true;
          break;
        }
        need -= cnt;
        p += w;
      }
    }
    if (!found && R < N - o) fl |= HMSE_LINES_END_CUT;
  }
  if (lane == 0) { start[i] = st; end[i] = en; flags[i] = (uint8_t)fl; }
}

// ---- gather -------------------------------------------------------------------------------------------------------------------
// One thread per range: status bit 1 for a range that descends or leaves the corpus, and for an out_off that is not the prefix sum of
// the lengths; thread 0: bit 0 for out_off[n] > out_cap.  Reads cuts only when the tables are consistent.
__global__ __launch_bounds__(LINES_NT) void lines_ranges_kernel(const uint64_t* __restrict__ cuts, uint64_t n_chunks, const uint64_t* __restrict__ start,
                                                                const uint64_t* __restrict__ end, const uint64_t* __restrict__ out_off, uint64_t n,
                                                                uint64_t out_cap, uint32_t* status) {
  if (*status & 2u) return;
  const uint64_t N = n_chunks ? cuts[n_chunks] : 0;
  const uint64_t stride = (uint64_t)gridDim.x * LINES_NT;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * LINES_NT + threadIdx.x; i < n; i += stride) {
    const uint64_t s = start[i], e = end[i], a = out_off[i], b = out_off[i + 1];
    bad |= s > e || e > N || b < a || b - a != e - s;
    if (i == 0 && out_off[n] > out_cap) atomicOr(status, 1u);
  }
  if (bad) atomicOr(status, 2u);
}

__global__ __launch_bounds__(LINES_NT) void lines_gather_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                                const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                                uint64_t n_chunks, const uint64_t* __restrict__ start, const uint64_t* __restrict__ end,
                                                                const uint64_t* __restrict__ out_off, uint64_t n, uint8_t* __restrict__ out,
                                                                const uint32_t* status) {
  const uint64_t i = (uint64_t)blockIdx.x * (LINES_NT / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= n || __builtin_amdgcn_readfirstlane((int)*status)) return;      // a refused call writes nothing (tables_validate_kernel, lines_ranges_kernel)
  const uint32_t lane = lane_id();
  const uint64_t s = start[i], e = end[i];
  if (s >= e) return;
  uint8_t* dst = out + out_off[i];
  uint64_t c = last_le(cuts, 0, n_chunks, s), p = s;
  while (p < e) {
    const uint64_t c0 = cuts[c], c1 = cuts[c + 1];
    if (p == c1) { c++; continue; }                    // p < e <= N: a chunk follows
    const uint64_t q = c1 < e ? c1 : e, len = q - p;   // the piece [p, q) of chunk c
    wave_copy(dst + (p - s), raw + raw_off[slot[c]] + (p - c0), len, lane);
    p = q;
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
// The table rules of chunkmap.h (status bit 1) and cuts[0] != 0: here the positions come from the caller, and one below cuts[0] would lie
// in no chunk.  It is the rule chunk_out[0] != 0, so cuts goes in as the chunk_out as well.  Every later kernel of the call reads
// nothing through the tables when it finds the bit.
static int lines_validate(const uint64_t* raw_off, uint64_t n_rec, uint64_t raw_bytes, const uint64_t* cuts, const uint64_t* slot,
                          uint64_t n_chunks, uint32_t* status, hipStream_t stream) {
  return tables_validate<LINES_NT>(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, /*chunk_out=*/cuts, status, LINES_MAX_BLOCKS, stream);
}

static bool lines_tables_null(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                              const uint64_t* slot, uint64_t n_chunks) {
  return (raw_bytes && !raw) || ((n_rec || n_chunks) && !raw_off) || (n_chunks && (!cuts || !slot));
}

extern "C" int hmse_lines_extent(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                                 const uint64_t* slot, uint64_t n_chunks, const uint64_t* pos, uint64_t n, uint32_t delim, uint32_t before,
                                 uint32_t after, uint32_t reach, uint64_t* start, uint64_t* end, uint8_t* flags, uint32_t* status,
                                 void* stream_) {
  if (!status || delim > 255u || reach == 0 || reach > HMSE_LINES_MAX_REACH || n >= (1ull << 33)) return HMSE_EINVAL;
  if (n && (!pos || !start || !end || !flags || lines_tables_null(raw, raw_bytes, raw_off, n_rec, cuts, slot, n_chunks))) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n == 0) return HMSE_OK;
  int rc = lines_validate(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t blocks = (n + LINES_NT / 64 - 1) / (LINES_NT / 64);
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  lines_extent_kernel<<<dim3((uint32_t)blocks), dim3(LINES_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, pos, n, delim, before, after,
                                                                             reach, start, end, flags, status);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_lines_gather(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                                 const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* out_off,
                                 uint64_t n, uint8_t* out, uint64_t out_cap, uint32_t* status, void* stream_) {
  if (!status || n >= (1ull << 33) || (out_cap && !out)) return HMSE_EINVAL;
  if (n && (!start || !end || !out_off || lines_tables_null(raw, raw_bytes, raw_off, n_rec, cuts, slot, n_chunks))) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n == 0) return HMSE_OK;
  int rc = lines_validate(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, status, stream);
  if (rc != HMSE_OK) return rc;
  uint64_t nb = (n + LINES_NT - 1) / LINES_NT;
  if (nb > LINES_MAX_BLOCKS) nb = LINES_MAX_BLOCKS;
  lines_ranges_kernel<<<dim3((uint32_t)nb), dim3(LINES_NT), 0, stream>>>(cuts, n_chunks, start, end, out_off, n, out_cap, status);
  HMSE_LAUNCH_CHECK();
  const uint64_t blocks = (n + LINES_NT / 64 - 1) / (LINES_NT / 64);
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  lines_gather_kernel<<<dim3((uint32_t)blocks), dim3(LINES_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, start, end, out_off, n, out, status);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
