// subst.hip — the corpus with a list of ranges replaced, written on the device (hmse_amd/find.py substitute / redact;
// include/hmse_subst.h hmse_subst_apply; a library of its own, libhmse_subst.so, beside libhmse_hip.so).
//
// find_regex / nonoverlapping say where something occurs; `sed 's/RX/repl/g'` and taking secrets out of a corpus before it is ingested
// again need the splice: O = C[0:start[0]) R_0 C[end[0]:start[1]) R_1 ... C[end[n-1]:N).  The header turns that into a rule per OUTPUT
// position p: the last edit i with out_off[i] <= p either covers p with its replacement, or p lies in the kept gap behind it and is the
// corpus byte p - D.  So the kernels are:
//   (1) subst_edits_kernel — one thread per edit and per replacement: the edit rule, sel, rep_off, and that the caller's out_off IS the
//       definition's (a recurrence between neighbours: out_off[i+1] - out_off[i] = |R_i| + start[i+1] - end[i]).  Any breach is status
//       bit 1; thread 0 sets bit 0 for an output that does not fit.
//   (2) subst_apply_kernel — one workgroup per tile of the output; it leaves at once when a status bit is set.  A thread owns strips of 16
//       output bytes at 16-byte-aligned ADDRESSES (the tiles count from out's address rounded down, so the first and the last strip
//       may be partial).  A strip that lies in one kept gap and in one chunk is one unaligned 16-byte load and one aligned 16-byte
//       store; any other is assembled byte by byte in two registers and stored once (a partial one bytewise).
// Both lookups (the edit at p in out_off, the chunk at p - D in cuts) are narrowed per tile first: wavefront 0 finds the edits of the
// tile's first and last byte and the chunks of the first and last corpus byte the tile can read, 64 probes a trip (wave_last_le: the
// loop and its ballot are wave-uniform), and leaves the four bounds in LDS; a strip then searches only between them, which for most
// tiles is no search at all.  Equal out_off values (deletions in a row, insertions at one place) are stepped over by the same search:
// the last of them is the right one.  No workspace, no atomics in the writing kernel.
#include "common.h"
#include "../../include/hmse_subst.h"
#include "chunkmap.h"

constexpr int SUBST_NT = 256;                // threads of a workgroup
constexpr int SUBST_TRIPS = 4;               // strips a thread owns
constexpr int SUBST_STRIP = 16;              // bytes of a strip: one aligned 16-byte store
constexpr int SUBST_TILE = SUBST_NT * SUBST_STRIP * SUBST_TRIPS;   // output bytes of a workgroup

// ---- edits --------------------------------------------------------------------------------------------------------------------
// |R_i| of an edit whose sel is below n_rep
__device__ __forceinline__ uint64_t subst_rep_len(const uint64_t* __restrict__ start, const uint64_t* __restrict__ end,
                                                  const uint64_t* __restrict__ sel, const uint64_t* __restrict__ rep_off, uint32_t fill, uint64_t i) {
  if (fill) return end[i] - start[i];
  const uint64_t r = sel[i];
  return rep_off[r + 1] - rep_off[r];
}

// Thread i proves edit i and replacement i; the grid covers max(n, n_rep, 1).  Reads cuts only when the tables are consistent.
template <int NT>
__global__ __launch_bounds__(NT) void subst_edits_kernel(const uint64_t* __restrict__ cuts, uint64_t n_chunks, const uint64_t* __restrict__ start,
                                                         const uint64_t* __restrict__ end, const uint64_t* __restrict__ sel, uint64_t n,
                                                         uint64_t rep_bytes, const uint64_t* __restrict__ rep_off, uint64_t n_rep, uint32_t fill,
                                                         const uint64_t* __restrict__ out_off, uint64_t out_cap, uint32_t* status) {
  if (*status & 2u) return;
  const uint64_t N = n_chunks ? cuts[n_chunks] : 0;
  const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const uint64_t s = start[i], e = end[i], prev = i ? end[i - 1] : 0, r = sel[i];
    bad |= prev > s || s > e || e > N || r >= n_rep;
    if (r < n_rep) {
      const uint64_t rlen = fill ? e - s : rep_off[r + 1] - rep_off[r];
      const uint64_t next = i + 1 < n ? start[i + 1] : N, a = out_off[i], b = out_off[i + 1];
      bad |= b < a || b - a != rlen + (next - e);      // (a next in front of e is the next thread's finding, or e > N)
    }
    if (i == 0) bad |= out_off[0] != s;
  }
  if (i < n_rep) {
    const uint64_t a = rep_off[i], b = rep_off[i + 1];
    bad |= a > b || (fill && b - a != 1);
    if (i == 0) bad |= a != 0 || rep_off[n_rep] > rep_bytes;
  }
  if (i == 0) {
    if (n == 0) bad |= out_off[0] != N;
    if (out_off[n] > out_cap) atomicOr(status, 1u);
  }
  if (bad) atomicOr(status, 2u);
}

// ---- apply --------------------------------------------------------------------------------------------------------------------
// last_le (chunkmap.h) by a whole wavefront, 64 probes a trip: the answer in every lane.  a, b and x are the same in every lane, so
// the loop, its exit and the ballot are wave-uniform.
__device__ __forceinline__ uint64_t wave_last_le(const uint64_t* __restrict__ arr, uint64_t a, uint64_t b, uint64_t x, uint32_t lane) {
  while (b - a > 1) {
    const uint64_t step = (b - a + 63) >> 6, at = a + 1 + (uint64_t)lane * step;
    const bool le = at < b && arr[at] <= x;
    const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(le));       // arr ascends: the lanes that hold are the first cnt
    if (cnt == 0) break;
    a += 1 + (uint64_t)(cnt - 1) * step;
    const uint64_t nb = a + step;                      // the first probe that did not hold (or lay outside)
    b = nb < b ? nb : b;
  }
  return a;
}

__device__ __forceinline__ void subst_put(uint64_t& lo, uint64_t& hi, uint32_t j, uint32_t byte) {
  if (j < 8) lo |= (uint64_t)byte << (8 * j);
  else hi |= (uint64_t)byte << (8 * (j - 8));
}

template <int NT, int TRIPS, bool FILL>
__global__ __launch_bounds__(NT) void subst_apply_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                         const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot, uint64_t n_chunks,
                                                         const uint64_t* __restrict__ start, const uint64_t* __restrict__ end,
                                                         const uint64_t* __restrict__ sel, uint64_t n, const uint8_t* __restrict__ rep,
                                                         const uint64_t* __restrict__ rep_off, const uint64_t* __restrict__ out_off,
                                                         uint8_t* __restrict__ out, const uint32_t* status) {
  __shared__ uint64_t bounds[4];                       // the tile's first and last edit, first and last chunk
  if (*status) return;                                 // a refused call writes nothing (tables_validate_kernel, subst_edits_kernel)
  constexpr uint64_t TILE = (uint64_t)NT * SUBST_STRIP * TRIPS;
  const uint64_t lead = (uint64_t)(uintptr_t)out & (SUBST_STRIP - 1);        // strips are aligned ADDRESSES: position p lies at v = p + lead
  const uint64_t total = out_off[n], N = n_chunks ? cuts[n_chunks] : 0;
  const uint64_t v0 = (uint64_t)blockIdx.x * TILE;
  if (total == 0 || v0 >= total + lead) return;
  const uint64_t t0 = v0 > lead ? v0 - lead : 0;                             // the tile's output positions [t0, t1), not empty
  const uint64_t t1 = (v0 + TILE < total + lead ? v0 + TILE : total + lead) - lead;
  if (threadIdx.x < 64) {
    const uint32_t lane = threadIdx.x;
    uint64_t e_lo = 0, e_hi = 0, q_lo = t0, q_end = t1;                      // with no edit at or in front: the corpus as it is
    if (n) {
      e_lo = wave_last_le(out_off, 0, n, t0, lane);
      e_hi = wave_last_le(out_off, e_lo, n, t1 - 1, lane);
      const uint64_t a = out_off[e_lo], b = out_off[e_hi];
      if (a <= t0) {                                   // t0 lies in R or in the gap behind it
        const uint64_t r_end = a + subst_rep_len(start, end, sel, rep_off, FILL, e_lo);
        q_lo = end[e_lo] + (t0 > r_end ? t0 - r_end : 0);
      }
      if (b <= t1 - 1) {
        const uint64_t r_end = b + subst_rep_len(start, end, sel, rep_off, FILL, e_hi);
        q_end = end[e_hi] + (t1 > r_end ? t1 - r_end : 0);
      }
    }
    uint64_t k_lo = 0, k_hi = 0;
    if (n_chunks) {
      k_lo = wave_last_le(cuts, 0, n_chunks, q_lo, lane);
      k_hi = wave_last_le(cuts, k_lo, n_chunks, q_end > q_lo ? q_end - 1 : q_lo, lane);
    }
    if (lane == 0) { bounds[0] = e_lo; bounds[1] = e_hi; bounds[2] = k_lo; bounds[3] = k_hi; }
  }
  __syncthreads();
  const uint64_t e_lo = bounds[0], e_hi = bounds[1], k_lo = bounds[2], k_hi = bounds[3];

#pragma unroll 1
  for (int trip = 0; trip < TRIPS; trip++) {
    const uint64_t v = v0 + ((uint64_t)trip * NT + threadIdx.x) * SUBST_STRIP;
    if (v >= total + lead) break;
    const uint64_t p0 = v > lead ? v - lead : 0;
    const uint64_t p1 = (v + SUBST_STRIP < total + lead ? v + SUBST_STRIP : total + lead) - lead;
    const bool whole = p1 - p0 == SUBST_STRIP;
    uint64_t i = 0, cur = p0, lo = 0, hi = 0;
    bool have = false;                                 // i is the last edit with out_off[i] <= cur; without, edit 0 is the next one
    if (n) {
      i = last_le(out_off, e_lo, e_hi + 1, p0);
      have = out_off[i] <= p0;
    }
    bool stored = false;
    while (cur < p1) {
      if (have) {
        const uint64_t at = out_off[i], r_end = at + subst_rep_len(start, end, sel, rep_off, FILL, i);
        if (cur < r_end) {                             // bytes of R_i
          const uint64_t stop = r_end < p1 ? r_end : p1;
          const uint8_t* src = rep + rep_off[sel[i]] + (FILL ? 0 : cur - at);
          for (uint64_t j = 0; j < stop - cur; j++) subst_put(lo, hi, (uint32_t)(cur - p0 + j), src[FILL ? 0 : j]);
          cur = stop;
          continue;
        }
      }
      const uint64_t nx = have ? i + 1 : 0;            // the kept gap in front of edit nx (behind the last edit: up to the end)
      const uint64_t gap_end = nx < n ? out_off[nx] : total;
      if (gap_end <= cur) {                            // nothing of it is left: on to the last edit that begins at or in front of cur
        i = last_le(out_off, nx, e_hi + 1, cur);
        have = true;
        continue;
      }
      const uint64_t q = cur + (nx < n ? start[nx] : N) - gap_end;           // cur - D
      const uint64_t stop = gap_end < p1 ? gap_end : p1;
      uint64_t k = last_le(cuts, k_lo, k_hi + 1, q);
      if (whole && stop - cur == SUBST_STRIP && q + SUBST_STRIP <= cuts[k + 1]) {      // one gap, one chunk
        *(uint4*)(out + p0) = load_u4_unaligned(raw + raw_off[slot[k]] + (q - cuts[k]));
        stored = true;
        break;
      }
      for (uint64_t j = 0; j < stop - cur; j++) subst_put(lo, hi, (uint32_t)(cur - p0 + j), corpus_byte(raw, raw_off, cuts, slot, q + j, k));
      cur = stop;
    }
    if (stored) continue;
    if (whole) {
      *(uint4*)(out + p0) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    } else {
      for (uint64_t j = 0; j < p1 - p0; j++) out[p0 + j] = (uint8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xFFu);
    }
  }
}

// ---- grids (host) ------------------------------------------------------------------------------------------------------------
// The three grids of one call, each covering its work outright; tools/subst_emu.cpp launches by the same function.  The writing
// kernel's tiles count from out's ADDRESS rounded down to a strip, so its `lead` bytes push the last position on.
struct SubstGrids {
  uint64_t tables, edits, tiles;
};
static inline SubstGrids subst_grids(uint64_t n_rec, uint64_t n_chunks, uint64_t n, uint64_t n_rep, const uint8_t* out, uint64_t out_cap,
                                     uint64_t nt, uint64_t tile) {
  const uint64_t n_tab = n_rec > n_chunks ? n_rec : n_chunks, n_chk = n > n_rep ? n : n_rep;
  const uint64_t lead = (uint64_t)(uintptr_t)out & (SUBST_STRIP - 1);
  SubstGrids g;
  g.tables = n_tab / nt + (n_tab % nt != 0);
  g.edits = n_chk ? n_chk / nt + (n_chk % nt != 0) : 1;  // thread 0 has work with no edit and no replacement
  g.tiles = out_cap / tile + ((out_cap % tile + lead) / tile) + ((out_cap % tile + lead) % tile != 0);     // ceil((out_cap + lead) / tile), no overflow
  return g;
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
// The table rules of chunkmap.h (status bit 1) and cuts[0] != 0, as lines.hip and tally.hip check them: cuts goes in as the chunk_out
// as well.  Every grid of this file covers its work outright; sizes that would need more than 2^31 - 1 workgroups are HMSE_EINVAL.
constexpr uint64_t SUBST_GRID_MAX = 0x7FFFFFFFull;

extern "C" int hmse_subst_apply(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                                const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* sel,
                                uint64_t n, const uint8_t* rep, uint64_t rep_bytes, const uint64_t* rep_off, uint64_t n_rep, uint32_t flags,
                                const uint64_t* out_off, uint8_t* out, uint64_t out_cap, uint32_t* status, void* stream_) {
  if (!status || !out_off || n >= (1ull << 33) || (flags & ~(uint32_t)HMSE_SUBST_FILL) || (n && !n_rep)) return HMSE_EINVAL;
  if ((raw_bytes && !raw) || ((n_rec || n_chunks) && !raw_off) || (n_chunks && (!cuts || !slot))) return HMSE_EINVAL;
  if ((n && (!start || !end || !sel)) || (rep_bytes && !rep) || (n_rep && !rep_off) || (out_cap && !out)) return HMSE_EINVAL;
  const SubstGrids g = subst_grids(n_rec, n_chunks, n, n_rep, out, out_cap, SUBST_NT, SUBST_TILE);
  if (g.tables > SUBST_GRID_MAX || g.edits > SUBST_GRID_MAX || g.tiles > SUBST_GRID_MAX) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  int rc = tables_validate<SUBST_NT>(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, /*chunk_out=*/cuts, status, SUBST_GRID_MAX, stream);
  if (rc != HMSE_OK) return rc;
  subst_edits_kernel<SUBST_NT><<<dim3((uint32_t)g.edits), dim3(SUBST_NT), 0, stream>>>(cuts, n_chunks, start, end, sel, n, rep_bytes, rep_off, n_rep,
                                                                                          flags & HMSE_SUBST_FILL, out_off, out_cap, status);
  HMSE_LAUNCH_CHECK();
  if (out_cap == 0) return HMSE_OK;
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  if (flags & HMSE_SUBST_FILL)
    subst_apply_kernel<SUBST_NT, SUBST_TRIPS, true><<<dim3((uint32_t)g.tiles), dim3(SUBST_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, start, end, sel, n,
                                                                                                           rep, rep_off, out_off, out, status);
  else
    subst_apply_kernel<SUBST_NT, SUBST_TRIPS, false><<<dim3((uint32_t)g.tiles), dim3(SUBST_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, start, end, sel, n,
                                                                                                            rep, rep_off, out_off, out, status);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
