// approx.hip — approximate search over the decoded records of a store: where does something within k edits of this byte string END?
// (hmse_amd/find.py StoreFinder.find_approx; include/hmse.h hmse_approx_*.)  Myers' bit-vector algorithm: one 64-bit column per
// pattern, a fixed number of integer operations per byte, the same trip count in every lane.
//
// Replaces the detour read_store -> host -> a dynamic programme over every duplicate chunk.  As for the literal and the regex search a
// record is looked at once and hmse_find_place (place_kernel<8>, chunkmap.h) lays its hits out at every chunk that maps to it; the split
// is by END (include/hmse.h has the definitions and the window argument it rests on):
//   (1) approx_scan_kernel  — per workgroup the match masks Peq[byte][pattern] go to LDS once; per tile of AX_TILE bytes (+ AX_FRONT in
//                             front) every raw byte is read from HBM once, in 16-byte pieces, folded on the way in.  Every lane owns a
//                             strip of AX_STRIP bytes, starts every column fresh W_max - 1 bytes (rounded up to a dword) in front of
//                             it and runs the same number of steps.  Only SCAN ends are answered: p + 1 - raw_off[r] >= W_j.  A
//                             counting walk, ONE reservation per workgroup and tile, and a writing walk only if the tile has hits;
//   (2) approx_seams_kernel — the first W_j - 1 ends of every chunk, walked through the chunk map from W_j bytes in front;
//   (3) approx_spans_kernel — per hit the start of its shortest best match: the anchored column of the reversed pattern, backwards.
// No kernel holds an atomic, a barrier or a cross-lane operation inside a loop that lanes leave at different times (tools/isa_audit.py).
//
// The tile in LDS: logical dword d lies at physical dword d + (d >> 4) — one dword of padding per 16.  The strips are 16 dwords apart, so
// at every step the lanes of a wavefront read physical dwords 17 apart: an odd stride, 32 distinct banks per 32 lanes.
#include "common.h"
#include "chunkmap.h"

constexpr int AX_NT = 256;                            // threads per workgroup
constexpr int AX_STRIP = 64;                          // S: bytes per lane and tile
constexpr int AX_TILE = AX_NT * AX_STRIP;             // T: 16 KiB of records per workgroup and trip
constexpr int AX_FRONT = 80;                          // staged in front of the tile: W_max - 1 <= 79 bytes, rounded to a piece
constexpr int AX_PIECES = (AX_TILE + AX_FRONT) / 16;  // 16-byte pieces per tile
constexpr int AX_DWORDS = (AX_TILE + AX_FRONT) / 4;
constexpr int AX_LDS_DWORDS = AX_DWORDS + (AX_DWORDS >> 4) + 1;
constexpr int AX_P = HMSE_APPROX_MAX_PATTERNS;
constexpr uint32_t AX_MAX_BLOCKS = 512;               // 256 CUs x 2 workgroups; the tiles beyond are reached by the grid stride

// The patterns of a launch, handed to the kernels by value.  Entries j >= n: m = 1, k = 0 and an empty mask — a column that never hits.
struct AxPats { uint32_t n, wmax, ic; uint32_t off[AX_P + 1], m[AX_P], k[AX_P]; };

// One column step of Myers' algorithm (Hyyro's form): Eq = the match mask of the text byte, Pv / Mv the vertical +1 / -1 deltas, sc the
// column's last value D[m], topsh = m - 1 (never 64: m = 64 uses bit 63 and drops the carry of the add).  ANCH = 0: D[0][t] = 0, a match
// may start anywhere; ANCH = 1: D[0][t] = t, it starts at the walk's first byte.  Bits at and above m are never read.
template <int ANCH>
__device__ __forceinline__ void ax_step(unsigned long long Eq, unsigned long long& Pv, unsigned long long& Mv, uint32_t& sc, uint32_t topsh) {
  const unsigned long long Xv = Eq | Mv;
  const unsigned long long Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  unsigned long long Ph = Mv | ~(Xh | Pv);
  unsigned long long Mh = Pv & Xh;
  sc += (uint32_t)((Ph >> topsh) & 1ull) - (uint32_t)((Mh >> topsh) & 1ull);
  Ph = (Ph << 1) | (unsigned long long)ANCH;
  Mh <<= 1;
  Pv = Mh | ~(Xv | Ph);
  Mv = Ph & Xv;
}

// The match masks: s_peq[b * STRIDE + j] has bit i set iff fold(pat_j[i]) == b (REV: pat_j read backwards).  Thread t serves byte value
// t, in loops of uniform length.  With ignore_case the text is folded before it is looked up, so the rows of A-Z stay unused.
template <int STRIDE, bool REV>
__device__ __forceinline__ void ax_build_peq(const uint8_t* __restrict__ pat, const AxPats& P, unsigned long long* s_peq) {
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < STRIDE; j++) {
    unsigned long long mask = 0;
    if ((uint32_t)j < P.n) {
      const uint32_t o = P.off[j], m = P.m[j];
      for (uint32_t i = 0; i < m; i++) {
        uint32_t b = pat[o + (REV ? m - 1 - i : i)];
        if (P.ic) b = fold_byte(b);
        if (b == t) mask |= 1ull << i;
      }
    }
    s_peq[t * STRIDE + j] = mask;
  }
}

// x - g0 as a tile-relative position, saturated far outside every tile
__device__ __forceinline__ int32_t ax_rel(uint64_t x, uint64_t g0) {
  const int64_t d = (int64_t)(x - g0);
  return d < -(1 << 30) ? -(1 << 30) : (d > (1 << 30) ? (1 << 30) : (int32_t)d);
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------
// One lane's walk over a tile: pre_dw dwords of warm-up in front of its strip, then the strip's AX_STRIP bytes — the same trip count in
// every lane.  (r, rs, re): the record of the strip's first byte and its bounds relative to the tile; r moves forward with the walk.
// WRITE = false counts (and adds mult[r] per hit to cnt[j]); WRITE = true writes the hits from index wr on.  -> the lane's hits.
template <int NP, bool WRITE>
__device__ __forceinline__ uint32_t ax_walk(const uint32_t* s_tile, const unsigned long long* s_peq, const AxPats& P, uint32_t pre_dw,
                                            const uint64_t* __restrict__ raw_off, uint64_t n_rec, const uint32_t* __restrict__ mult,
                                            uint64_t g0, uint64_t r, int32_t rs, int32_t re, uint64_t* cnt,
                                            unsigned long long* __restrict__ hits, uint64_t wr, uint64_t hits_cap) {
  unsigned long long Pv[NP], Mv[NP];
  uint32_t sc[NP];
#pragma unroll
  for (int j = 0; j < NP; j++) { Pv[j] = ~0ull; Mv[j] = 0; sc[j] = P.m[j]; }
  uint32_t ld = AX_FRONT / 4 + threadIdx.x * (AX_STRIP / 4) - pre_dw;      // logical dword of the walk's first byte
  for (uint32_t i = 0; i < pre_dw; i++, ld++) {
    const uint32_t w = s_tile[ld + (ld >> 4)];
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const uint32_t c = (w >> (8 * b)) & 0xFFu;
#pragma unroll
      for (int j = 0; j < NP; j++) ax_step<0>(s_peq[c * NP + j], Pv[j], Mv[j], sc[j], P.m[j] - 1);
    }
  }
  int32_t rel = (int32_t)(threadIdx.x * AX_STRIP);
  uint32_t n = 0;
  for (int i = 0; i < AX_STRIP / 4; i++, ld++) {
    const uint32_t w = s_tile[ld + (ld >> 4)];
#pragma unroll
    for (int b = 0; b < 4; b++, rel++) {
      const uint32_t c = (w >> (8 * b)) & 0xFFu;
      while (rel >= re && r + 1 < n_rec) { r++; rs = re; re = ax_rel(raw_off[r + 1], g0); }   // (empty records: more than one trip)
      const uint32_t avail = (rel >= rs && rel < re) ? (uint32_t)(rel + 1 - rs) : 0u;          // bytes of record r up to this end
#pragma unroll
      for (int j = 0; j < NP; j++) {
        ax_step<0>(s_peq[c * NP + j], Pv[j], Mv[j], sc[j], P.m[j] - 1);
        if (sc[j] <= P.k[j] && avail >= P.m[j] + P.k[j]) {                                     // a scan end
          if (WRITE) {
            if (wr < hits_cap) hits[wr] = ((g0 + (uint64_t)rel) << 8) | (sc[j] << 3) | (uint32_t)j;
            wr++;
          } else {
            cnt[j] += mult ? mult[r] : 1u;
          }
          n++;
        }
      }
    }
  }
  return n;
}

template <int NP>
__global__ __launch_bounds__(AX_NT) void approx_scan_kernel(const uint8_t* __restrict__ raw, uint64_t raw_bytes, const uint64_t* __restrict__ raw_off,
                                                            uint64_t n_rec, const uint32_t* __restrict__ mult, const uint8_t* __restrict__ pat,
                                                            AxPats P, unsigned long long* __restrict__ hits, uint64_t hits_cap,
                                                            unsigned long long* n_hits, unsigned long long* counts, uint32_t* status,
                                                            uint64_t n_tiles) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_peq[256 * NP];
  __shared__ uint32_t s_tile[AX_LDS_DWORDS];
  __shared__ uint32_t s_red[AX_NT / 64 + 1];
  __shared__ uint64_t s_red64[AX_NT / 64 + 1];
  __shared__ unsigned long long s_base;
  __shared__ uint64_t s_rec[2];                       // the records of the tile's first and last byte

  if (*status & 2u) return;                           // inconsistent tables (tables_validate_kernel)
  const uint32_t t = threadIdx.x;
  ax_build_peq<NP, false>(pat, P, s_peq);
  __syncthreads();
  const uint32_t pre_dw = (P.wmax + 2) / 4;           // W_max - 1 bytes of warm-up, rounded up to a dword: at most AX_FRONT / 4
  const uint64_t lo = raw_off[0], hi = raw_off[n_rec];               // the records cover [lo, hi) of raw
  uint64_t cnt[NP];
#pragma unroll
  for (int j = 0; j < NP; j++) cnt[j] = 0;

  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t g0 = tile * (uint64_t)AX_TILE;
    if (t < 2) {
      // the tile's first and last byte, both clamped to [lo, hi]: s_rec[0] <= s_rec[1] also for a tile that lies wholly in front of the
      // records (junk in front of raw_off[0], leading empty records) or behind them — last_le wants a range that does not descend
      const uint64_t x = t == 0 ? g0 : g0 + AX_TILE - 1;
      s_rec[t] = last_le(raw_off, 0, n_rec, x < lo ? lo : (x > hi ? hi : x));
    }
    // ---- stage: piece q = the 16 bytes from raw[g0 - AX_FRONT + 16 q] on (0 outside raw), folded, into the padded layout ----
#pragma unroll
    for (int jj = 0; jj < (AX_PIECES + AX_NT - 1) / AX_NT; jj++) {
      const uint32_t q = t + jj * AX_NT;
      if (q < AX_PIECES) {
        const uint64_t gq = g0 + 16ull * q;           // the piece's first byte + AX_FRONT
        uint32_t w[4] = {0, 0, 0, 0};
        if (gq >= AX_FRONT && gq - AX_FRONT + 16 <= raw_bytes) {
          const uint4 v = load_u4_unaligned(raw + (gq - AX_FRONT));
          w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
          for (int i = 0; i < 16; i++) {
            const uint64_t pos = gq + i;
            const uint32_t b = (pos >= AX_FRONT && pos - AX_FRONT < raw_bytes) ? raw[pos - AX_FRONT] : 0u;
            w[i >> 2] |= b << (8 * (i & 3));
          }
        }
        const uint32_t pd = 4u * q + (q >> 2);        // the piece's four dwords share one group of 16
#pragma unroll
        for (int i = 0; i < 4; i++) s_tile[pd + i] = P.ic ? fold_dword(w[i]) : w[i];
      }
    }
    __syncthreads();                                  // s_tile and s_rec are complete

    // ---- the record of the strip's first byte (of the first record behind it, if it lies in front of lo) ----
    const uint64_t r = last_le(raw_off, s_rec[0], s_rec[1] + 1, g0 + (uint64_t)t * AX_STRIP);
    const int32_t rs = ax_rel(raw_off[r], g0), re = ax_rel(raw_off[r + 1], g0);

    // ---- count, reserve once per workgroup and tile, and walk again to write only if the tile has hits ----
    const uint32_t n = ax_walk<NP, false>(s_tile, s_peq, P, pre_dw, raw_off, n_rec, mult, g0, r, rs, re, cnt, hits, 0, 0);
    uint32_t total;
    const uint32_t my = block_exclusive_scan<AX_NT>(n, s_red, &total);
    total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
    if (total) {
      if (t == 0) {
        const unsigned long long base = atomicAdd(n_hits, (unsigned long long)total);
        if (hits_cap && base + total > hits_cap) atomicOr(status, 1u);
        s_base = base;
      }
      if (hits_cap) {
        __syncthreads();
        ax_walk<NP, true>(s_tile, s_peq, P, pre_dw, raw_off, n_rec, mult, g0, r, rs, re, cnt, hits, s_base + my, hits_cap);
      }
    }
    __syncthreads();                                  // the next tile overwrites s_tile, s_rec and s_base
  }
#pragma unroll
  for (int j = 0; j < NP; j++) {
    uint64_t tot;
    block_exclusive_scan<AX_NT>(cnt[j], s_red64, &tot);
    if (t == 0 && (uint32_t)j < P.n && tot) atomicAdd(&counts[j], (unsigned long long)tot);
  }
}

// ---- seams --------------------------------------------------------------------------------------------------------------------
// The seam ends of chunk [c0, c1) for pattern j: the bytes q = s0 .. e1 - 1 through the chunk map (kc: the chunk of s0), at most 2 W - 2
// of them; the ends q + 1 with q >= c0 are reported.  -> the hits.
template <bool WRITE>
__device__ __forceinline__ uint32_t ax_seam_walk(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                 const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                 const unsigned long long* s_peq, uint32_t j, uint32_t ic, uint32_t m, uint32_t k, uint64_t s0,
                                                 uint64_t c0, uint64_t e1, uint64_t kc, unsigned long long* __restrict__ hits, uint64_t wr,
                                                 uint64_t hits_cap) {
  unsigned long long Pv = ~0ull, Mv = 0;
  uint32_t sc = m, n = 0;
  for (uint64_t q = s0; q < e1; q++) {                // q < e1 <= cuts[c + 1] <= N
    uint32_t b = corpus_byte(raw, raw_off, cuts, slot, q, kc);
    if (ic) b = fold_byte(b);
    ax_step<0>(s_peq[b * AX_P + j], Pv, Mv, sc, m - 1);
    if (q >= c0 && sc <= k) {
      if (WRITE) {
        if (wr < hits_cap) hits[wr] = (q << 8) | (sc << 3) | j;
        wr++;
      }
      n++;
    }
  }
  return n;
}

// One thread per (chunk, pattern slot j = t & 7); lanes of slots j >= n_pat and of patterns with W = 1 idle.
__global__ __launch_bounds__(AX_NT) void approx_seams_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                             const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                             uint64_t n_chunks, const uint8_t* __restrict__ pat, AxPats P,
                                                             unsigned long long* __restrict__ hits, uint64_t hits_cap, unsigned long long* n_hits,
                                                             unsigned long long* counts, uint32_t* status, uint64_t n_ids) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_peq[256 * AX_P];
  __shared__ uint32_t s_m[AX_P], s_k[AX_P];
  __shared__ uint32_t s_red[AX_NT / 64 + 1];
  __shared__ unsigned long long s_base;
  __shared__ unsigned long long s_cnt[AX_P];
  if (*status & 2u) return;
  const uint32_t t = threadIdx.x;
  ax_build_peq<AX_P, false>(pat, P, s_peq);
#pragma unroll
  for (int j = 0; j < AX_P; j++)
    if (t == (uint32_t)j) { s_m[j] = P.m[j]; s_k[j] = P.k[j]; s_cnt[j] = 0; }
  __syncthreads();
  const uint32_t j = t & (AX_P - 1);
  const uint32_t m = s_m[j], k = s_k[j], W = m + k;
  const bool live = j < P.n && W >= 2;                // W = 1: every end is a scan end
  const uint64_t first = cuts[0];
  unsigned long long mine = 0;
  for (uint64_t id0 = (uint64_t)blockIdx.x * AX_NT; id0 < n_ids; id0 += (uint64_t)gridDim.x * AX_NT) {
    const uint64_t c = (id0 + t) / AX_P;
    uint64_t s0 = 0, c0 = 0, e1 = 0, kc = 0;
    bool work = live && c < n_chunks;
    if (work) {
      c0 = cuts[c];
      const uint64_t c1 = cuts[c + 1];
      work = c1 > c0;
      if (work) {
        e1 = c1 - c0 < W ? c1 : c0 + W - 1;           // the ends c0 + 1 .. e1: e - c0 < W
        s0 = c0 + 1 >= first + W ? c0 + 1 - W : first;                 // a fresh column W bytes in front of the first end, or at the corpus's start
        kc = last_le(cuts, 0, c + 1, s0);
      }
    }
    const uint32_t n = work ? ax_seam_walk<false>(raw, raw_off, cuts, slot, s_peq, j, P.ic, m, k, s0, c0, e1, kc, hits, 0, 0) : 0u;
    uint32_t total;
    const uint32_t my = block_exclusive_scan<AX_NT>(n, s_red, &total);
    total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
    if (total) {
      if (t == 0) {
        const unsigned long long base = atomicAdd(n_hits, (unsigned long long)total);
        if (hits_cap && base + total > hits_cap) atomicOr(status, 1u);
        s_base = base;
      }
      if (hits_cap) {
        __syncthreads();
        if (n) ax_seam_walk<true>(raw, raw_off, cuts, slot, s_peq, j, P.ic, m, k, s0, c0, e1, kc, hits, s_base + my, hits_cap);
      }
    }
    __syncthreads();                                  // the next trip overwrites s_base
    mine += n;
  }
  atomicAdd(&s_cnt[j], mine);                         // every thread, once, behind the loop
  __syncthreads();
  if (t < P.n && s_cnt[t]) atomicAdd(&counts[t], s_cnt[t]);
}

// ---- spans --------------------------------------------------------------------------------------------------------------------
// One lane per hit (corpus offset o of the match's last byte, errors d, pattern j): the anchored column of the REVERSED pattern over
// C[o], C[o - 1], ... for at most m_j + d bytes (a match of d errors is no longer) and not beyond the corpus's first byte; the first step
// at which the column's last value equals d is the shortest best match's start.
__global__ __launch_bounds__(AX_NT) void approx_spans_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                             const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                             uint64_t n_chunks, const uint8_t* __restrict__ pat, AxPats P,
                                                             const unsigned long long* __restrict__ hits, uint64_t n,
                                                             unsigned long long* __restrict__ start, uint32_t* status) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_peq[256 * AX_P];
  __shared__ uint32_t s_m[AX_P];
  if (*status & 2u) return;
  const uint32_t t = threadIdx.x;
  ax_build_peq<AX_P, true>(pat, P, s_peq);
#pragma unroll
  for (int j = 0; j < AX_P; j++)
    if (t == (uint32_t)j) s_m[j] = P.m[j];
  __syncthreads();
  const uint64_t first = n_chunks ? cuts[0] : 0, N = n_chunks ? cuts[n_chunks] : 0;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * AX_NT + t; i < n; i += (uint64_t)gridDim.x * AX_NT) {
    const unsigned long long h = hits[i];
    const uint64_t o = h >> 8;
    const uint32_t d = (uint32_t)(h >> 3) & 31u, j = (uint32_t)h & 7u;
    uint64_t st = o + 1;                              // an empty span: the answer for a hit that cannot be
    bool ok = false;
    if (o >= first && o < N && j < P.n) {
      const uint32_t m = s_m[j];
      uint64_t steps = m + d;
      if (steps > o - first + 1) steps = o - first + 1;
      uint64_t kc = last_le(cuts, 0, n_chunks, o);
      unsigned long long Pv = ~0ull, Mv = 0;
      uint32_t sc = m;
      for (uint64_t s = 0; s < steps; s++) {
        const uint64_t q = o - s;
        while (q < cuts[kc]) kc--;                    // q >= cuts[0]: kc stays at or above 0
        uint32_t b = raw[raw_off[slot[kc]] + (q - cuts[kc])];
        if (P.ic) b = fold_byte(b);
        ax_step<1>(s_peq[b * AX_P + j], Pv, Mv, sc, m - 1);
        if (sc == d) { st = q; ok = true; break; }
      }
    }
    start[i] = st;
    bad |= !ok;
  }
  if (bad) atomicOr(status, 1u);
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
// k == nullptr (hmse_approx_spans): no bounds are given, the hits carry their errors.
static int approx_patterns(const uint32_t* pat_off, const uint8_t* k, bool with_k, uint32_t n_pat, uint32_t flags, AxPats* P) {
  if (!pat_off || (with_k && !k) || n_pat == 0 || n_pat > HMSE_APPROX_MAX_PATTERNS || (flags & ~HMSE_FIND_IGNORE_CASE)) return HMSE_EINVAL;
  P->n = n_pat;
  P->wmax = 1;
  P->ic = (flags & HMSE_FIND_IGNORE_CASE) ? 1u : 0u;
  for (uint32_t j = 0; j <= AX_P; j++) P->off[j] = pat_off[j < n_pat ? j : n_pat];
  for (uint32_t j = 0; j < AX_P; j++) { P->m[j] = 1; P->k[j] = 0; }
  for (uint32_t j = 0; j < n_pat; j++) {
    if (pat_off[j + 1] <= pat_off[j] || pat_off[j + 1] - pat_off[j] > HMSE_APPROX_MAX_LEN) return HMSE_EINVAL;
    const uint32_t m = pat_off[j + 1] - pat_off[j], kj = with_k ? k[j] : 0;
    if (kj > HMSE_APPROX_MAX_K || kj >= m) return HMSE_EINVAL;
    P->m[j] = m;
    P->k[j] = kj;
    if (m + kj > P->wmax) P->wmax = m + kj;
  }
  return HMSE_OK;
}

static int approx_validate(const uint64_t* raw_off, uint64_t n_rec, uint64_t raw_bytes, const uint64_t* cuts, const uint64_t* slot,
                           uint64_t n_chunks, uint32_t* status, hipStream_t stream) {
  return tables_validate<AX_NT>(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, nullptr, status, AX_MAX_BLOCKS, stream);
}

extern "C" int hmse_approx_scan(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint32_t* mult,
                                const uint8_t* pat, const uint32_t* pat_off, const uint8_t* k, uint32_t n_pat, uint32_t flags,
                                uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits, uint64_t* counts, uint32_t* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AxPats P;
  if (approx_patterns(pat_off, k, true, n_pat, flags, &P) != HMSE_OK || !pat || !n_hits || !counts || !status) return HMSE_EINVAL;
  if (n_rec && (!raw_off || (raw_bytes && !raw))) return HMSE_EINVAL;
  if (raw_bytes >= (1ull << 56)) return HMSE_EINVAL;  // a hit is position << 8 | errors << 3 | pattern
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(n_hits, 0, 8, stream);
  HMSE_FILL(counts, 0, 8 * (size_t)n_pat, stream);
  if (n_rec == 0 || raw_bytes == 0) return HMSE_OK;
  if (!hits) hits_cap = 0;
  int rc = approx_validate(raw_off, n_rec, raw_bytes, nullptr, nullptr, 0, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t n_tiles = (raw_bytes + AX_TILE - 1) / AX_TILE;
  const dim3 grid((uint32_t)(n_tiles < AX_MAX_BLOCKS ? n_tiles : AX_MAX_BLOCKS)), block(AX_NT);
  unsigned long long *h = (unsigned long long*)hits, *nh = (unsigned long long*)n_hits, *cn = (unsigned long long*)counts;
  PROF_BEGIN(HMSE_STAGE_FIND_SCAN, stream);
#define HMSE_APPROX_SCAN(NP) approx_scan_kernel<NP><<<grid, block, 0, stream>>>(raw, raw_bytes, raw_off, n_rec, mult, pat, P, h, hits_cap, nh, cn, status, n_tiles)
  if (n_pat == 1) HMSE_APPROX_SCAN(1);
  else if (n_pat == 2) HMSE_APPROX_SCAN(2);
  else if (n_pat <= 4) HMSE_APPROX_SCAN(4);
  else HMSE_APPROX_SCAN(8);
#undef HMSE_APPROX_SCAN
  PROF_END(HMSE_STAGE_FIND_SCAN, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_approx_seams(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                                 const uint64_t* slot, uint64_t n_chunks, const uint8_t* pat, const uint32_t* pat_off, const uint8_t* k,
                                 uint32_t n_pat, uint32_t flags, uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits, uint64_t* counts,
                                 uint32_t* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AxPats P;
  if (approx_patterns(pat_off, k, true, n_pat, flags, &P) != HMSE_OK || !pat || !n_hits || !counts || !status) return HMSE_EINVAL;
  if (n_chunks && (!cuts || !slot || !raw_off || !raw)) return HMSE_EINVAL;
  if (n_chunks > (1ull << 40) || raw_bytes >= (1ull << 56)) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(n_hits, 0, 8, stream);
  HMSE_FILL(counts, 0, 8 * (size_t)n_pat, stream);
  if (n_chunks == 0) return HMSE_OK;
  if (!hits) hits_cap = 0;
  int rc = approx_validate(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, status, stream);
  if (rc != HMSE_OK) return rc;
  if (P.wmax < 2) return HMSE_OK;                     // W = 1 for every pattern: every end is a scan end
  const uint64_t n_ids = n_chunks * (uint64_t)AX_P;
  uint64_t nb = (n_ids + AX_NT - 1) / AX_NT;
  if (nb > AX_MAX_BLOCKS) nb = AX_MAX_BLOCKS;         // (the masks are built once per workgroup; the rest by the grid stride)
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  approx_seams_kernel<<<dim3((uint32_t)nb), dim3(AX_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, pat, P, (unsigned long long*)hits, hits_cap,
                                                                      (unsigned long long*)n_hits, (unsigned long long*)counts, status, n_ids);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_approx_spans(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                                 const uint64_t* slot, uint64_t n_chunks, const uint8_t* pat, const uint32_t* pat_off, uint32_t n_pat,
                                 uint32_t flags, const uint64_t* hits, uint64_t n, uint64_t* start, uint32_t* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AxPats P;
  if (approx_patterns(pat_off, nullptr, false, n_pat, flags, &P) != HMSE_OK || !pat || !status) return HMSE_EINVAL;
  if (n && (!hits || !start)) return HMSE_EINVAL;
  if (n_chunks && (!cuts || !slot || !raw_off || !raw)) return HMSE_EINVAL;
  if (n >= (1ull << 33) || n_chunks > (1ull << 40) || raw_bytes >= (1ull << 56)) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n == 0) return HMSE_OK;
  int rc = approx_validate(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, status, stream);
  if (rc != HMSE_OK) return rc;
  uint64_t nb = (n + AX_NT - 1) / AX_NT;
  if (nb > AX_MAX_BLOCKS) nb = AX_MAX_BLOCKS;
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  approx_spans_kernel<<<dim3((uint32_t)nb), dim3(AX_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, pat, P, (const unsigned long long*)hits, n,
                                                                      (unsigned long long*)start, status);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
