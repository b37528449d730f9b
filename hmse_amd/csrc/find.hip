// find.hip — exact byte-pattern search over the decoded records of a store (hmse_amd/find.py; include/hmse.h hmse_find_*).
//
// Replaces what a user of the reference layout does to answer "where does this byte string occur": read the store back
// (README.md:1621-1675), move it to the host and loop over bytes.find().  A corpus of N bytes holds U <= N unique record bytes, so
//   (1) find_scan_kernel  — HBM-bound scan of the records, each byte read once: one FIND_STRIP-byte strip per lane loaded with 16-byte
//                           loads (plus 4 bytes of the next strip), a 4-byte window per position formed with v_alignbyte, and a cheap
//                           filter that rejects almost every position — few patterns: masked dword compare against every pattern's
//                           head (running minimum, the rare group with a zero is replayed); many patterns: one bit lookup in an 8 KiB
//                           LDS bitmap over the first two bytes of all patterns (cost per position independent of their number).
//                           Survivors are verified byte by byte against the patterns in LDS, clipped to their record (raw_off);
//                           the hits of a tile are emitted after the strip with ONE reservation per workgroup;
//   (2) find_seams_kernel — the strip of max(m) - 1 candidate starts in front of every chunk boundary, read through the chunk map;
//   (3) place_kernel<8>   — the sorted in-record hits laid out at every chunk that maps to their record (chunkmap.h).
// Every call starts with tables_validate_kernel (chunkmap.h): the kernels behind it leave when it set status bit 1.
// No kernel holds an atomic or a cross-lane operation inside a loop that lanes leave at different times (tools/isa_audit.py).
#include "common.h"
#include "chunkmap.h"

constexpr int FIND_NT = 256;                          // threads per workgroup
constexpr int FIND_STRIP = 128;                       // S: bytes per lane
constexpr int FIND_TILE = FIND_NT * FIND_STRIP;       // T: 32 KiB of records per workgroup and trip
constexpr int FIND_WORDS = FIND_STRIP / 32;           // candidate bitmap dwords per lane
constexpr uint32_t FIND_FEW = 4;                      // up to this many patterns: head compare; more: the two-byte bitmap
constexpr uint32_t FIND_MAX_BLOCKS = 2048;            // 256 CUs x 8 workgroups; the tiles beyond are reached by the grid stride
constexpr uint32_t FIND_PAT_BYTES = HMSE_FIND_MAX_PATTERNS * HMSE_FIND_MAX_LEN;

// The patterns' bounds, read on the host during the call and handed to the kernels by value.
struct FindPats { uint32_t n, max_len; uint32_t off[HMSE_FIND_MAX_PATTERNS + 1]; };

template <bool IC>
__device__ __forceinline__ bool find_match(const uint8_t* __restrict__ p, const uint8_t* sp, uint32_t m) {
  for (uint32_t i = 0; i < m; i++) {
    uint32_t b = p[i];
    if (IC) b = fold_byte(b);
    if (b != sp[i]) return false;
  }
  return true;
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------
// (at least 4 waves per SIMD: left alone the head-compare instantiations take 142 VGPRs and run 3; at 128 they neither spill nor use scratch)
template <bool FEW, bool IC>
__global__ __launch_bounds__(FIND_NT) __attribute__((amdgpu_waves_per_eu(4))) void find_scan_kernel(const uint8_t* __restrict__ raw, uint64_t raw_bytes, const uint64_t* __restrict__ raw_off,
                                                            uint64_t n_rec, const uint32_t* __restrict__ mult, const uint8_t* __restrict__ pat,
                                                            FindPats P, unsigned long long* __restrict__ hits, uint64_t hits_cap,
                                                            unsigned long long* n_hits, unsigned long long* counts, uint32_t* status,
                                                            uint64_t n_tiles) {
  __shared__ uint8_t s_pat[FIND_PAT_BYTES];           // the patterns back to back (folded when IC)
  __shared__ uint32_t s_bm[FEW ? 1 : 2048];           // bit (c0 | c1 << 8): some pattern starts with c0 c1 (length 1: with c0)
  __shared__ uint32_t s_head[FIND_FEW], s_mask[FIND_FEW];
  __shared__ uint32_t s_red[FIND_NT / 64 + 1];
  __shared__ unsigned long long s_base;

  if (*status & 2u) return;                           // inconsistent tables (tables_validate_kernel)
  const uint32_t t = threadIdx.x;
  const uint32_t n_pat = P.n;
  const uint32_t o0 = P.off[0];       // (the bounds are read from the kernel arguments where they are used: scalar loads)
  {
    const uint32_t total = P.off[n_pat] - o0;
    for (uint32_t i = t; i < total; i += FIND_NT) {
      const uint32_t b = pat[o0 + i];
      s_pat[i] = (uint8_t)(IC ? fold_byte(b) : b);
    }
    if (!FEW)
      for (int i = 0; i < 8; i++) s_bm[t + i * FIND_NT] = 0;
  }
  __syncthreads();
  if (FEW) {
    if (t < n_pat) {
      const uint32_t o = P.off[t] - o0, m = P.off[t + 1] - P.off[t];
      uint32_t h = 0;
      for (uint32_t i = 0; i < 4 && i < m; i++) h |= (uint32_t)s_pat[o + i] << (8 * i);
      s_head[t] = h;
      s_mask[t] = m >= 4 ? 0xFFFFFFFFu : (1u << (8 * m)) - 1u;
    }
  } else {
    // every spelling of the first two bytes: a folded letter stands for both of its cases
    for (uint32_t j = 0; j < n_pat; j++) {
      const uint32_t o = P.off[j] - o0, m = P.off[j + 1] - P.off[j];
      const uint32_t a0 = s_pat[o], a1 = (IC && (a0 - 'a') < 26u) ? a0 - 32u : a0;
      if (m == 1) {                                   // any second byte: thread t sets (a, t)
        atomicOr(&s_bm[(a0 | (t << 8)) >> 5], 1u << (a0 & 31u));
        atomicOr(&s_bm[(a1 | (t << 8)) >> 5], 1u << (a1 & 31u));
      } else if (t < 4) {
        const uint32_t b0 = s_pat[o + 1], b1 = (IC && (b0 - 'a') < 26u) ? b0 - 32u : b0;
        const uint32_t idx = ((t & 1u) ? a1 : a0) | (((t & 2u) ? b1 : b0) << 8);
        atomicOr(&s_bm[idx >> 5], 1u << (idx & 31u));
      }
    }
  }
  __syncthreads();

  const uint64_t lo = raw_off[0], hi = raw_off[n_rec];              // the records cover [lo, hi) of raw
  auto ld16 = [&](uint64_t g) -> uint4 {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (g + 16 <= raw_bytes) v = load_u4_unaligned(raw + g);
    else if (g < raw_bytes) { uint8_t tmp[16]; for (int bb = 0; bb < 16; bb++) tmp[bb] = (g + bb < raw_bytes) ? raw[g + bb] : (uint8_t)0; __builtin_memcpy(&v, tmp, 16); }
    return v;
  };
  auto ld4 = [&](uint64_t g) -> uint32_t {
    uint32_t v = 0;
    if (g + 4 <= raw_bytes) v = load_u32_unaligned(raw + g);
    else if (g < raw_bytes) { for (int bb = 0; bb < 4; bb++) v |= (g + bb < raw_bytes) ? (uint32_t)raw[g + bb] << (8 * bb) : 0u; }
    return v;
  };

  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t gs0 = tile * (uint64_t)FIND_TILE + (uint64_t)t * FIND_STRIP;
    // the strip and the first four bytes of the next one: a window at the strip's last position reads three bytes past it
    uint32_t w[FIND_STRIP / 4 + 1];
#pragma unroll
    for (int j = 0; j < FIND_STRIP / 16; j++) {
      const uint4 v = ld16(gs0 + 16 * j);
      w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
    }
    w[FIND_STRIP / 4] = ld4(gs0 + FIND_STRIP);

    // ---- filter: cand = positions where some pattern may start ----
    uint32_t cand[FIND_WORDS];
#pragma unroll
    for (int g = 0; g < FIND_WORDS; g++) cand[g] = 0;
    if (FEW) {
      if (IC) {
#pragma unroll
        for (int d = 0; d <= FIND_STRIP / 4; d++) w[d] = fold_dword(w[d]);
      }
#pragma unroll
      for (int g = 0; g < FIND_WORDS; g++) {
        // (window ^ head) & mask == 0 <=> the head matches: one v_min per position into a running minimum; the rare word with a
        // zero is replayed for its positions (l2_hash_kernel's way with its threshold).  The word's 32 windows serve every pattern.
        uint32_t win[32];
#pragma unroll
        for (int k = 0; k < 32; k++) {
          const int d = g * 8 + (k >> 2), b = k & 3;
          win[k] = b ? __builtin_amdgcn_alignbyte(w[d + 1], w[d], (uint32_t)b) : w[d];
        }
        for (uint32_t j = 0; j < n_pat; j++) {
          const uint32_t h = s_head[j], mk = s_mask[j];
          uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
          for (int k = 0; k < 32; k++) {
            const uint32_t x = (win[k] ^ h) & mk;
            mn = x < mn ? x : mn;
          }
          if (mn == 0) {
            uint32_t cm = 0;
#pragma unroll
            for (int k = 0; k < 32; k++) cm |= (((win[k] ^ h) & mk) == 0 ? 1u : 0u) << k;
            cand[g] |= cm;
          }
        }
      }
    } else {
#pragma unroll
      for (int g = 0; g < FIND_WORDS; g++) {
        uint32_t cm = 0;
#pragma unroll
        for (int k = 0; k < 32; k++) {
          const int d = g * 8 + (k >> 2), b = k & 3;
          const uint32_t idx = b < 3 ? ((w[d] >> (8 * b)) & 0xFFFFu) : (__builtin_amdgcn_alignbyte(w[d + 1], w[d], 3u) & 0xFFFFu);
          cm |= ((s_bm[idx >> 5] >> (idx & 31u)) & 1u) << k;
        }
        cand[g] = cm;
      }
    }
#pragma unroll
    for (int g = 0; g < FIND_WORDS; g++) cand[g] &= range_mask(gs0 + 32 * g, lo, hi);

    // ---- verify: hb = positions where at least one pattern matches inside its record, nh = (position, pattern) pairs ----
    uint32_t hb[FIND_WORDS];
    uint32_t nh = 0;
#pragma unroll
    for (int g = 0; g < FIND_WORDS; g++) hb[g] = 0;
    uint64_t rec0 = 0;
    if (cand[0] | cand[1] | cand[2] | cand[3]) {
      rec0 = last_le(raw_off, 0, n_rec, gs0 > lo ? gs0 : lo);
      uint64_t r = rec0;
      auto verify_word = [&](uint32_t c, uint32_t& h, uint64_t start) {
        while (c) {
          const uint32_t b = (uint32_t)__builtin_ctz(c);
          c &= c - 1;
          const uint64_t p = start + b;
          while (r + 1 < n_rec && raw_off[r + 1] <= p) r++;
          const uint64_t end = raw_off[r + 1];
          uint32_t k = 0;
          for (uint32_t j = 0; j < n_pat; j++) {
            const uint32_t o = P.off[j] - o0, m = P.off[j + 1] - P.off[j];
            if (p + m <= end && find_match<IC>(raw + p, s_pat + o, m)) k++;
          }
          if (k) { h |= 1u << b; nh += k; }
        }
      };
      verify_word(cand[0], hb[0], gs0);
      verify_word(cand[1], hb[1], gs0 + 32);
      verify_word(cand[2], hb[2], gs0 + 64);
      verify_word(cand[3], hb[3], gs0 + 96);
    }

    // ---- emit: one reservation per workgroup, then per pattern (a loop every lane runs n_pat times) the lane's hits ----
    uint32_t total;
    const uint32_t my = block_exclusive_scan<FIND_NT>(nh, s_red, &total);
    total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
    if (total) {
      if (t == 0) {
        const unsigned long long base = atomicAdd(n_hits, (unsigned long long)total);
        if (hits_cap && base + total > hits_cap) atomicOr(status, 1u);
        s_base = base;
      }
      __syncthreads();
      uint64_t wr = s_base + my;
      for (uint32_t j = 0; j < n_pat; j++) {
        const uint32_t o = P.off[j] - o0, m = P.off[j + 1] - P.off[j];
        unsigned long long cj = 0;
        uint64_t r = rec0;
        auto emit_word = [&](uint32_t c, uint64_t start) {
          while (c) {
            const uint32_t b = (uint32_t)__builtin_ctz(c);
            c &= c - 1;
            const uint64_t p = start + b;
            while (r + 1 < n_rec && raw_off[r + 1] <= p) r++;
            if (p + m <= raw_off[r + 1] && find_match<IC>(raw + p, s_pat + o, m)) {
              if (wr < hits_cap) hits[wr] = (p << 8) | j;
              wr++;
              cj += mult ? mult[r] : 1u;
            }
          }
        };
        emit_word(hb[0], gs0);
        emit_word(hb[1], gs0 + 32);
        emit_word(hb[2], gs0 + 64);
        emit_word(hb[3], gs0 + 96);
        if (cj) atomicAdd(&counts[j], cj);
      }
    }
  }
}

// ---- seams --------------------------------------------------------------------------------------------------------------------
// One thread and trip per (chunk c, distance d = 1 .. max_len - 1 of the start from the chunk's end).  The start o = cuts[c + 1] - d lies in c;
// pattern j is a seam hit there iff m_j > d (it crosses cuts[c + 1]), o + m_j <= N and the bytes agree, read through the chunk map.
template <bool IC>
__global__ __launch_bounds__(FIND_NT) void find_seams_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                             const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                             uint64_t n_chunks, const uint8_t* __restrict__ pat, FindPats P,
                                                             unsigned long long* __restrict__ hits, uint64_t hits_cap, unsigned long long* n_hits,
                                                             unsigned long long* counts, uint32_t* status, uint64_t n_threads) {
  __shared__ uint8_t s_pat[FIND_PAT_BYTES];           // the patterns back to back (folded when IC)
  __shared__ uint32_t s_red[FIND_NT / 64 + 1];
  __shared__ unsigned long long s_base;
  if (*status & 2u) return;
  const uint32_t t = threadIdx.x;
  const uint32_t n_pat = P.n, o0 = P.off[0];
  for (uint32_t i = t; i < P.off[n_pat] - o0; i += FIND_NT) {
    const uint32_t b = pat[o0 + i];
    s_pat[i] = (uint8_t)(IC ? fold_byte(b) : b);
  }
  __syncthreads();
  const uint32_t span = P.max_len - 1;
  const uint64_t n = cuts[n_chunks];
  for (uint64_t id0 = (uint64_t)blockIdx.x * FIND_NT; id0 < n_threads; id0 += (uint64_t)gridDim.x * FIND_NT) {
    const uint64_t id = id0 + t;
    uint32_t hm = 0;                                  // bit j: pattern j is a seam hit at o
    uint64_t o = 0;
    if (id < n_threads) {
      const uint64_t c = id / span, d = id % span + 1;
      const uint64_t c0 = cuts[c], c1 = cuts[c + 1];
      if (d <= c1 - c0) {
        o = c1 - d;
        uint32_t b0 = raw[raw_off[slot[c]] + (o - c0)];
        if (IC) b0 = fold_byte(b0);
        for (uint32_t j = 0; j < n_pat; j++) {
          const uint32_t po = P.off[j] - o0, m = P.off[j + 1] - P.off[j];
          if (m > d && o + m <= n && s_pat[po] == b0) {
            uint64_t k = c;
            bool ok = true;
            for (uint32_t i = 1; i < m && ok; i++) {
              const uint64_t q = o + i;
              while (q >= cuts[k + 1]) k++;           // q < N = cuts[n_chunks]: k stays below n_chunks
              uint32_t b = raw[raw_off[slot[k]] + (q - cuts[k])];
              if (IC) b = fold_byte(b);
              ok = b == s_pat[po + i];
            }
            if (ok) hm |= 1u << j;
          }
        }
      }
    }
    uint32_t total;
    const uint32_t my = block_exclusive_scan<FIND_NT>((uint32_t)__builtin_popcount(hm), s_red, &total);
    total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
    if (total) {
      if (t == 0) {
        const unsigned long long base = atomicAdd(n_hits, (unsigned long long)total);
        if (hits_cap && base + total > hits_cap) atomicOr(status, 1u);
        s_base = base;
      }
      __syncthreads();
      uint64_t wr = s_base + my;
      for (uint32_t j = 0; j < n_pat; j++) {
        if ((hm >> j) & 1u) {
          if (wr < hits_cap) hits[wr] = (o << 8) | j;
          wr++;
          atomicAdd(&counts[j], 1ull);
        }
      }
    }
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
static int find_patterns(const uint32_t* pat_off, uint32_t n_pat, uint32_t flags, FindPats* P) {
  if (!pat_off || n_pat == 0 || n_pat > HMSE_FIND_MAX_PATTERNS || (flags & ~HMSE_FIND_IGNORE_CASE)) return HMSE_EINVAL;
  P->n = n_pat;
  P->max_len = 0;
  for (uint32_t j = 0; j <= n_pat; j++) P->off[j] = pat_off[j];
  for (uint32_t j = n_pat + 1; j <= HMSE_FIND_MAX_PATTERNS; j++) P->off[j] = pat_off[n_pat];
  for (uint32_t j = 0; j < n_pat; j++) {
    if (pat_off[j + 1] <= pat_off[j] || pat_off[j + 1] - pat_off[j] > HMSE_FIND_MAX_LEN) return HMSE_EINVAL;
    const uint32_t m = pat_off[j + 1] - pat_off[j];
    if (m > P->max_len) P->max_len = m;
  }
  return HMSE_OK;
}

// the tables and nothing else, at this family's geometry
static int find_validate(const uint64_t* raw_off, uint64_t n_rec, uint64_t raw_bytes, const uint64_t* cuts, const uint64_t* slot,
                         uint64_t n_chunks, const uint64_t* chunk_out, uint32_t* status, hipStream_t stream) {
  return tables_validate<FIND_NT>(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, chunk_out, status, FIND_MAX_BLOCKS, stream);
}

extern "C" int hmse_find_scan(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint32_t* mult,
                              const uint8_t* pat, const uint32_t* pat_off, uint32_t n_pat, uint32_t flags, uint64_t* hits,
                              uint64_t hits_cap, uint64_t* n_hits, uint64_t* counts, uint32_t* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FindPats P;
  if (find_patterns(pat_off, n_pat, flags, &P) != HMSE_OK || !pat || !n_hits || !counts || !status) return HMSE_EINVAL;
  if (n_rec && (!raw_off || (raw_bytes && !raw))) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(n_hits, 0, 8, stream);
  HMSE_FILL(counts, 0, 8 * (size_t)n_pat, stream);
  if (n_rec == 0 || raw_bytes == 0) return HMSE_OK;
  if (!hits) hits_cap = 0;
  int rc = find_validate(raw_off, n_rec, raw_bytes, nullptr, nullptr, 0, nullptr, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t n_tiles = (raw_bytes + FIND_TILE - 1) / FIND_TILE;
  const dim3 grid((uint32_t)(n_tiles < FIND_MAX_BLOCKS ? n_tiles : FIND_MAX_BLOCKS)), block(FIND_NT);
  const bool few = n_pat <= FIND_FEW, ic = (flags & HMSE_FIND_IGNORE_CASE) != 0;
  unsigned long long *h = (unsigned long long*)hits, *nh = (unsigned long long*)n_hits, *cn = (unsigned long long*)counts;
  PROF_BEGIN(HMSE_STAGE_FIND_SCAN, stream);
#define HMSE_FIND_SCAN(F, I) find_scan_kernel<F, I><<<grid, block, 0, stream>>>(raw, raw_bytes, raw_off, n_rec, mult, pat, P, h, hits_cap, nh, cn, status, n_tiles)
  if (few) { if (ic) HMSE_FIND_SCAN(true, true); else HMSE_FIND_SCAN(true, false); }
  else     { if (ic) HMSE_FIND_SCAN(false, true); else HMSE_FIND_SCAN(false, false); }
#undef HMSE_FIND_SCAN
  PROF_END(HMSE_STAGE_FIND_SCAN, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_find_seams(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                               const uint64_t* slot, uint64_t n_chunks, const uint8_t* pat, const uint32_t* pat_off, uint32_t n_pat,
                               uint32_t flags, uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits, uint64_t* counts, uint32_t* status,
                               void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FindPats P;
  if (find_patterns(pat_off, n_pat, flags, &P) != HMSE_OK || !pat || !n_hits || !counts || !status) return HMSE_EINVAL;
  if (n_chunks && (!cuts || !slot || !raw_off || !raw)) return HMSE_EINVAL;
  if (n_chunks > (1ull << 40)) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(n_hits, 0, 8, stream);
  HMSE_FILL(counts, 0, 8 * (size_t)n_pat, stream);
  if (n_chunks == 0) return HMSE_OK;
  if (!hits) hits_cap = 0;
  int rc = find_validate(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, nullptr, status, stream);
  if (rc != HMSE_OK) return rc;
  if (P.max_len < 2) return HMSE_OK;                  // a one-byte pattern crosses no boundary
  const uint64_t n_threads = n_chunks * (uint64_t)(P.max_len - 1);
  uint64_t nb = (n_threads + FIND_NT - 1) / FIND_NT;
  if (nb > FIND_MAX_BLOCKS) nb = FIND_MAX_BLOCKS;     // (the patterns are staged once per workgroup; the rest by the grid stride)
  unsigned long long *h = (unsigned long long*)hits, *nh = (unsigned long long*)n_hits, *cn = (unsigned long long*)counts;
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  if (flags & HMSE_FIND_IGNORE_CASE)
    find_seams_kernel<true><<<dim3((uint32_t)nb), dim3(FIND_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, pat, P, h, hits_cap, nh, cn, status, n_threads);
  else
    find_seams_kernel<false><<<dim3((uint32_t)nb), dim3(FIND_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, pat, P, h, hits_cap, nh, cn, status, n_threads);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_find_place(const uint64_t* hits, uint64_t n_hits, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                               const uint64_t* slot, uint64_t n_chunks, const uint64_t* chunk_out, uint64_t* out, uint64_t out_cap,
                               uint32_t* status, void* stream_) {
  return place<8, FIND_NT>(find_validate, hits, n_hits, raw_off, n_rec, cuts, slot, n_chunks, chunk_out, out, out_cap, status, stream_);
}
