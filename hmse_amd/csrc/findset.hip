// findset.hip — a whole dictionary of byte patterns looked for in one pass over the decoded records of a store (hmse_amd/find.py
// PatternSet; include/hmse.h hmse_findset_*).  find.hip answers up to 32 patterns per pass and its work per byte grows with them; here
// the patterns (4..256 bytes, up to 2^20 of them) are compiled once into a hashed directory (struct hmse_findset) and the work per
// position does not depend on their number as long as the filter rejects the position:
//   (1) findset_scan_kernel  — find.hip's scan geometry (a strip per lane, 16-byte loads with overhang, the 4-byte window of every position
//                              from v_alignbyte, folded once per dword when the case is ignored); the window is hashed and probed in a
//                              64 KiB bitmap held in LDS; a survivor is looked up in the directory (two adjacent loads and a short walk
//                              over the keys) and verified byte by byte inside its record.  A lane's number of hits is unbounded (128
//                              positions x 253 nested prefixes), so it COUNTS in a first walk, the workgroup reserves once per tile, and
//                              the lane walks again and stores;
//   (2) findset_seams_kernel — one thread per (chunk, distance from its end): the window gathered through the chunk map, the same filter
//                              (read from memory) and directory, only the patterns longer than the distance verified; count, reserve, store;
//   (3) place_kernel<HMSE_FINDSET_ID_BITS> — the in-record hits laid out at every chunk of their record (chunkmap.h).
// Every call starts with findset_validate_kernel over the tables AND the set: the kernels behind it leave when it set status bit 1.
// No kernel holds a cross-lane operation or a barrier inside a loop that lanes leave at different times (tools/isa_audit.py).
#include "common.h"
#include "chunkmap.h"

constexpr int FSET_NT = 512;                          // threads per workgroup: two fit on a CU beside their LDS bitmaps, 4 waves per SIMD
constexpr int FSET_STRIP = 128;                       // S: bytes per lane
constexpr int FSET_TILE = FSET_NT * FSET_STRIP;       // T: 64 KiB of records per workgroup and trip
constexpr int FSET_WORDS = FSET_STRIP / 32;           // candidate bitmap dwords per lane
constexpr uint32_t FSET_BM_WORDS = 1u << (HMSE_FINDSET_BITMAP_BITS - 5);   // 16384 dwords = 64 KiB
constexpr uint32_t FSET_BM_SHIFT = 32 - HMSE_FINDSET_BITMAP_BITS;
constexpr uint32_t FSET_MAX_BLOCKS = 512;             // 256 CUs x 2 workgroups (the LDS bitmap); the tiles beyond by the grid stride
constexpr uint32_t FSET_POS_BITS = 40;                // positions below 2^40, ids below 2^24 in a hit word

// The set as the kernels get it: hmse_findset's arrays and header by value.
struct FsetDev {
  const uint8_t* upat; const uint32_t *uoff, *ukey, *uid, *dir, *bitmap;
  uint64_t pat_bytes; uint32_t n, n_ids, bits, max_len, folded;
};

__device__ __forceinline__ uint32_t fset_hash(uint32_t key) { return key * HMSE_FINDSET_HASH; }

template <bool IC>
__device__ __forceinline__ bool fset_match(const uint8_t* __restrict__ p, const uint8_t* __restrict__ sp, uint32_t m) {
  for (uint32_t i = 0; i < m; i++) {
    uint32_t b = p[i];
    if (IC) b = fold_byte(b);
    if (b != sp[i]) return false;
  }
  return true;
}

// ---- tables and set -----------------------------------------------------------------------------------------------------------
// status bit 1: tables that break a rule of chunkmap.h (tables_bad_at), a corpus of 2^40 bytes or more (a hit word holds 40 bits of
// position), and the set: a directory that descends or does not cover [0, n), an id >= n_ids, a byte range that descends, leaves upat or is not 4..max_len long, a key that is not the first four bytes of
// its pattern (folded ones if the set is), an entry outside its directory cell or without its bit in the bitmap.
__global__ __launch_bounds__(FSET_NT) void findset_validate_kernel(const uint64_t* __restrict__ raw_off, uint64_t n_rec, uint64_t raw_bytes,
                                                                   const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                                   uint64_t n_chunks, const uint64_t* __restrict__ chunk_out, FsetDev F,
                                                                   uint64_t n, uint32_t* status) {
  const uint64_t stride = (uint64_t)gridDim.x * FSET_NT;
  const uint64_t cells = F.n ? (1ull << F.bits) : 0;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * FSET_NT + threadIdx.x; i < n; i += stride) {
    bad |= tables_bad_at(i, raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, chunk_out);
    if (i == 0 && n_chunks) bad |= (cuts[n_chunks] >> FSET_POS_BITS) != 0;
    if (i < cells) {
      bad |= F.dir[i] > F.dir[i + 1];
      if (i == 0) bad |= F.dir[0] != 0 || F.dir[cells] != F.n;
    }
    if (i < F.n) {
      const uint32_t a = F.uoff[i], e = F.uoff[i + 1], key = F.ukey[i];
      bad |= F.uid[i] >= F.n_ids;
      if (e < a || e - a < HMSE_FINDSET_MIN_LEN || e - a > F.max_len || e > F.pat_bytes) bad = true;
      else bad |= load_u32_unaligned(F.upat + a) != key;
      if (F.folded) bad |= fold_dword(key) != key;
      const uint32_t h = fset_hash(key), cell = h >> (32u - F.bits), bit = h >> FSET_BM_SHIFT;
      bad |= F.dir[cell] > i || F.dir[cell + 1] <= i;
      bad |= ((F.bitmap[bit >> 5] >> (bit & 31u)) & 1u) == 0;
    }
  }
  if (bad) atomicOr(status, 2u);
}

// ---- the walk over a position's directory cell --------------------------------------------------------------------------------
// Every pattern of the set that matches at raw + p and ends at or before `end` (p + 4 <= end: the key was read inside the record).
// EMIT false: -> their number.  EMIT true: each stored at hits[wr++] (below hits_cap) and weighed into counts.
template <bool IC, bool EMIT>
__device__ __forceinline__ uint32_t fset_walk(const uint8_t* __restrict__ raw, uint64_t p, uint64_t end, uint32_t weight, const FsetDev& F,
                                              unsigned long long* __restrict__ hits, uint64_t hits_cap, uint64_t& wr, unsigned long long* counts) {
  uint32_t key = load_u32_unaligned(raw + p);
  if (IC) key = fold_dword(key);
  const uint32_t cell = fset_hash(key) >> (32u - F.bits);
  uint32_t i = F.dir[cell], i1 = F.dir[cell + 1];
  if (i1 > F.n) i1 = F.n;
  uint32_t k = 0;
  for (; i < i1; i++) {
    if (F.ukey[i] != key) continue;
    const uint32_t a = F.uoff[i], m = F.uoff[i + 1] - a;
    if (p + m <= end && fset_match<IC>(raw + p + 4, F.upat + a + 4, m - 4)) {
      if (EMIT) {
        const uint32_t id = F.uid[i];
        if (wr < hits_cap) hits[wr] = ((unsigned long long)p << HMSE_FINDSET_ID_BITS) | id;
        wr++;
        atomicAdd(&counts[id], (unsigned long long)weight);
      }
      k++;
    }
  }
  return k;
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------
template <bool IC>
__global__ __launch_bounds__(FSET_NT) void findset_scan_kernel(const uint8_t* __restrict__ raw, uint64_t raw_bytes, const uint64_t* __restrict__ raw_off,
                                                               uint64_t n_rec, const uint32_t* __restrict__ mult, FsetDev F,
                                                               unsigned long long* __restrict__ hits, uint64_t hits_cap, unsigned long long* n_hits,
                                                               unsigned long long* counts, uint32_t* status, uint64_t n_tiles) {
  __shared__ __attribute__((aligned(16))) uint32_t s_bm[FSET_BM_WORDS];   // bit (h >> 13): some pattern's key hashes to h
  __shared__ uint32_t s_red[FSET_NT / 64 + 1];
  __shared__ unsigned long long s_base;

  if (*status & 2u) return;                           // inconsistent tables or set (findset_validate_kernel)
  const uint32_t t = threadIdx.x;
  {
    for (uint32_t i = t; i < FSET_BM_WORDS; i += FSET_NT) s_bm[i] = F.bitmap[i];
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
    const uint64_t gs0 = tile * (uint64_t)FSET_TILE + (uint64_t)t * FSET_STRIP;
    // the strip and the first four bytes of the next one: a window at the strip's last position reads three bytes past it
    uint32_t w[FSET_STRIP / 4 + 1];
#pragma unroll
    for (int j = 0; j < FSET_STRIP / 16; j++) {
      const uint4 v = ld16(gs0 + 16 * j);
      w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
    }
    w[FSET_STRIP / 4] = ld4(gs0 + FSET_STRIP);
    if (IC) {
#pragma unroll
      for (int d = 0; d <= FSET_STRIP / 4; d++) w[d] = fold_dword(w[d]);
    }

    // ---- filter: cand = positions whose window's hash has its bit in the bitmap ----
    uint32_t cand[FSET_WORDS];
#pragma unroll
    for (int g = 0; g < FSET_WORDS; g++) {
      uint32_t cm = 0;
#pragma unroll
      for (int k = 0; k < 32; k++) {
        const int d = g * 8 + (k >> 2), b = k & 3;
        const uint32_t win = b ? __builtin_amdgcn_alignbyte(w[d + 1], w[d], (uint32_t)b) : w[d];
        const uint32_t bit = fset_hash(win) >> FSET_BM_SHIFT;
        cm |= ((s_bm[bit >> 5] >> (bit & 31u)) & 1u) << k;
      }
      cand[g] = cm & range_mask(gs0 + 32 * g, lo, hi);
    }

    // ---- count: hb = positions where at least one pattern matches inside its record, nh = (position, pattern) pairs ----
    uint32_t hb[FSET_WORDS];
    uint32_t nh = 0;
#pragma unroll
    for (int g = 0; g < FSET_WORDS; g++) hb[g] = 0;
    uint64_t rec0 = 0;
    if (cand[0] | cand[1] | cand[2] | cand[3]) {
      rec0 = last_le(raw_off, 0, n_rec, gs0 > lo ? gs0 : lo);
      uint64_t r = rec0, none = 0;
      auto count_word = [&](uint32_t c, uint32_t& h, uint64_t start) {
        while (c) {
          const uint32_t b = (uint32_t)__builtin_ctz(c);
          c &= c - 1;
          const uint64_t p = start + b;
          while (r + 1 < n_rec && raw_off[r + 1] <= p) r++;
          const uint64_t end = raw_off[r + 1];
          if (p + 4 > end) continue;                  // no pattern is shorter than its key
          const uint32_t k = fset_walk<IC, false>(raw, p, end, 0, F, nullptr, 0, none, nullptr);
          if (k) { h |= 1u << b; nh += k; }
        }
      };
      count_word(cand[0], hb[0], gs0);
      count_word(cand[1], hb[1], gs0 + 32);
      count_word(cand[2], hb[2], gs0 + 64);
      count_word(cand[3], hb[3], gs0 + 96);
    }

    // ---- emit: one reservation per workgroup, then every lane walks its hit positions again and stores at its place ----
    uint32_t total;
    const uint32_t my = block_exclusive_scan<FSET_NT>(nh, s_red, &total);
    total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
    if (total) {
      if (t == 0) {
        const unsigned long long base = atomicAdd(n_hits, (unsigned long long)total);
        if (hits_cap && base + total > hits_cap) atomicOr(status, 1u);
        s_base = base;
      }
      __syncthreads();
      uint64_t wr = s_base + my;
      uint64_t r = rec0;
      auto emit_word = [&](uint32_t c, uint64_t start) {
        while (c) {
          const uint32_t b = (uint32_t)__builtin_ctz(c);
          c &= c - 1;
          const uint64_t p = start + b;
          while (r + 1 < n_rec && raw_off[r + 1] <= p) r++;
          fset_walk<IC, true>(raw, p, raw_off[r + 1], mult ? mult[r] : 1u, F, hits, hits_cap, wr, counts);
        }
      };
      emit_word(hb[0], gs0);
      emit_word(hb[1], gs0 + 32);
      emit_word(hb[2], gs0 + 64);
      emit_word(hb[3], gs0 + 96);
    }
  }
}

// ---- seams --------------------------------------------------------------------------------------------------------------------
// One thread and trip per (chunk c, distance d = 1 .. max_len - 1 of the start from the chunk's end).  The start o = cuts[c + 1] - d lies in c;
// a pattern of m bytes is a seam hit there iff m > d (it crosses cuts[c + 1]), o + m <= N and the bytes agree, read through the chunk map.
template <bool IC, bool EMIT>
__device__ __forceinline__ uint32_t fset_seam_walk(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off, const uint64_t* __restrict__ cuts,
                                                   const uint64_t* __restrict__ slot, uint64_t c, uint64_t d, uint64_t o, uint64_t n, uint32_t key,
                                                   const FsetDev& F, unsigned long long* __restrict__ hits, uint64_t hits_cap, uint64_t& wr,
                                                   unsigned long long* counts) {
  const uint32_t cell = fset_hash(key) >> (32u - F.bits);
  uint32_t i = F.dir[cell], i1 = F.dir[cell + 1];
  if (i1 > F.n) i1 = F.n;
  uint32_t found = 0;
  for (; i < i1; i++) {
    if (F.ukey[i] != key) continue;
    const uint32_t a = F.uoff[i], m = F.uoff[i + 1] - a;
    if (m <= d || o + m > n) continue;
    uint64_t k = c;
    bool ok = true;
    for (uint32_t j = 4; j < m && ok; j++) {
      uint32_t b = corpus_byte(raw, raw_off, cuts, slot, o + j, k);
      if (IC) b = fold_byte(b);
      ok = b == F.upat[a + j];
    }
    if (!ok) continue;
    if (EMIT) {
      const uint32_t id = F.uid[i];
      if (wr < hits_cap) hits[wr] = ((unsigned long long)o << HMSE_FINDSET_ID_BITS) | id;
      wr++;
      atomicAdd(&counts[id], 1ull);
    }
    found++;
  }
  return found;
}

template <bool IC>
__global__ __launch_bounds__(FSET_NT) void findset_seams_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                                const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                                uint64_t n_chunks, FsetDev F, unsigned long long* __restrict__ hits, uint64_t hits_cap,
                                                                unsigned long long* n_hits, unsigned long long* counts, uint32_t* status,
                                                                uint64_t n_threads) {
  __shared__ uint32_t s_red[FSET_NT / 64 + 1];
  __shared__ unsigned long long s_base;
  if (*status & 2u) return;
  const uint32_t t = threadIdx.x;
  const uint32_t span = F.max_len - 1;
  const uint64_t n = cuts[n_chunks];
  for (uint64_t id0 = (uint64_t)blockIdx.x * FSET_NT; id0 < n_threads; id0 += (uint64_t)gridDim.x * FSET_NT) {
    const uint64_t id = id0 + t;
    uint32_t nh = 0, key = 0;
    uint64_t o = 0, c = 0, d = 0, none = 0;
    if (id < n_threads) {
      c = id / span; d = id % span + 1;
      const uint64_t c0 = cuts[c], c1 = cuts[c + 1];
      if (d <= c1 - c0 && c1 - d + 4 <= n) {          // the start lies in chunk c and the key inside the corpus
        o = c1 - d;
        uint64_t k = c;
        for (uint32_t j = 0; j < 4; j++) key |= corpus_byte(raw, raw_off, cuts, slot, o + j, k) << (8 * j);
        if (IC) key = fold_dword(key);
        const uint32_t bit = fset_hash(key) >> FSET_BM_SHIFT;
        if ((F.bitmap[bit >> 5] >> (bit & 31u)) & 1u)
          nh = fset_seam_walk<IC, false>(raw, raw_off, cuts, slot, c, d, o, n, key, F, nullptr, 0, none, nullptr);
      }
    }
    uint32_t total;
    const uint32_t my = block_exclusive_scan<FSET_NT>(nh, s_red, &total);
    total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
    if (total) {
      if (t == 0) {
        const unsigned long long base = atomicAdd(n_hits, (unsigned long long)total);
        if (hits_cap && base + total > hits_cap) atomicOr(status, 1u);
        s_base = base;
      }
      __syncthreads();
      uint64_t wr = s_base + my;
      if (nh) fset_seam_walk<IC, true>(raw, raw_off, cuts, slot, c, d, o, n, key, F, hits, hits_cap, wr, counts);
    }
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
// The header's ranges, checked on the host.  An empty set (n_entries == 0) needs no array.
static int fset_header(const hmse_findset* set, uint32_t flags, FsetDev* F) {
  if (!set || set->struct_size != sizeof(hmse_findset) || (flags & ~HMSE_FIND_IGNORE_CASE) || (set->flags & ~HMSE_FIND_IGNORE_CASE)) return HMSE_EINVAL;
  if (set->flags != flags) return HMSE_EINVAL;        // the set is folded iff the text is
  if (set->n_ids > HMSE_FINDSET_MAX_PATTERNS || set->n_entries > HMSE_FINDSET_MAX_PATTERNS) return HMSE_EINVAL;
  if (set->n_entries) {
    if (set->n_ids == 0 || set->dir_bits < 1 || set->dir_bits > 21) return HMSE_EINVAL;
    if (set->max_len < HMSE_FINDSET_MIN_LEN || set->max_len > HMSE_FIND_MAX_LEN) return HMSE_EINVAL;
    if (set->pat_bytes < (uint64_t)HMSE_FINDSET_MIN_LEN * set->n_entries || set->pat_bytes > (uint64_t)HMSE_FIND_MAX_LEN * set->n_entries) return HMSE_EINVAL;
    if (!set->upat || !set->uoff || !set->ukey || !set->uid || !set->dir || !set->bitmap) return HMSE_EINVAL;
  }
  F->upat = set->upat; F->uoff = set->uoff; F->ukey = set->ukey; F->uid = set->uid; F->dir = set->dir; F->bitmap = set->bitmap;
  F->pat_bytes = set->pat_bytes; F->n = set->n_entries; F->n_ids = set->n_ids; F->bits = set->dir_bits; F->max_len = set->max_len;
  F->folded = set->flags & HMSE_FIND_IGNORE_CASE;
  return HMSE_OK;
}

static int fset_validate(const uint64_t* raw_off, uint64_t n_rec, uint64_t raw_bytes, const uint64_t* cuts, const uint64_t* slot,
                         uint64_t n_chunks, const uint64_t* chunk_out, const FsetDev& F, uint32_t* status, hipStream_t stream) {
  uint64_t n = n_rec > n_chunks ? n_rec : n_chunks;
  if (F.n) {
    if (F.n > n) n = F.n;
    if ((1ull << F.bits) > n) n = 1ull << F.bits;
  }
  if (n == 0) return HMSE_OK;
  uint64_t nb = (n + FSET_NT - 1) / FSET_NT;
  if (nb > 2048) nb = 2048;
  findset_validate_kernel<<<dim3((uint32_t)nb), dim3(FSET_NT), 0, stream>>>(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, chunk_out, F, n, status);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

// no set: the tables alone, and the corpus below 2^40 bytes (hmse_findset_place)
static int fset_validate_tables(const uint64_t* raw_off, uint64_t n_rec, uint64_t raw_bytes, const uint64_t* cuts, const uint64_t* slot,
                                uint64_t n_chunks, const uint64_t* chunk_out, uint32_t* status, hipStream_t stream) {
  return fset_validate(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, chunk_out, FsetDev{}, status, stream);
}

extern "C" int hmse_findset_scan(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint32_t* mult,
                                 const hmse_findset* set, uint32_t flags, uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits,
                                 uint64_t* counts, uint32_t* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FsetDev F;
  if (fset_header(set, flags, &F) != HMSE_OK || !n_hits || !status || (F.n_ids && !counts)) return HMSE_EINVAL;
  if (n_rec && (!raw_off || (raw_bytes && !raw))) return HMSE_EINVAL;
  if (raw_bytes >> FSET_POS_BITS) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(n_hits, 0, 8, stream);
  if (F.n_ids) HMSE_FILL(counts, 0, 8 * (size_t)F.n_ids, stream);
  if (n_rec == 0 || raw_bytes == 0 || F.n == 0) return HMSE_OK;
  if (!hits) hits_cap = 0;
  int rc = fset_validate(raw_off, n_rec, raw_bytes, nullptr, nullptr, 0, nullptr, F, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t n_tiles = (raw_bytes + FSET_TILE - 1) / FSET_TILE;
  const dim3 grid((uint32_t)(n_tiles < FSET_MAX_BLOCKS ? n_tiles : FSET_MAX_BLOCKS)), block(FSET_NT);
  unsigned long long *h = (unsigned long long*)hits, *nh = (unsigned long long*)n_hits, *cn = (unsigned long long*)counts;
  PROF_BEGIN(HMSE_STAGE_FIND_SCAN, stream);
  if (flags & HMSE_FIND_IGNORE_CASE)
    findset_scan_kernel<true><<<grid, block, 0, stream>>>(raw, raw_bytes, raw_off, n_rec, mult, F, h, hits_cap, nh, cn, status, n_tiles);
  else
    findset_scan_kernel<false><<<grid, block, 0, stream>>>(raw, raw_bytes, raw_off, n_rec, mult, F, h, hits_cap, nh, cn, status, n_tiles);
  PROF_END(HMSE_STAGE_FIND_SCAN, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_findset_seams(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                                  const uint64_t* slot, uint64_t n_chunks, const hmse_findset* set, uint32_t flags, uint64_t* hits,
                                  uint64_t hits_cap, uint64_t* n_hits, uint64_t* counts, uint32_t* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FsetDev F;
  if (fset_header(set, flags, &F) != HMSE_OK || !n_hits || !status || (F.n_ids && !counts)) return HMSE_EINVAL;
  if (n_chunks && (!cuts || !slot || !raw_off || !raw)) return HMSE_EINVAL;
  if (n_chunks > (1ull << 40) || (raw_bytes >> FSET_POS_BITS)) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(n_hits, 0, 8, stream);
  if (F.n_ids) HMSE_FILL(counts, 0, 8 * (size_t)F.n_ids, stream);
  if (n_chunks == 0 || F.n == 0) return HMSE_OK;
  if (!hits) hits_cap = 0;
  int rc = fset_validate(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, nullptr, F, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t n_threads = n_chunks * (uint64_t)(F.max_len - 1);    // max_len >= 4
  uint64_t nb = (n_threads + FSET_NT - 1) / FSET_NT;
  if (nb > 4096) nb = 4096;                           // (no LDS table here: 256 CUs x 4 workgroups x 4 rounds; the rest by the grid stride)
  unsigned long long *h = (unsigned long long*)hits, *nh = (unsigned long long*)n_hits, *cn = (unsigned long long*)counts;
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  if (flags & HMSE_FIND_IGNORE_CASE)
    findset_seams_kernel<true><<<dim3((uint32_t)nb), dim3(FSET_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, F, h, hits_cap, nh, cn, status, n_threads);
  else
    findset_seams_kernel<false><<<dim3((uint32_t)nb), dim3(FSET_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, F, h, hits_cap, nh, cn, status, n_threads);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_findset_place(const uint64_t* hits, uint64_t n_hits, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                                  const uint64_t* slot, uint64_t n_chunks, const uint64_t* chunk_out, uint64_t* out, uint64_t out_cap,
                                  uint32_t* status, void* stream_) {
  return place<HMSE_FINDSET_ID_BITS, FSET_NT>(fset_validate_tables, hits, n_hits, raw_off, n_rec, cuts, slot, n_chunks, chunk_out, out, out_cap, status, stream_);
}
