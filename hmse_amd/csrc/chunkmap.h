// chunkmap.h — the three tables through which every search kernel reads a store, once: raw_off (n_rec + 1 bounds of the decoded records
// in raw), cuts (n_chunks + 1 bounds of the chunks in the corpus) and slot (the record of every chunk).  Corpus byte q of chunk k is
// raw[raw_off[slot[k]] + q - cuts[k]].  find.hip, findset.hip, lines.hip, regex.hip, regexa.hip and approx.hip include this after common.h; the CPU emulators
// (tools/*_emu.cpp) include it after tools/hip_on_cpu.h, so the device part uses only what both provide and the file includes nothing.
// Everything here is a template or __forceinline__: several translation units include it (five of them link into one library).
#pragma once

// ---- bytes --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fold_byte(uint32_t b) { return (b - 'A') < 26u ? (b | 0x20u) : b; }
// A..Z -> a..z in the four bytes of a dword, every other value (>= 0x80 included) as it is
__device__ __forceinline__ uint32_t fold_dword(uint32_t w) {
  const uint32_t t = w & 0x7F7F7F7Fu;
  const uint32_t ge = t + 0x3F3F3F3Fu;                // bit 7 of a byte: its low seven bits >= 'A'
  const uint32_t gt = t + 0x25252525u;                // ...                               >  'Z'
  return w | (((ge & ~gt & ~w) & 0x80808080u) >> 2);
}

// bits b of a 32-position word starting at `start` with lo <= start + b < hi
__device__ __forceinline__ uint32_t range_mask(uint64_t start, uint64_t lo, uint64_t hi) {
  uint32_t m = 0xFFFFFFFFu;
  if (start + 32 > hi) m = start >= hi ? 0u : (0xFFFFFFFFu >> (32u - (uint32_t)(hi - start)));
  if (start < lo) m = (lo - start >= 32) ? 0u : (m & (0xFFFFFFFFu << (uint32_t)(lo - start)));
  return m;
}

// ---- lookups ------------------------------------------------------------------------------------------------------------------
// largest i in [a, b) with arr[i] <= x (a if there is none): the record of a raw position in raw_off, the chunk of a corpus position
// in cuts (empty chunks hold nothing), the chunk of an output element in chunk_out
__device__ __forceinline__ uint64_t last_le(const uint64_t* __restrict__ arr, uint64_t a, uint64_t b, uint64_t x) {
  while (b - a > 1) {
    const uint64_t mid = a + ((b - a) >> 1);
    if (arr[mid] <= x) a = mid; else b = mid;
  }
  return a;
}

// corpus byte q, with k a chunk at or in front of q's (k moves forward to q's chunk; q < N = cuts[n_chunks] keeps it below n_chunks)
__device__ __forceinline__ uint32_t corpus_byte(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot, uint64_t q, uint64_t& k) {
  while (q >= cuts[k + 1]) k++;
  return raw[raw_off[slot[k]] + (q - cuts[k])];
}

// ---- the table rules ----------------------------------------------------------------------------------------------------------
// Index i of max(n_rec, n_chunks) breaks a rule: raw_off or cuts (or chunk_out, where there is one: it also starts at 0) descending,
// records beyond raw_bytes, slot[i] >= n_rec, a chunk whose length is not its record's.  A validate kernel sets status bit 1 for it, and
// every later kernel of the call leaves when it finds the bit: nothing is then read through these tables.
__device__ __forceinline__ bool tables_bad_at(uint64_t i, const uint64_t* __restrict__ raw_off, uint64_t n_rec, uint64_t raw_bytes,
                                              const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot, uint64_t n_chunks,
                                              const uint64_t* __restrict__ chunk_out) {
  bool bad = false;
  if (i < n_rec) {
    bad |= raw_off[i] > raw_off[i + 1];
    if (i == 0) bad |= raw_off[n_rec] > raw_bytes;
  }
  if (i < n_chunks) {
    bad |= cuts[i] > cuts[i + 1];
    const uint64_t s = slot[i];
    if (s >= n_rec) bad = true;
    else bad |= raw_off[s + 1] - raw_off[s] != cuts[i + 1] - cuts[i];
    if (chunk_out) bad |= chunk_out[i] > chunk_out[i + 1] || (i == 0 && chunk_out[0] != 0);
  }
  return bad;
}

// the rules and nothing else (findset.hip and regex.hip check their set and their automaton in the same pass, in kernels of their own)
template <int NT>
__global__ __launch_bounds__(NT) void tables_validate_kernel(const uint64_t* __restrict__ raw_off, uint64_t n_rec, uint64_t raw_bytes,
                                                             const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                             uint64_t n_chunks, const uint64_t* __restrict__ chunk_out, uint32_t* status) {
  const uint64_t n = n_rec > n_chunks ? n_rec : n_chunks;
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride)
    bad |= tables_bad_at(i, raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, chunk_out);
  if (bad) atomicOr(status, 2u);
}

// ---- place --------------------------------------------------------------------------------------------------------------------
// A hit word is position << LOW_BITS | low field.  The sorted in-record hits are laid out at every chunk that maps to their record
// (POINTERs included): one thread per output element e, its chunk k (chunk_out[k] <= e < chunk_out[k + 1]), the (e - chunk_out[k])-th
// hit of record slot[k] in the sorted list, its position moved from raw to the corpus and its low field passed through.
template <int LOW_BITS, int NT>
__global__ __launch_bounds__(NT) void place_kernel(const unsigned long long* __restrict__ hits, uint64_t n_hits,
                                                   const uint64_t* __restrict__ raw_off, const uint64_t* __restrict__ cuts,
                                                   const uint64_t* __restrict__ slot, uint64_t n_chunks,
                                                   const uint64_t* __restrict__ chunk_out, unsigned long long* __restrict__ out,
                                                   uint64_t out_cap, uint32_t* status) {
  if (*status & 2u) return;
  const uint64_t e = (uint64_t)blockIdx.x * NT + threadIdx.x;
  const uint64_t total = chunk_out[n_chunks];
  if (e == 0 && total > out_cap) atomicOr(status, 1u);
  if (e >= total || e >= out_cap) return;
  const uint64_t k = last_le(chunk_out, 0, n_chunks, e), s = slot[k], r0 = raw_off[s], r1 = raw_off[s + 1];
  uint64_t x = 0, y = n_hits;                         // first hit at or behind r0
  while (x < y) {
    const uint64_t mid = x + ((y - x) >> 1);
    if ((hits[mid] >> LOW_BITS) < r0) x = mid + 1; else y = mid;
  }
  const uint64_t idx = x + (e - chunk_out[k]);
  bool bad = idx >= n_hits;
  if (!bad) {
    const unsigned long long h = hits[idx];
    const uint64_t pos = h >> LOW_BITS;
    bad = pos < r0 || pos >= r1;
    if (!bad) out[e] = ((cuts[k] + (pos - r0)) << LOW_BITS) | (h & ((1ull << LOW_BITS) - 1));
  }
  if (bad) atomicOr(status, 2u);                      // chunk_out is not the count of the record's hits
}

// ---- host side (the library only) ---------------------------------------------------------------------------------------------
#ifdef __HIPCC__
template <int NT>
static int tables_validate(const uint64_t* raw_off, uint64_t n_rec, uint64_t raw_bytes, const uint64_t* cuts, const uint64_t* slot,
                           uint64_t n_chunks, const uint64_t* chunk_out, uint32_t* status, uint64_t max_blocks, hipStream_t stream) {
  const uint64_t n = n_rec > n_chunks ? n_rec : n_chunks;
  if (n == 0) return HMSE_OK;
  uint64_t nb = (n + NT - 1) / NT;
  if (nb > max_blocks) nb = max_blocks;
  tables_validate_kernel<NT><<<dim3((uint32_t)nb), dim3(NT), 0, stream>>>(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, chunk_out, status);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

// The body of hmse_find_place and hmse_findset_place.  `validate` is the family's check of the tables with chunk_out; raw_bytes is not
// an argument here: the records' end bounds nothing that is read (the hits carry the positions).
template <int LOW_BITS, int NT, typename Validate>
static int place(Validate validate, const uint64_t* hits, uint64_t n_hits, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                 const uint64_t* slot, uint64_t n_chunks, const uint64_t* chunk_out, uint64_t* out, uint64_t out_cap, uint32_t* status,
                 void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!status || (n_hits && !hits) || (out_cap && !out)) return HMSE_EINVAL;
  if (n_chunks && (!cuts || !slot || !raw_off || !chunk_out)) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n_chunks == 0) return HMSE_OK;
  int rc = validate(raw_off, n_rec, ~0ull, cuts, slot, n_chunks, chunk_out, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t nb = out_cap ? (out_cap + NT - 1) / NT : 1;
  if (nb > 0x7FFFFFFFull) return HMSE_EINVAL;
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  place_kernel<LOW_BITS, NT><<<dim3((uint32_t)nb), dim3(NT), 0, stream>>>((const unsigned long long*)hits, n_hits, raw_off, cuts, slot, n_chunks,
                                                                           chunk_out, (unsigned long long*)out, out_cap, status);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
#endif
