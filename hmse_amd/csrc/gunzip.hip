// gunzip.hip — multi-member gzip / BGZF comes into the project (hmse_amd/gunzip.py; include/hmse_gunzip.h hmse_gzip_candidates,
// hmse_gzip_measure).  Decoding is hmse_l1_inflate's and the CRC-32 hmse_crc32's; what a gzip file does not say is where its members are:
// a member's end is known only after its stream has been walked, so a sequential reader is serial over the whole file.  Here:
//   (1) candidates_*_kernel — every position that could start a member (1f 8b 08 and no reserved FLG bit, 20 bytes of room), in ascending
//                           order: two passes over tiles of GZ_TILE positions (count, block-sum scan of blockops.h, compact).  One 16-byte
//                           load and one 4-byte test per position.
//   (2) measure_kernel    — one wavefront per candidate, persistent wavefronts pulling candidates in index order: the header by RFC 1952;
//                           then either the BGZF fast path (the header says how long the block is: nothing is decoded) or a walk of the
//                           DEFLATE stream FOR ITS LENGTH ONLY: ifl::walk_stream of inflate_core.h, the very walk ifl::l1_inflate_kernel
//                           decodes with and so every validity rule of it, here with a sink that counts — no store, no window.
// A candidate inside compressed data is measured like any other and comes out invalid or with some end; the caller follows the ends from
// offset 0 (hmse_amd/gunzip.py), and only real ends lead to the next member.
// The CONVERGENCE RULE of l1_inflate.hip holds in measure_kernel: every loop has a wave-uniform trip count, every value that steers control
// flow is scalar (uni32 / uni64 / a ballot), results are stored by all lanes (same address, same value), no lane-dependent branch stands
// at a loop tail.
#include "common.h"
#include "../../include/hmse_gunzip.h"
#include "blockops.h"
#include "inflate_core.h"

constexpr int GZ_NT = 256;                            // threads per workgroup of both kernels
constexpr int GZ_PER = 16;                            // positions per thread and trip: one 16-byte load
constexpr int GZ_TRIPS = 4;
constexpr int GZ_TILE = GZ_NT * GZ_PER * GZ_TRIPS;    // positions per workgroup: 16 KiB
constexpr int GZ_SCAN_NT = 1024;
constexpr uint32_t GZ_MIN_MEMBER = 20;                // 10 header bytes, the 2-byte empty fixed block, 8 trailer bytes
constexpr uint32_t GZ_POLY = 0xEDB88320u;

namespace gz {

// bit j = position p0 + j starts with 1f 8b 08 and a FLG byte without reserved bits, and has GZ_MIN_MEMBER bytes of room.
// Reads data[p0, p0 + 20) and only if that lies inside data.
__device__ __forceinline__ uint32_t cand_mask(const uint8_t* __restrict__ data, uint64_t n, uint64_t p0) {
  if (p0 + GZ_MIN_MEMBER > n) return 0u;              // not even position p0 has room
  const uint64_t left = n - GZ_MIN_MEMBER - p0;       // positions behind p0 that have room as well
  const uint32_t room = left >= GZ_PER - 1 ? (uint32_t)GZ_PER : (uint32_t)left + 1u;
  const uint4 v = load_u4_unaligned(data + p0);       // p0 + 20 <= n: these 20 bytes exist
  const uint32_t w[5] = {v.x, v.y, v.z, v.w, load_u32_unaligned(data + p0 + 16)};
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < GZ_PER; j++) {
    const uint32_t x = __builtin_amdgcn_alignbyte(w[j / 4 + 1], w[j / 4], (uint32_t)(j & 3));
    m |= ((x & 0xE0FFFFFFu) == 0x00088B1Fu ? 1u : 0u) << j;
  }
  return room >= GZ_PER ? m : m & ((1u << room) - 1u);
}

// pass 1: candidates per tile
__global__ __launch_bounds__(GZ_NT) void candidates_count_kernel(const uint8_t* __restrict__ data, uint64_t n, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t s_red[GZ_NT / 64 + 1];
  const uint64_t base = (uint64_t)blockIdx.x * GZ_TILE + (uint64_t)threadIdx.x * GZ_PER;
  uint32_t c = 0;
#pragma unroll
  for (int it = 0; it < GZ_TRIPS; it++) c += (uint32_t)__builtin_popcount(cand_mask(data, n, base + (uint64_t)it * (GZ_NT * GZ_PER)));
  uint32_t tot;
  block_exclusive_scan<GZ_NT>(c, s_red, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// pass 2: bsum holds the candidates in front of every tile, *count their number; positions in ascending order, none beyond cap
__global__ __launch_bounds__(GZ_NT) void candidates_compact_kernel(const uint8_t* __restrict__ data, uint64_t n, const uint32_t* __restrict__ bsum,
                                                                   uint64_t* __restrict__ cand_off, uint64_t cap, const uint64_t* __restrict__ count,
                                                                   uint32_t* status) {
  __shared__ uint32_t s_red[GZ_NT / 64 + 1];
  if (blockIdx.x == 0 && threadIdx.x == 0 && *count > cap) atomicOr(status, 1u);
  const uint64_t base = (uint64_t)blockIdx.x * GZ_TILE + (uint64_t)threadIdx.x * GZ_PER;
  uint64_t at = bsum[blockIdx.x];
  for (int it = 0; it < GZ_TRIPS; it++) {
    const uint64_t p0 = base + (uint64_t)it * (GZ_NT * GZ_PER);
    uint32_t m = cand_mask(data, n, p0);
    uint32_t tot;
    uint64_t o = at + block_exclusive_scan<GZ_NT>((uint32_t)__builtin_popcount(m), s_red, &tot);
    for (; m; m &= m - 1u, o++)
      if (o < cap) cand_off[o] = p0 + (uint32_t)__builtin_ctz(m);
    at += tot;
  }
}

// ---- one candidate per wavefront ------------------------------------------------------------------------------------------------------
struct MeasureArgs {
  const uint8_t* data; uint64_t n; const uint64_t* cand_off; uint32_t n_cand;
  uint64_t* stream_off; uint64_t* end; uint64_t* raw_len; uint32_t* crc; uint32_t* flags; uint32_t* counter;
};

// a byte / little-endian u16 / u32 at a wave-uniform address, scalar; the caller has checked the bounds
__device__ __forceinline__ uint32_t ub(const uint8_t* d, uint64_t i) { return uni32(d[i]); }
__device__ __forceinline__ uint32_t u16le(const uint8_t* d, uint64_t i) { return ub(d, i) | (ub(d, i + 1) << 8); }
__device__ __forceinline__ uint32_t u32le(const uint8_t* d, uint64_t i) { return uni32(load_u32_unaligned(d + i)); }

// the end of a zero-terminated field that starts at q: 64 bytes per step.  -> the byte behind the zero, or 0 if none lies inside data
__device__ __forceinline__ uint64_t skip_zstring(const uint8_t* d, uint64_t n, uint64_t q, uint32_t lane) {
  while (q < n) {
    const uint64_t i = q + lane;
    const uint64_t m = __ballot(i < n && d[i] == 0);
    if (m) return q + (uint32_t)__builtin_ctzll(m) + 1u;
    q += 64;
  }
  return 0;
}

// CRC-32 of data[a, b), 64 bytes per load, byte-serial through a uniform readlane: headers are short
__device__ __forceinline__ uint32_t header_crc(const uint8_t* d, uint64_t a, uint64_t b, uint32_t lane) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint64_t b0 = a; b0 < b; b0 += 64) {
    const uint64_t i = b0 + lane;
    const uint32_t v = i < b ? d[i] : 0u;
    const uint32_t m = b - b0 < 64 ? (uint32_t)(b - b0) : 64u;
    for (uint32_t j = 0; j < m; j++) {
      c ^= (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j);
#pragma unroll
      for (int k = 0; k < 8; k++) c = (c >> 1) ^ (GZ_POLY & (0u - (c & 1u)));
    }
  }
  return ~c;
}

// The Sink of ifl::walk_stream (inflate_core.h) that measures: nothing is stored and there is no window, so a stored block of any length
// fits and the one refusal is a match that starts in front of the stream.
struct CountSink {
  uint64_t pos;                                        // bytes the stream has decoded to so far
  __device__ __forceinline__ bool fits(uint32_t) const { return true; }
  __device__ __forceinline__ void stored(const uint8_t*, uint32_t len) { pos += len; }
  __device__ __forceinline__ bool literal(uint32_t) { pos++; return true; }
  __device__ __forceinline__ bool match(uint32_t len, uint32_t dist) { if (dist > pos) return false; pos += len; return true; }
  __device__ __forceinline__ void trace(uint32_t) const {}
};

__global__ __launch_bounds__(GZ_NT, 8) void measure_kernel(MeasureArgs a) {
  __shared__ ifl::WaveTables s_tab[GZ_NT / 64];
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  ifl::WaveTables& T = s_tab[wave];
  const uint8_t* const d = a.data;
  const uint64_t n = a.n;
  for (;;) {
    // one pull per wavefront, every lane taking part (see ifl::l1_inflate_kernel)
    const uint32_t k = uni32(atomicAdd(a.counter, lane == 0 ? 1u : 0u));
    if (k >= a.n_cand) break;
    const uint64_t p = uni64(a.cand_off[k]);
    uint32_t why = 0;                                  // HMSE_GZIP_WHY_*: 0 = valid so far
    uint32_t bgzf = 0;
    uint64_t q = p, m_end = p, m_raw = 0;
    uint32_t m_crc = 0;
    // ---- header (RFC 1952) ----
    uint32_t flg = 0;
    if (p > n || n - p < GZ_MIN_MEMBER) why = HMSE_GZIP_WHY_BOUNDS;
    else {
      const uint32_t w0 = u32le(d, p);
      if ((w0 & 0xE0FFFFFFu) != 0x00088B1Fu) why = HMSE_GZIP_WHY_HEADER;
      flg = w0 >> 24;
      q = p + 10;
    }
    uint32_t bsize1 = 0;                               // BSIZE + 1 of a BC subfield, 0 = none
    if (!why && (flg & 4u)) {                          // FEXTRA
      const uint32_t xlen = u16le(d, q);               // (q + 2 <= p + 20 <= n)
      const uint64_t x0 = q + 2, x1 = x0 + xlen;
      if (x1 > n) why = HMSE_GZIP_WHY_BOUNDS;
      else {
        // subfields SI1 SI2 SLEN(u16) data: at most xlen / 4 of them; zlib does not look inside, so a broken list only ends the search
        uint64_t s = x0;
        while (s + 4 <= x1) {
          const uint32_t id = u16le(d, s), slen = u16le(d, s + 2);
          if (id == 0x4342u && slen == 2u && s + 6 <= x1 && bsize1 == 0) bsize1 = u16le(d, s + 4) + 1u;
          s += 4ull + slen;
        }
        q = x1;
      }
    }
    if (!why && (flg & 8u)) { q = skip_zstring(d, n, q, lane); if (q == 0) { why = HMSE_GZIP_WHY_BOUNDS; q = p; } }     // FNAME
    if (!why && (flg & 16u)) { q = skip_zstring(d, n, q, lane); if (q == 0) { why = HMSE_GZIP_WHY_BOUNDS; q = p; } }    // FCOMMENT
    if (!why && (flg & 2u)) {                          // FHCRC: the low 16 bits of the CRC-32 of the header in front of it
      if (n - q < 2) why = HMSE_GZIP_WHY_BOUNDS;
      else {
        if ((header_crc(d, p, q, lane) & 0xFFFFu) != u16le(d, q)) why = HMSE_GZIP_WHY_HEADER;
        q += 2;
      }
    }
    // ---- BGZF: the header says where the block ends ----
    if (!why && bsize1 != 0 && bsize1 >= (q - p) + 2 + 8 && n - p >= bsize1) {
      const uint32_t isize = u32le(d, p + bsize1 - 4);
      if (isize <= 65536u) { bgzf = 1; m_end = p + bsize1; m_raw = isize; m_crc = u32le(d, p + bsize1 - 8); }
    }
    // ---- any other member: walk the stream for its length ----
    if (!why && !bgzf) {
      CountSink sk; sk.pos = 0;
      uint64_t s_end;                                  // the byte after the final block's last bit
      const bool walked = ifl::walk_stream(d, q, n, T, sk, s_end);
      if (!walked) why = HMSE_GZIP_WHY_STREAM;
      else if (s_end > n || n - s_end < 8) why = HMSE_GZIP_WHY_BOUNDS;
      else if (sk.pos > 0xFFFFFFFFull || s_end - q > 0xFFFFFFFFull || (uint32_t)sk.pos != u32le(d, s_end + 4)) why = HMSE_GZIP_WHY_LENGTH;
      else { m_end = s_end + 8; m_raw = sk.pos; m_crc = u32le(d, s_end); }
    }
    // every lane stores the same words (the convergence rule)
    a.stream_off[k] = q;
    a.end[k] = why ? p : m_end;
    a.raw_len[k] = why ? 0 : m_raw;
    a.crc[k] = why ? 0u : m_crc;
    a.flags[k] = why ? why << HMSE_GZIP_WHY_SHIFT : (HMSE_GZIP_VALID | (bgzf ? HMSE_GZIP_FAST : 0u));
  }
}

}  // namespace gz

// ---- entry points -------------------------------------------------------------------------------------------------------------
static inline uint64_t gz_tiles(uint64_t n) { return n < GZ_MIN_MEMBER ? 0 : hmse_blocks(n - GZ_MIN_MEMBER + 1, GZ_TILE); }

// candidates: u32 per tile and one more (256-byte pieces), then the pull counter of hmse_gzip_measure in a piece of its own
extern "C" size_t hmse_gzip_workspace_bytes(uint64_t n) { return hmse_align_up((gz_tiles(n) + 1) * sizeof(uint32_t), 256) + 256; }

extern "C" int hmse_gzip_candidates(const uint8_t* data, uint64_t n, uint64_t* cand_off, uint64_t cap, uint64_t* count, uint32_t* status,
                                    void* ws, size_t ws_bytes, void* stream_) {
  HMSE_WS_ALIGNED(ws);
  hipStream_t stream = (hipStream_t)stream_;
  if (!status || !count || (n && !data) || (cap && !cand_off) || n > (1ull << 40)) return HMSE_EINVAL;
  const uint64_t nb = gz_tiles(n);
  if (nb && (!ws || ws_bytes < hmse_gzip_workspace_bytes(n))) return HMSE_ENOSPC;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(count, 0, 8, stream);
  if (nb == 0) return HMSE_OK;
  uint32_t* bsum = (uint32_t*)ws;
  gz::candidates_count_kernel<<<dim3((uint32_t)nb), dim3(GZ_NT), 0, stream>>>(data, n, bsum);
  HMSE_LAUNCH_CHECK();
  block_sums_scan_kernel<GZ_SCAN_NT><<<dim3(1), dim3(GZ_SCAN_NT), 0, stream>>>(bsum, nb, count, nullptr);
  HMSE_LAUNCH_CHECK();
  gz::candidates_compact_kernel<<<dim3((uint32_t)nb), dim3(GZ_NT), 0, stream>>>(data, n, bsum, cand_off, cap, count, status);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_gzip_measure(const uint8_t* data, uint64_t n, const uint64_t* cand_off, uint64_t n_cand, uint64_t* stream_off, uint64_t* end,
                                 uint64_t* raw_len, uint32_t* crc, uint32_t* flags, uint32_t* status, void* ws, size_t ws_bytes, void* stream_) {
  HMSE_WS_ALIGNED(ws);
  hipStream_t stream = (hipStream_t)stream_;
  if (!status || (n && !data) || n > (1ull << 40) || n_cand > 0x7FFFFFFFull) return HMSE_EINVAL;
  if (n_cand && (!cand_off || !stream_off || !end || !raw_len || !crc || !flags)) return HMSE_EINVAL;
  if (n_cand && (!ws || ws_bytes < hmse_gzip_workspace_bytes(n))) return HMSE_ENOSPC;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n_cand == 0) return HMSE_OK;
  uint32_t* counter = (uint32_t*)((uint8_t*)ws + hmse_gzip_workspace_bytes(n) - 256);
  HMSE_FILL(counter, 0, 256, stream);
  gz::MeasureArgs a;
  a.data = data; a.n = n; a.cand_off = cand_off; a.n_cand = (uint32_t)n_cand;
  a.stream_off = stream_off; a.end = end; a.raw_len = raw_len; a.crc = crc; a.flags = flags; a.counter = counter;
  uint64_t blocks = hmse_blocks(n_cand, GZ_NT / 64);
  if (blocks > 256 * 8) blocks = 256 * 8;             // persistent wavefronts
  gz::measure_kernel<<<dim3((uint32_t)blocks), dim3(GZ_NT), 0, stream>>>(a);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
