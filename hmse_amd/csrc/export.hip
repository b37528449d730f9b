// export.hip — a store leaves the project as multi-member gzip / BGZF (hmse_amd/export.py; include/hmse.h hmse_crc32, hmse_crc32_combine,
// hmse_gzip_members).  The records are raw DEFLATE streams already, so a member is a copy of a stream between a header and a trailer
// of CRC-32 and length; the CRC-32 (zlib's: reflected 0xEDB88320, init and final xor 0xFFFFFFFF) is the one thing that is computed.
//
// Arithmetic.  A register is a polynomial over GF(2) modulo P, reflected: bit 31 is x^0.  ex_mulmod multiplies two of them, EX_X2N holds
// x^(2^k) (k and k + 32 give the same: x^(2^32 - 1) = 1), ex_xpow8(n) = x^(8 n) takes one multiplication per set bit of n.  With
// reg(M) the register after the bytes M from a register of 0:
//   reg(A | B) = reg(A) * x^(8 |B|) ^ reg(B)                 (linearity; the same holds for the finished CRCs: the init terms cancel)
//   crc(M)     = reg(M) ^ 0xFFFFFFFF * x^(8 |M|) ^ 0xFFFFFFFF
// and leading zero bytes leave a register of 0 at 0.
//   (1) crc32_kernel         — one wavefront (= one workgroup) per range.  The range is right-aligned into 64 strips of SS bytes, one
//                              per lane, zeros in front; SS = n_tiles * S with S a multiple of 16 up to EX_SMAX.  Per tile every lane's
//                              next S bytes are staged in LDS by 16-byte pieces (a strip's pieces are contiguous in HBM) at a stride of
//                              S / 4 + 1 dwords — odd, so the strip reads of a step hit 32 banks per 32 lanes — and walked with the
//                              slicing-by-4 tables (LDS, built in the prologue): the same trip count in every lane.  The 64 remainders
//                              meet in 6 levels through LDS, c = c_left * x^(8 SS 2^level) ^ c, the multiplier squared per level.
//   (2) crc32_combine_kernel — one thread per entry: crc[k] * x^(8 * bytes behind k), xor-reduced (xor commutes: no order matters).
//   (3) gzip_members_kernel  — one wavefront per member: header, the record's stream from one of two sources (wave_copy), trailer.
// No kernel holds a cross-lane operation inside a loop at all; barriers stand in loops whose trip counts are wave-uniform.
#include "common.h"
#include "blockops.h"

constexpr int EX_NT = 64;                             // CRC: threads per workgroup — one wavefront
constexpr int EX_SMAX = 128;                          // bytes per lane and tile at most
constexpr int EX_TILE = 64 * EX_SMAX;                 // 8 KiB of a range per tile at most
constexpr int EX_LDS_TILE = 64 * (EX_SMAX / 4 + 1);   // dwords: 64 strips at the padded stride
constexpr int EX_CNT = 256;                           // threads per workgroup of the other kernels
constexpr uint32_t EX_MAX_BLOCKS = 4096;              // CRC: 256 CUs x 16 workgroups; the ranges beyond are reached by the grid stride
constexpr uint32_t EX_POLY = 0xEDB88320u;

// a * b mod P: bit 31 - i of a is the coefficient of x^i; b runs through b * x^i
__host__ __device__ constexpr uint32_t ex_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (EX_POLY & (0u - (b & 1u)));
  }
  return p;
}
struct ExX2n { uint32_t v[32]; };
__host__ __device__ constexpr ExX2n ex_x2n_make() {
  ExX2n t{};
  uint32_t p = 1u << 30;                              // x^1
  for (int k = 0; k < 32; k++) { t.v[k] = p; p = ex_mulmod(p, p); }
  return t;
}
__device__ const ExX2n EX_X2N = ex_x2n_make();        // x^(2^k) mod P
// x^(8 n) mod P
__device__ __forceinline__ uint32_t ex_xpow8(uint64_t n) {
  uint32_t p = 0x80000000u;                           // x^0
  for (uint32_t k = 3; n; n >>= 1, k++)
    if (n & 1) p = ex_mulmod(EX_X2N.v[k & 31u], p);
  return p;
}
__device__ __forceinline__ uint64_t ex_uni64(uint64_t v) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// cuts descending or beyond the n bytes of data: status bit 0, and the kernel behind leaves when it finds it
__global__ __launch_bounds__(EX_CNT) void crc32_validate_kernel(const uint64_t* __restrict__ cuts, uint64_t n_chunks, uint64_t n, uint32_t* status) {
  const uint64_t stride = (uint64_t)gridDim.x * EX_CNT;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * EX_CNT + threadIdx.x; i < n_chunks; i += stride) {
    bad |= cuts[i] > cuts[i + 1];
    if (i == 0) bad |= cuts[n_chunks] > n;
  }
  if (bad) atomicOr(status, 1u);
}

// ---- CRC-32 of many ranges ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EX_NT) void crc32_kernel(const uint8_t* __restrict__ data, const uint64_t* __restrict__ cuts, uint64_t n_chunks,
                                                      uint32_t* __restrict__ crc_out, uint32_t* status) {
  __shared__ uint32_t s_tab[4 * 256];                 // slicing-by-4: s_tab[256 j + b] = the register after byte b and j zero bytes
  __shared__ uint32_t s_tile[EX_LDS_TILE];
  __shared__ uint32_t s_c[2][64];
  if (*status & 1u) return;
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint32_t c = t + 64u * j;
    for (int b = 0; b < 8; b++) c = (c >> 1) ^ (EX_POLY & (0u - (c & 1u)));
    s_tab[t + 64u * j] = c;
  }
  __syncthreads();
  for (int lv = 1; lv < 4; lv++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t p = s_tab[256 * (lv - 1) + t + 64u * j];
      s_tab[256 * lv + t + 64u * j] = (p >> 8) ^ s_tab[p & 0xFFu];
    }
    __syncthreads();
  }

  for (uint64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
    const uint64_t start = ex_uni64(cuts[k]), len = ex_uni64(cuts[k + 1]) - start;
    if (len == 0) {                                   // (wave-uniform)
      if (t == 63) crc_out[k] = 0;
      continue;
    }
    // ---- geometry: n_tiles tiles of 64 strips of S bytes; lane l owns the padded bytes [l SS, (l + 1) SS), pad zeros in front ----
    const uint64_t n_tiles = (len + EX_TILE - 1) / EX_TILE;
    const uint64_t per = n_tiles == 1 ? (len + 63) >> 6 : (len + 64 * n_tiles - 1) / (64 * n_tiles);       // <= EX_SMAX
    const uint32_t S = ((uint32_t)per + 15u) & ~15u;
    const uint32_t sdw = S >> 2, pps = S >> 4, pstride = sdw + 1;      // dwords and 16-byte pieces per strip; the odd LDS stride
    const uint64_t SS = n_tiles * S, pad = 64 * SS - len;
    const uint8_t* base = data + start;
    const uint32_t q64 = 64u / pps, r64 = 64u % pps, l0 = t / pps, w0 = t % pps;
    uint32_t c = 0;
    for (uint64_t i = 0; i < n_tiles; i++) {
      // ---- stage: piece 64 j + t = 16 bytes of strip l at 16 w; its last byte lies inside the range (l SS + i S + 16 w + 16 <= 64 SS),
      // its first ones may lie in the padding ----
      uint32_t l = l0, w = w0;
      for (uint32_t j = 0; j < pps; j++) {
        const int64_t g = (int64_t)(l * SS + i * S + 16u * w) - (int64_t)pad;
        uint32_t wv[4] = {0, 0, 0, 0};
        if (g >= 0) {
          const uint4 v = load_u4_unaligned(base + g);
          wv[0] = v.x; wv[1] = v.y; wv[2] = v.z; wv[3] = v.w;
        } else if (g > -16) {
          for (int b = 0; b < 16; b++)
            if (g + b >= 0) wv[b >> 2] |= (uint32_t)base[g + b] << (8 * (b & 3));
        }
        const uint32_t pd = l * pstride + 4u * w;
#pragma unroll
        for (int b = 0; b < 4; b++) s_tile[pd + b] = wv[b];
        w += r64; l += q64;
        if (w >= pps) { w -= pps; l++; }
      }
      __syncthreads();
      // ---- walk: sdw steps of four bytes in every lane ----
      const uint32_t* strip = s_tile + t * pstride;
      for (uint32_t d = 0; d < sdw; d++) {
        c ^= strip[d];
        c = s_tab[768 + (c & 0xFFu)] ^ s_tab[512 + ((c >> 8) & 0xFFu)] ^ s_tab[256 + ((c >> 16) & 0xFFu)] ^ s_tab[c >> 24];
      }
      __syncthreads();                                // the next tile overwrites s_tile
    }
    // ---- the 64 remainders: after level lv lane 63 holds the strips 63 - (2 << lv) + 1 .. 63 (lanes below 2^lv - 1 hold junk nobody reads) ----
    uint32_t m = ex_xpow8(SS);
#pragma unroll 1
    for (int lv = 0; lv < 6; lv++) {
      s_c[lv & 1][t] = c;
      __syncthreads();
      c ^= ex_mulmod(s_c[lv & 1][(t - (1u << lv)) & 63u], m);
      m = ex_mulmod(m, m);
    }
    if (t == 63) crc_out[k] = c ^ ex_mulmod(0xFFFFFFFFu, ex_xpow8(len)) ^ 0xFFFFFFFFu;
  }
}

// ---- CRC-32 of a concatenation ----------------------------------------------------------------------------------------------------
// One thread per entry.  The bytes behind entry i: those behind its workgroup's entries (summed by the workgroup: no workspace) plus
// those of the workgroup's later entries.  out is cleared by the entry point.
__global__ __launch_bounds__(EX_CNT) void crc32_combine_kernel(const uint32_t* __restrict__ crc, const uint64_t* __restrict__ len, uint64_t n,
                                                               uint32_t* out) {
  __shared__ uint64_t s_red[EX_CNT / 64 + 1];
  __shared__ uint32_t s_x;
  const uint32_t t = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * EX_CNT + t;
  if (t == 0) s_x = 0;
  uint64_t mine = 0;
  for (uint64_t j = ((uint64_t)blockIdx.x + 1) * EX_CNT + t; j < n; j += EX_CNT) mine += len[j];
  uint64_t behind, inside;
  block_exclusive_scan<EX_CNT>(mine, s_red, &behind);
  const uint64_t v = i < n ? len[i] : 0;
  const uint64_t ex = block_exclusive_scan<EX_CNT>(v, s_red, &inside);
  const uint32_t x = i < n ? ex_mulmod(crc[i], ex_xpow8(behind + (inside - ex - v))) : 0u;
  if (x) atomicXor(&s_x, x);
  __syncthreads();
  if (t == 0 && s_x) atomicXor(out, s_x);
}

// ---- members ----------------------------------------------------------------------------------------------------------------------
// header bytes of a member: 10 (gzip: no name, MTIME 0, XFL 0, OS 255) or 18 (BGZF: FLG.FEXTRA, XLEN 6, 'B' 'C' 2 0, BSIZE = size - 1)
__device__ __forceinline__ uint32_t ex_header_bytes(uint32_t flags) { return (flags & HMSE_GZIP_BGZF) ? 18u : 10u; }

// one thread per member: bit 0 = a member outside its source or the destination, a record that does not exist, a size that is not
// header + stream + 8, a raw length that is no u32; bit 1 = a BGZF member above 65536 bytes
__global__ __launch_bounds__(EX_CNT) void gzip_validate_kernel(uint64_t src0_bytes, uint64_t src1_bytes, const uint64_t* __restrict__ src_off,
                                                               const uint64_t* __restrict__ stream_len, const uint8_t* __restrict__ src_sel,
                                                               const uint64_t* __restrict__ raw_off, uint64_t n_rec,
                                                               const uint64_t* __restrict__ slot, uint64_t n_chunks,
                                                               const uint64_t* __restrict__ member_off, uint32_t flags, uint64_t dst_bytes,
                                                               uint32_t* status) {
  const uint64_t stride = (uint64_t)gridDim.x * EX_CNT;
  const uint64_t H = ex_header_bytes(flags);
  uint32_t bad = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * EX_CNT + threadIdx.x; i < n_chunks; i += stride) {
    const uint64_t r = slot[i], m0 = member_off[i], m1 = member_off[i + 1];
    if (r >= n_rec || m1 < m0 || m1 > dst_bytes) { bad |= 1u; continue; }
    const uint64_t so = src_off[r], sl = stream_len[r], cap = src_sel[r] ? src1_bytes : src0_bytes;
    if (so > cap || sl > cap - so || m1 - m0 != H + sl + 8) bad |= 1u;
    if (raw_off[r] > raw_off[r + 1] || raw_off[r + 1] - raw_off[r] > 0xFFFFFFFFull) bad |= 1u;
    if ((flags & HMSE_GZIP_BGZF) && m1 - m0 > 65536) bad |= 2u;
  }
  if (bad) atomicOr(status, bad);
}

__global__ __launch_bounds__(EX_CNT) void gzip_members_kernel(const uint8_t* __restrict__ src0, const uint8_t* __restrict__ src1,
                                                              const uint64_t* __restrict__ src_off, const uint64_t* __restrict__ stream_len,
                                                              const uint8_t* __restrict__ src_sel, const uint32_t* __restrict__ crc,
                                                              const uint64_t* __restrict__ raw_off, const uint64_t* __restrict__ slot,
                                                              uint64_t n_chunks, const uint64_t* __restrict__ member_off, uint32_t flags,
                                                              uint8_t* __restrict__ dst, uint32_t* status) {
  if (*status) return;                                // refused by gzip_validate_kernel: nothing is written
  const uint64_t i = (uint64_t)blockIdx.x * (EX_CNT / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= n_chunks) return;
  const uint32_t lane = lane_id();
  const uint64_t r = slot[i], m0 = member_off[i], sl = stream_len[r];
  const uint32_t H = ex_header_bytes(flags), bs = (uint32_t)(member_off[i + 1] - m0) - 1u;
  if (lane < H) {
    const bool z = H == 18;
    const uint32_t hb = lane == 0 ? 0x1Fu : lane == 1 ? 0x8Bu : lane == 2 ? 8u : lane == 3 ? (z ? 4u : 0u) : lane == 9 ? 0xFFu : lane == 10 ? 6u
                      : lane == 12 ? 0x42u : lane == 13 ? 0x43u : lane == 14 ? 2u : lane == 16 ? (bs & 0xFFu) : lane == 17 ? ((bs >> 8) & 0xFFu) : 0u;
    dst[m0 + lane] = (uint8_t)hb;
  }
  wave_copy(dst + m0 + H, (src_sel[r] ? src1 : src0) + src_off[r], sl, lane);
  if (lane < 8) {
    const uint32_t word = lane < 4 ? crc[r] : (uint32_t)(raw_off[r + 1] - raw_off[r]);
    dst[m0 + H + sl + lane] = (uint8_t)(word >> (8 * (lane & 3u)));
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
extern "C" int hmse_crc32(const uint8_t* data, uint64_t n, const uint64_t* cuts, uint64_t n_chunks, uint32_t* crc_out, uint32_t* status,
                          void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!status || (n_chunks && (!cuts || !crc_out)) || (n && !data) || n_chunks > (1ull << 40)) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n_chunks == 0) return HMSE_OK;
  uint64_t nb = hmse_blocks(n_chunks, EX_CNT);
  if (nb > EX_MAX_BLOCKS) nb = EX_MAX_BLOCKS;
  crc32_validate_kernel<<<dim3((uint32_t)nb), dim3(EX_CNT), 0, stream>>>(cuts, n_chunks, n, status);
  HMSE_LAUNCH_CHECK();
  const uint32_t grid = (uint32_t)(n_chunks < EX_MAX_BLOCKS ? n_chunks : EX_MAX_BLOCKS);
  PROF_BEGIN(HMSE_STAGE_EXPORT_CRC, stream);
  crc32_kernel<<<dim3(grid), dim3(EX_NT), 0, stream>>>(data, cuts, n_chunks, crc_out, status);
  PROF_END(HMSE_STAGE_EXPORT_CRC, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_crc32_combine(const uint32_t* crc, const uint64_t* len, uint64_t n, uint32_t* out, uint32_t* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!out || !status || (n && (!crc || !len)) || n > (1ull << 32)) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(out, 0, 4, stream);
  if (n == 0) return HMSE_OK;
  crc32_combine_kernel<<<dim3((uint32_t)hmse_blocks(n, EX_CNT)), dim3(EX_CNT), 0, stream>>>(crc, len, n, out);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

extern "C" int hmse_gzip_members(const uint8_t* src0, uint64_t src0_bytes, const uint8_t* src1, uint64_t src1_bytes, const uint64_t* src_off,
                                 const uint64_t* stream_len, const uint8_t* src_sel, const uint32_t* crc, const uint64_t* raw_off,
                                 uint64_t n_rec, const uint64_t* slot, uint64_t n_chunks, const uint64_t* member_off, uint32_t flags,
                                 uint8_t* dst, uint64_t dst_bytes, uint32_t* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!status || (flags & ~(uint32_t)HMSE_GZIP_BGZF)) return HMSE_EINVAL;
  if (n_chunks && (!src_off || !stream_len || !src_sel || !crc || !raw_off || !slot || !member_off || !dst)) return HMSE_EINVAL;
  if ((!src0 && src0_bytes) || (!src1 && src1_bytes) || n_chunks >= (1ull << 33)) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n_chunks == 0) return HMSE_OK;
  uint64_t nb = hmse_blocks(n_chunks, EX_CNT);
  if (nb > EX_MAX_BLOCKS) nb = EX_MAX_BLOCKS;
  gzip_validate_kernel<<<dim3((uint32_t)nb), dim3(EX_CNT), 0, stream>>>(src0_bytes, src1_bytes, src_off, stream_len, src_sel, raw_off, n_rec, slot,
                                                                        n_chunks, member_off, flags, dst_bytes, status);
  HMSE_LAUNCH_CHECK();
  const uint64_t blocks = hmse_blocks(n_chunks, EX_CNT / 64);
  PROF_BEGIN(HMSE_STAGE_EXPORT_MEMBERS, stream);
  gzip_members_kernel<<<dim3((uint32_t)blocks), dim3(EX_CNT), 0, stream>>>(src0, src1, src_off, stream_len, src_sel, crc, raw_off, slot, n_chunks,
                                                                           member_off, flags, dst, status);
  PROF_END(HMSE_STAGE_EXPORT_MEMBERS, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
