// inflate_core.h — what every DEFLATE decoder of this library that runs ONE STREAM PER WAVEFRONT is built on: the scalar bit reader, the
// canonical-code tables built with wave ballots and the one-step symbol decode.  l1_inflate.hip (ifl::l1_inflate_kernel: decodes) and
// gunzip.hip (gz::measure_kernel: walks a stream for its length only) include it after common.h; tools/gunzip_emu.cpp includes it after
// tools/hip_on_cpu.h.  The CONVERGENCE RULE at the top of l1_inflate.hip holds for everything here and for every caller: all state that
// steers control flow is wave-uniform and kept in SGPRs.
#pragma once

namespace ifl {

struct WaveTables {
  uint16_t lsym[288];   // lit/len symbols sorted by (length, symbol)
  uint16_t dsym[32];
  uint8_t lens[320];    // code lengths while a dynamic header is read
};

// bit reader over streams[p, end): 64-bit window, LSB first (RFC 1951 §3.1.1); all state scalar
struct Bits {
  const uint8_t* s; uint64_t p, end; uint64_t acc; uint32_t n;
  __device__ __forceinline__ void refill() {
    if (p + 8 <= end) {  // one unaligned 8-byte load at a uniform address
      uint64_t w;
      __builtin_memcpy(&w, s + p, 8);
      acc |= uni64(w) << n;
      const uint32_t adv = (63u - n) >> 3;
      p += adv; n += adv * 8u;
      return;
    }
    while (n <= 56) {  // last bytes of the stream; zeros behind it (the final length check catches their use)
      uint32_t b = 0;
      if (p < end) b = uni32(s[p]);
      p++;
      acc |= (uint64_t)b << n; n += 8;
    }
  }
  __device__ __forceinline__ uint32_t peek(uint32_t k) const { return (uint32_t)acc & ((1u << k) - 1u); }  // k <= 16
  __device__ __forceinline__ void drop(uint32_t k) { acc >>= k; n -= k; }
  __device__ __forceinline__ uint32_t take(uint32_t k) { if (n < k) refill(); const uint32_t v = peek(k); drop(k); return v; }
};

// Per-lane view of a canonical code: lane l (1..15) owns code length l.
struct LaneCode { uint32_t count, first, offs; };

// Build the canonical decode tables from code lengths lens[0..n): per length the count, first code and offset into
// `sym`, which receives the symbols sorted by (length, symbol).  Returns false for a set stock zlib rejects:
// over-subscribed, or incomplete unless its longest code has length 1 (never allowed for the code-length code).
__device__ bool build_table(const uint8_t* lens, uint32_t n, uint16_t* sym, bool is_codes, LaneCode& lc) {
  const uint32_t lane = lane_id();
  uint32_t mycnt = 0;
  for (uint32_t b = 0; b < n; b += 64) {
    const uint32_t s = b + lane;
    const uint32_t l = s < n ? lens[s] : 0u;
#pragma nounroll
    for (uint32_t k = 1; k < 16; k++) {
      const uint32_t c = (uint32_t)__builtin_popcountll(__ballot(l == k));
      mycnt += lane == k ? c : 0u;
    }
  }
  uint32_t code = 0, off = 0, prevc = 0, maxl = 0, myfirst = 0, myoff = 0;
  int32_t left = 1;
  bool over = false;
#pragma nounroll
  for (uint32_t k = 1; k < 16; k++) {
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)mycnt, (int)k);
    code = (code + prevc) << 1;
    myfirst = lane == k ? code : myfirst;
    myoff = lane == k ? off : myoff;
    off += c; prevc = c;
    left = (left << 1) - (int32_t)c;
    if (left < 0) over = true;
    if (c) maxl = k;
  }
  const bool mine = lane >= 1 && lane <= 15;
  lc.count = mine ? mycnt : 0u; lc.first = myfirst; lc.offs = myoff;
  if (over || (maxl != 0 && left > 0 && (is_codes || maxl != 1))) return false;
  // symbols of equal length keep index order: rank inside the length by ballots
  uint32_t myrun = myoff;
  for (uint32_t b = 0; b < n; b += 64) {
    const uint32_t s = b + lane;
    const uint32_t l = s < n ? lens[s] : 0u;
#pragma nounroll
    for (uint32_t k = 1; k < 16; k++) {
      const uint64_t m = __ballot(l == k);
      if (m == 0) continue;
      const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)myrun, (int)k);
      if (l == k) sym[at + (uint32_t)__builtin_popcountll(m & lanemask_lt())] = (uint16_t)s;
      myrun += lane == k ? (uint32_t)__builtin_popcountll(m) : 0u;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return true;
}

// One symbol in one step: lane l tests whether the next l bits are a code of length l (canonical codes: the l-bit
// value minus the first code of that length indexes the symbols of that length); the shortest hit is the code.
// Returns 0xFFFF on an undefined code.
__device__ __forceinline__ uint32_t decode_sym(Bits& br, const LaneCode& lc, const uint16_t* sym) {
  if (br.n < 15) br.refill();
  const uint32_t l = lane_id() & 15u;
  const uint32_t rev = __builtin_bitreverse32(br.peek(15));                     // first stream bit -> bit 31
  const uint32_t code = l ? rev >> (32u - l) : 0u;                              // first l bits, MSB-first value
  const uint32_t rel = code - lc.first;
  const uint64_t m = __ballot(rel < lc.count);                                  // count is 0 outside lanes 1..15
  if (m == 0) return 0xFFFFu;
  const uint32_t len = (uint32_t)__builtin_ctzll(m);
  const uint32_t idx = (uint32_t)__builtin_amdgcn_readlane((int)(lc.offs + rel), (int)len);
  br.drop(len);
  return uni32(sym[idx]);
}

}  // namespace ifl
