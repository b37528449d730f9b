// inflate_core.h — what every DEFLATE decoder of this library that runs ONE STREAM PER WAVEFRONT is built on: the scalar bit reader, the
// canonical-code tables built with wave ballots, the one-step symbol decode, and walk_stream: the one walk over a stream's blocks and
// symbols, with every validity rule in it.  What a walker does with the bytes is its Sink's: l1_inflate.hip (ifl::l1_inflate_kernel)
// stores them, gunzip.hip (gz::measure_kernel) counts them.  Both include this file after common.h; tools/gunzip_emu.cpp and
// tools/inflate_emu.cpp include it after tools/hip_on_cpu.h.  The CONVERGENCE RULE at the top of l1_inflate.hip holds for everything here
// and for every caller: all state that steers control flow is wave-uniform and kept in SGPRs.
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

// order of the code-length code lengths (RFC 1951 §3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
__device__ __forceinline__ uint32_t cl_order(uint32_t i) { return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? (19 - i) >> 1 : 6 + (i >> 1); }

// The walk over the raw DEFLATE stream s[p, end), from the first block's final bit to the final block's last bit: the decoders' one
// definition of a valid stream (whatever stock zlib accepts).  -> true if the stream was walked to its end, and `stop` = the byte after the
// final block's last bit (whether that is where the stream should end is the caller's to say); false at the first of these refusals:
//    1  more steps than the budget: every block costs >= 3 bits and every symbol >= 1 bit, so 8 * (end - p) + 64 steps is a budget no
//       valid stream exceeds, and a wavefront reaches its exit whatever the bytes are
//    2  block type 3
//    3  a stored block whose NLEN is not ~LEN, that does not fit the sink, or whose bytes end behind the stream
//    4  HLIT > 286 or HDIST > 30
//    5  a code-length code that is over-subscribed or incomplete
//    6  a code-length symbol that is undefined; repeat code 16 with nothing before it; a run that passes HLIT + HDIST lengths
//    7  no end-of-block code
//    8  a literal/length or distance code set that is over-subscribed, or incomplete unless it is one code of length 1
//    9  a literal the sink refuses
//   10  a literal/length symbol above 285 (286, 287, an undefined code)
//   11  a distance symbol above 29 (30, 31, an undefined code; any at all where the set is empty); a match the sink refuses
// A Sink says what becomes of the bytes and how many there may be.  It is called from wave-uniform control flow only and answers with
// wave-uniform values:
//   bool fits(len)            a stored block of len bytes may follow
//   void stored(src, len)     take the len bytes at src (a stored block that fits)
//   bool literal(sym)         take one byte; false = refused
//   bool match(len, dist)     take len bytes from dist bytes back; false = refused
//   void trace(phase)         progress for a diagnostic build: 3 = at a block's header, 6 = at its first symbol
// The bit reader is a local of the walk, and the refusals set a flag and leave their loop rather than return: in both the compiler keeps
// the reader's window in scalar registers without copies at the loop tails, and tools/isa_audit.py sees no exit it takes for divergent
// (DESIGN.md §11.38 has the forms that were measured).
template <class Sink>
__device__ __forceinline__ bool walk_stream(const uint8_t* s, uint64_t p, uint64_t end, WaveTables& T, Sink& sink, uint64_t& stop) {
  const uint32_t lane = lane_id();
  Bits br; br.s = s; br.p = p; br.end = end; br.acc = 0; br.n = 0;
  uint64_t budget = 8ull * (end - p) + 64;
  LaneCode LL{0, 0, 0}, LD{0, 0, 0};
  bool bad = false, last = false;
  while (!bad && !last) {
    if (budget-- == 0) { bad = true; break; }
    sink.trace(3);
    last = br.take(1) != 0;
    const uint32_t type = br.take(2);
    if (type == 0) {  // stored
      br.drop(br.n & 7u);
      const uint32_t len = br.take(16), nlen = br.take(16);
      if ((len ^ nlen) != 0xFFFFu || !sink.fits(len)) { bad = true; break; }
      const uint64_t src = br.p - (br.n >> 3);  // whole bytes still in the window come first
      if (src + len > br.end) { bad = true; break; }
      sink.stored(br.s + src, len);
      br.p = src + len; br.acc = 0; br.n = 0;
      continue;
    }
    if (type == 3) { bad = true; break; }
    if (type == 1) {  // fixed codes
      for (uint32_t s0 = 0; s0 < 320; s0 += 64) {
        const uint32_t s = s0 + lane;
        if (s < 288) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      build_table(T.lens, 288, T.lsym, false, LL);
      if (lane < 32) T.lens[lane] = 5;   // 32 five-bit distance codes; 30 and 31 are rejected where they are used
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      build_table(T.lens, 32, T.dsym, false, LD);
    } else {  // dynamic codes
      const uint32_t nlit = br.take(5) + 257, ndist = br.take(5) + 1, ncl = br.take(4) + 4;
      if (nlit > 286 || ndist > 30) { bad = true; break; }
      if (lane < 19) T.lens[lane] = 0;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      for (uint32_t i = 0; i < ncl; i++) {
        const uint32_t v = br.take(3);
        T.lens[cl_order(i)] = (uint8_t)v;  // every lane, same address and value
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      LaneCode LC;
      if (!build_table(T.lens, 19, T.dsym, true, LC)) { bad = true; break; }  // the code-length code borrows dsym
      // the lengths are decoded over lens[0..19), which feeds nothing any more; dsym is read by decode_sym
      uint32_t i = 0, prev = 0;
      const uint32_t tot = nlit + ndist;
      while (i < tot) {
        const uint32_t s = decode_sym(br, LC, T.dsym);
        if (s > 18) { bad = true; break; }
        uint32_t rep = 1, val = s;
        if (s == 16) { if (i == 0) { bad = true; break; } rep = 3 + br.take(2); val = prev; }
        else if (s == 17) { rep = 3 + br.take(3); val = 0; }
        else if (s == 18) { rep = 11 + br.take(7); val = 0; }
        if (i + rep > tot) { bad = true; break; }
        for (uint32_t j0 = 0; j0 < rep; j0 += 64) {
          const uint32_t j = j0 + lane;
          if (j < rep) T.lens[i + j] = (uint8_t)val;
        }
        i += rep; prev = val;
      }
      if (bad) break;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      if (uni32(T.lens[256]) == 0) { bad = true; break; }  // no end-of-block code
      if (!build_table(T.lens, nlit, T.lsym, false, LL)) { bad = true; break; }
      if (!build_table(T.lens + nlit, ndist, T.dsym, false, LD)) { bad = true; break; }
    }
    sink.trace(6);
    // ---- symbols of this block ----
    for (;;) {
      if (budget-- == 0) { bad = true; break; }
      const uint32_t s = decode_sym(br, LL, T.lsym);
      if (s < 256) {
        if (!sink.literal(s)) { bad = true; break; }
        continue;
      }
      if (s == 256) break;
      if (s > 285) { bad = true; break; }  // 286, 287 and the undefined-code marker 0xFFFF
      // length and distance (RFC 1951 §3.2.5)
      const uint32_t lc = s - 257;
      uint32_t len;
      if (lc < 8) len = 3 + lc;
      else if (lc == 28) len = 258;
      else { const uint32_t e = (lc - 4) >> 2; len = 3 + ((4 + (lc & 3)) << e) + br.take(e); }
      const uint32_t ds = decode_sym(br, LD, T.dsym);
      if (ds > 29) { bad = true; break; }
      uint32_t dist;
      if (ds < 4) dist = 1 + ds;
      else { const uint32_t e = (ds >> 1) - 1; dist = 1 + ((2 + (ds & 1)) << e) + br.take(e); }
      if (!sink.match(len, dist)) { bad = true; break; }
    }
  }
  stop = br.p - (br.n >> 3);
  return !bad;
}

}  // namespace ifl
