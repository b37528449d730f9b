// regex_core.h — the kernels and entry-point bodies of the regular-expression search over the decoded records of a store, once for both
// forms: the PLAIN one (regex.hip: hmse_regex_*, include/hmse.h) and the ASSERTING one (regexa.hip: hmse_regexa_*, include/hmse_regexa.h, ^ $
// \A \Z \b \B).  A bounded DFA walk; hmse_amd/regex.py compiles the automaton on the host, hmse_amd/find.py StoreFinder.find_regex picks
// the entry points by Regex.asserting.
//
// Replaces the detour read_store -> host -> re.finditer, which decodes and scans every duplicate chunk once per occurrence.  As for
// the literal search (find.hip) a record is looked at once and hmse_find_place (place_kernel<8>, chunkmap.h) lays its hits out at every
// chunk that maps to it:
//   (1) *_scan_kernel  — per workgroup the transition table (up to 32 KiB) and the class map go to LDS once; per tile of RX_TILE
//                        bytes (+ RX_OVER of overhang) every raw byte is read from HBM once, in 16-byte pieces, translated to its
//                        byte class on the way into LDS, and the first-step filter (does this byte leave the start state alive?)
//                        comes out of the same lookup.  The survivors go into an LDS work list through block_exclusive_scan and
//                        are handed out round-robin, so every lane walks the same number of them whatever strip they came from;
//                        a walk reads classes and transitions from LDS only, runs at most `reach` steps and stops at state 0.
//                        Only SCAN starts are answered: raw_off[r + 1] - p >= reach (the answer then depends on the record only).
//                        The hits of a tile are emitted with ONE reservation per workgroup;
//   (2) *_seams_kernel — the last reach - 1 starts of every chunk, walked through the chunk map.
// The plain form answers a start from the record's bytes behind it.  An assertion also looks one byte BEHIND the start and one byte AHEAD
// of the match, and for a deduplicated record those differ from place to place.  So in the asserting form the partition moves by one
// byte at either end, and the automaton takes the context in: four start states, chosen by the KIND of the previous byte (EDGE, NL,
// WORD, OTHER), and an accept flag on the transition that says "a match may end just before this byte" (include/hmse_regexa.h has the
// compiled form).  There
//   (1) per byte VALUE one LDS entry holds class | 4 survival bits (does the start state of kind a survive this byte?) | the byte's own
//       kind.  On the way into LDS a position survives iff the bit of its predecessor's kind is set; the predecessor of a piece's first
//       byte is raw[g - 1].  The work list keeps the start kind beside the offset.  A walk runs reach + 1 reads: the last one is
//       look-ahead only.  Scan starts: p > raw_off[r] and raw_off[r + 1] - p > reach — the byte in front, the match and the look-ahead
//       byte lie in the record, and inside the staged bytes: a start at the tile's last position reads RX_TILE - 1 + reach <= RX_TILE +
//       255, the last staged byte;
//   (2) the seams are the first start of every chunk and its last `reach` ones, both context bytes fetched through the chunk map
//       (C[o - 1]: the last byte of the nearest non-empty chunk in front; EDGE at 0 and at N).
// No kernel holds an atomic, a barrier or a cross-lane operation inside a loop that lanes leave at different times (tools/isa_audit.py).
//
// One algorithm with a compile-time switch.  The including file sets, in front of the #include,
//   constexpr bool RX_A       — the asserting form or the plain one; every difference below is behind it, stated where it branches;
//   using RxX, RxHeader       — RxDev and hmse_regex, or RxaDev and hmse_regexa;
//   #define RX_KERNEL(name)   — the kernels' names: regex_##name or regexa_##name.
// A discarded `if constexpr` branch of a non-template still compiles, so what only one form HAS (RxaDev::start) is reached through an
// overload.  regex.hip and regexa.hip include this after common.h, include/hmse_regexa.h and chunkmap.h; tools/regex_emu.cpp includes it
// after tools/hip_on_cpu.h and chunkmap.h, so the device part uses only what both provide and the file includes nothing.  It is included
// once per translation unit, and the two translation units link into two libraries.
#pragma once

constexpr int RX_NT = 256;                            // threads per workgroup
constexpr int RX_STRIP = 32;                          // S: bytes per lane and tile (two 16-byte pieces)
constexpr int RX_TILE = RX_NT * RX_STRIP;             // T: 8 KiB of records per workgroup and trip
constexpr int RX_OVER = 256;                          // staged behind the tile: 255 bytes of overhang and the look-ahead byte of a 256-byte match
constexpr int RX_PIECES = (RX_TILE + RX_OVER) / 16;   // 16-byte pieces per tile
constexpr int RX_ROUNDS = RX_TILE / RX_NT;            // survivors per lane at the most (every position of the tile survives)
constexpr uint32_t RX_MAX_BLOCKS = 512;               // 256 CUs x 2 workgroups (LDS); the tiles beyond are reached by the grid stride
static_assert(RX_NT == 256, "one thread per byte value where the class map is staged and checked");
static_assert(RX_TILE <= 8192, "a work-list entry is the offset in the tile (13 bits) | the start kind << 13");
static_assert(RX_OVER >= HMSE_REGEX_MAX_LEN, "the look-ahead byte of the longest match from the tile's last position is staged");

// The automaton's header, handed to the kernels by value: plain, asserting.
struct RxDev { const uint16_t* table; const uint8_t* classmap; uint32_t n_states, n_classes, reach; };
struct RxaDev { const uint16_t* table; const uint8_t* classmap; uint32_t n_states, n_classes, reach, start[4]; };

// the start state by the kind a of the byte in front (asserting); the plain form starts in state 1
__device__ __forceinline__ uint32_t rx_start(const RxDev&, int) { return 1u; }
__device__ __forceinline__ uint32_t rx_start(const RxaDev& X, int a) { return X.start[a]; }

// EDGE = 0 is no byte's kind
__device__ __forceinline__ uint32_t rxa_kind(uint32_t b) {
  if (b == 0x0Au) return HMSE_REGEXA_NL;
  const bool word = (b - '0') < 10u || ((b | 0x20u) - 'a') < 26u || b == '_';
  return word ? HMSE_REGEXA_WORD : HMSE_REGEXA_OTHER;
}

// the sum of v over the workgroup, in every thread (s_sum: RX_NT entries)
__device__ __forceinline__ unsigned long long rx_block_sum(unsigned long long v, unsigned long long* s_sum) {
  const uint32_t t = threadIdx.x;
  s_sum[t] = v;
  __syncthreads();
  if (t < 16) {
    unsigned long long a = 0;
    for (int i = 0; i < RX_NT / 16; i++) a += s_sum[t + 16 * i];
    s_sum[t] = a;
  }
  __syncthreads();
  unsigned long long a = 0;
  for (int i = 0; i < 16; i++) a += s_sum[i];
  __syncthreads();
  return a;
}

// ---- tables and automaton -----------------------------------------------------------------------------------------------------
// status bit 1: tables that break a rule of chunkmap.h (tables_bad_at).  status bit 2: a bad automaton — a table entry whose low 15 bits
// are >= n_states, a non-zero dead row; plain: a classmap value >= n_classes; asserting: a non-zero next state in the EDGE column, a byte
// mapped to the EDGE class or beyond, a class that holds bytes of two kinds.  Every later kernel of the call leaves when it finds either bit.
__global__ __launch_bounds__(RX_NT) void RX_KERNEL(validate_kernel)(const uint64_t* __restrict__ raw_off, uint64_t n_rec, uint64_t raw_bytes,
                                                                    const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                                    uint64_t n_chunks, RxX X, uint64_t n, uint32_t* status) {
  const uint64_t stride = (uint64_t)gridDim.x * RX_NT;
  const uint64_t n_tab = (uint64_t)X.n_states * X.n_classes;
  bool bad = false, bad_rx = false;
  if constexpr (RX_A) {                               // asserting: the class map is checked by workgroup 0, with the kinds
    if (blockIdx.x == 0) {                            // one byte value per thread (RX_NT = 256): the kinds met in every class
      __shared__ uint32_t s_kinds[256];
      const uint32_t c = X.classmap[threadIdx.x];
      s_kinds[threadIdx.x] = 0;
      __syncthreads();
      atomicOr(&s_kinds[c], 1u << rxa_kind(threadIdx.x));
      __syncthreads();
      bad_rx = c >= X.n_classes - 1 || (s_kinds[c] & (s_kinds[c] - 1)) != 0;
    }
  }
  for (uint64_t i = (uint64_t)blockIdx.x * RX_NT + threadIdx.x; i < n; i += stride) {
    bad |= tables_bad_at(i, raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, nullptr);
    if (i < n_tab) {
      const uint32_t e = X.table[i];
      bad_rx |= (e & 0x7FFFu) >= X.n_states || (i < X.n_classes && e != 0);
      if constexpr (RX_A) bad_rx |= ((uint32_t)i % X.n_classes) == X.n_classes - 1 && (e & 0x7FFFu) != 0;     // (i < n_tab <= HMSE_REGEX_MAX_TABLE)
    }
    if constexpr (!RX_A) {                            // plain: the class map is checked in the same pass
      if (i < 256) bad_rx |= X.classmap[i] >= X.n_classes;
    }
  }
  if (bad) atomicOr(status, 2u);
  if (bad_rx) atomicOr(status, 4u);
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_NT) void RX_KERNEL(scan_kernel)(const uint8_t* __restrict__ raw, uint64_t raw_bytes, const uint64_t* __restrict__ raw_off,
                                                                uint64_t n_rec, const uint32_t* __restrict__ mult, RxX X,
                                                                unsigned long long* __restrict__ hits, uint64_t hits_cap, unsigned long long* n_hits,
                                                                unsigned long long* count, uint32_t* status, uint64_t n_tiles) {
  __shared__ uint16_t s_tab[HMSE_REGEX_MAX_TABLE];    // the transition table
  __shared__ uint16_t s_cmx[256];                     // per byte value: its class | 0x100 iff the start state survives it
                                                      //   (asserting: | 0x100 << a iff start[a] survives it | its kind << 12)
  __shared__ __attribute__((aligned(16))) uint8_t s_cls[RX_TILE + RX_OVER];   // the tile, its overhang and the look-ahead byte, as byte classes
  __shared__ uint16_t s_work[RX_TILE];                // the survivors' offsets in the tile (asserting: | the kind of the byte in front << 13)
  __shared__ unsigned long long s_sum[RX_NT];
  __shared__ uint32_t s_red[RX_NT / 64 + 1];
  __shared__ unsigned long long s_base;
  __shared__ uint64_t s_rec[2];                       // the records of the tile's first and last byte
  __shared__ uint32_t s_start[4];                     // (asserting only)

  if (*status & 6u) return;                           // inconsistent tables or a bad automaton (*_validate_kernel)
  const uint32_t t = threadIdx.x;
  const uint32_t nc = X.n_classes, reach = X.reach;
  for (uint32_t i = t; i < X.n_states * nc; i += RX_NT) s_tab[i] = X.table[i];
  if (RX_A && t == 0) { s_start[0] = rx_start(X, 0); s_start[1] = rx_start(X, 1); s_start[2] = rx_start(X, 2); s_start[3] = rx_start(X, 3); }
  __syncthreads();
  {
    const uint32_t c = X.classmap[t];
    if constexpr (RX_A) {                             // one survival bit per start state, and the byte's kind
      uint32_t x = c | (rxa_kind(t) << 12);
#pragma unroll
      for (int a = 0; a < 4; a++) x |= (s_tab[s_start[a] * nc + c] & 0x7FFFu) ? (0x100u << a) : 0u;
      s_cmx[t] = (uint16_t)x;
    } else {
      s_cmx[t] = (uint16_t)(c | ((s_tab[nc + c] & 0x7FFFu) ? 0x100u : 0u));
    }
  }
  __syncthreads();

  const uint64_t lo = raw_off[0], hi = raw_off[n_rec];              // the records cover [lo, hi) of raw
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t g0 = tile * (uint64_t)RX_TILE;
    if (t < 2) {
      const uint64_t last = g0 + RX_TILE - 1 < hi ? g0 + RX_TILE - 1 : hi;
      s_rec[t] = last_le(raw_off, 0, n_rec, t == 0 ? (g0 > lo ? g0 : lo) : last);
    }
    // ---- stage and filter: piece q of the tile = 16 bytes from HBM -> 16 classes in LDS; bit i of surv = byte i may start a match
    //      (asserting: behind ITS predecessor, whose kind goes into kinds, 2 bits per byte, for the work list) ----
    uint32_t surv = 0;                                // bits 0..15: piece t, bits 16..31: piece t + RX_NT
    uint32_t kinds[RX_STRIP / 16] = {0, 0};
#pragma unroll
    for (int j = 0; j < (RX_PIECES + RX_NT - 1) / RX_NT; j++) {
      const uint32_t q = t + j * RX_NT;
      if (q < RX_PIECES) {
        const uint64_t g = g0 + 16ull * q;
        uint8_t b[16];
        if (g + 16 <= raw_bytes) { const uint4 v = load_u4_unaligned(raw + g); __builtin_memcpy(b, &v, 16); }
        else { for (int i = 0; i < 16; i++) b[i] = (g + i < raw_bytes) ? raw[g + i] : (uint8_t)0; }
        // asserting: the filter is keyed on the predecessor's kind.  The kind in front of the piece: raw[g - 1] (g = 0 and positions at
        // or behind raw_bytes start nothing: any kind serves)
        uint32_t a = HMSE_REGEXA_OTHER;
        if constexpr (RX_A) a = (j < RX_STRIP / 16 && g > 0 && g <= raw_bytes) ? (uint32_t)s_cmx[raw[g - 1]] >> 12 : HMSE_REGEXA_OTHER;
        uint32_t w[4] = {0, 0, 0, 0}, m = 0, kk = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const uint32_t x = s_cmx[b[i]];
          w[i >> 2] |= (x & 0xFFu) << (8 * (i & 3));
          if constexpr (RX_A) {
            m |= ((x >> (8 + a)) & 1u) << i;
            kk |= a << (2 * i);
            a = x >> 12;
          } else {
            m |= (x >> 8) << i;
          }
        }
        *(uint4*)(s_cls + 16u * q) = make_uint4(w[0], w[1], w[2], w[3]);
        if (j < RX_STRIP / 16) {                      // (the overhang's positions belong to the next tile)
          if constexpr (RX_A) {
            // a record's first byte is no scan start, so neither is position lo; the walk checks the other records' first bytes
            if (g <= lo) m = (lo - g >= 15) ? 0u : (m & (0xFFFEu << (uint32_t)(lo - g)) & 0xFFFFu);
          } else {
            if (g < lo) m = (lo - g >= 16) ? 0u : (m & (0xFFFFu << (uint32_t)(lo - g)) & 0xFFFFu);
          }
          if (g + 16 > hi) m = (g >= hi) ? 0u : (m & (0xFFFFu >> (uint32_t)(g + 16 - hi)));
          surv |= m << (16 * j);
          kinds[j] = kk;
        }
      }
    }
    // ---- the work list: the survivors of the whole tile, in lane order ----
    uint32_t n_work;
    uint32_t wp = block_exclusive_scan<RX_NT>((uint32_t)__builtin_popcount(surv), s_red, &n_work);
    n_work = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_work);
    for (uint32_t m = surv; m; m &= m - 1) {
      const uint32_t b = (uint32_t)__builtin_ctz(m);
      if constexpr (RX_A) {                           // the entry carries the start kind in its three high bits
        const uint32_t a = (kinds[b >> 4] >> (2 * (b & 15u))) & 3u;
        s_work[wp++] = (uint16_t)((((b >> 4) * RX_NT + t) * 16u + (b & 15u)) | (a << 13));
      } else {
        s_work[wp++] = (uint16_t)(((b >> 4) * RX_NT + t) * 16u + (b & 15u));
      }
    }
    __syncthreads();                                  // s_cls, s_work and s_rec are complete

    // ---- walk: survivor t, t + RX_NT, ... — the same number for every lane; results stay in registers until the tile's reservation ----
    const uint64_t r_first = s_rec[0], r_last = s_rec[1];
    uint32_t got = 0;                                 // bit i: the lane's i-th survivor is a hit
    uint32_t len[RX_ROUNDS / 4];                      // its length - 1, a byte each
#pragma unroll
    for (int i = 0; i < RX_ROUNDS / 4; i++) len[i] = 0;
    unsigned long long weight = 0;
#pragma unroll
    for (int i = 0; i < RX_ROUNDS; i++) {
      const uint32_t k = t + (uint32_t)i * RX_NT;
      if (k < n_work) {
        const uint32_t off = RX_A ? s_work[k] & 0x1FFFu : s_work[k], a = s_work[k] >> 13;
        const uint64_t p = g0 + off;
        const uint64_t r = last_le(raw_off, r_first, r_last + 1, p);
        // a scan start: the walk stays inside record r (and inside the staged bytes).  Asserting: both ends move by one byte, so that
        // raw[p - 1] .. raw[p + reach] lie in record r (and are staged)
        if (RX_A ? p > raw_off[r] && raw_off[r + 1] - p > reach : raw_off[r + 1] - p >= reach) {
          uint32_t s = RX_A ? s_start[a] : 1u, best = 0;
          for (uint32_t step = 0; RX_A ? step <= reach : step < reach; step++) {     // asserting: reach + 1 reads, the last is look-ahead only
            const uint32_t e = s_tab[s * nc + s_cls[off + step]];
            if constexpr (RX_A) {                     // accept is tested BEFORE the state: a match may end just before this byte
              if (e & HMSE_REGEX_ACCEPT) best = step; //   (step 0: the empty one, no hit)
            }
            s = e & 0x7FFFu;
            if (s == 0) break;
            if constexpr (!RX_A) {
              if (e & HMSE_REGEX_ACCEPT) best = step + 1;
            }
          }
          if (best) {
            got |= 1u << i;
            len[i >> 2] |= (best - 1) << (8 * (i & 3));
            weight += mult ? mult[r] : 1u;
          }
        }
      }
    }

    // ---- emit: one reservation per workgroup and tile ----
    uint32_t total;
    const uint32_t my = block_exclusive_scan<RX_NT>((uint32_t)__builtin_popcount(got), s_red, &total);
    total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
    if (total) {
      const unsigned long long w = rx_block_sum(weight, s_sum);
      if (t == 0) {
        const unsigned long long base = atomicAdd(n_hits, (unsigned long long)total);
        atomicAdd(count, w);
        if (hits_cap && base + total > hits_cap) atomicOr(status, 1u);
        s_base = base;
      }
      __syncthreads();
      uint64_t wr = s_base + my;
#pragma unroll
      for (int i = 0; i < RX_ROUNDS; i++) {
        if ((got >> i) & 1u) {
          if (wr < hits_cap) hits[wr] = ((g0 + (s_work[t + (uint32_t)i * RX_NT] & (RX_A ? 0x1FFFu : 0xFFFFu))) << 8) | ((len[i >> 2] >> (8 * (i & 3))) & 0xFFu);
          wr++;
        }
      }
    }
    __syncthreads();                                  // the next tile overwrites s_cls, s_work, s_rec and s_base
  }
}

// ---- seams --------------------------------------------------------------------------------------------------------------------
// Plain: one thread and trip per (chunk c, distance d = 1 .. reach - 1 of the start from the chunk's end, not beyond its start).  The start
// o = cuts[c + 1] - d is walked through the chunk map, over any number of tiny or empty chunks, at most reach steps and not beyond N.
// Asserting: per (chunk c, d = 0 .. reach).  d >= 1: the start o = cuts[c + 1] - d as above; d = 0: the chunk's first byte, where the
// chunk is longer than reach (else d = its length has it).  The byte in front of o comes through the chunk map — the last byte of the
// nearest non-empty chunk in front, the EDGE at the corpus's start — and so does the walk: reach + 1 reads, the EDGE class at N.
__global__ __launch_bounds__(RX_NT) void RX_KERNEL(seams_kernel)(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off,
                                                                 const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ slot,
                                                                 uint64_t n_chunks, RxX X, unsigned long long* __restrict__ hits, uint64_t hits_cap,
                                                                 unsigned long long* n_hits, unsigned long long* count, uint32_t* status,
                                                                 uint64_t n_threads) {
  __shared__ uint16_t s_tab[HMSE_REGEX_MAX_TABLE];
  __shared__ uint8_t s_cm[256];
  __shared__ uint32_t s_red[RX_NT / 64 + 1];
  __shared__ unsigned long long s_base;
  __shared__ uint32_t s_start[4];                     // (asserting only)
  if (*status & 6u) return;
  const uint32_t t = threadIdx.x;
  const uint32_t nc = X.n_classes, reach = X.reach;
  for (uint32_t i = t; i < X.n_states * nc; i += RX_NT) s_tab[i] = X.table[i];
  s_cm[t] = X.classmap[t];
  if (RX_A && t == 0) { s_start[0] = rx_start(X, 0); s_start[1] = rx_start(X, 1); s_start[2] = rx_start(X, 2); s_start[3] = rx_start(X, 3); }
  __syncthreads();
  const uint32_t span = RX_A ? reach + 1 : reach - 1;
  const uint64_t first = cuts[0], n = cuts[n_chunks];
  for (uint64_t id0 = (uint64_t)blockIdx.x * RX_NT; id0 < n_threads; id0 += (uint64_t)gridDim.x * RX_NT) {
    const uint64_t id = id0 + t;
    uint32_t best = 0;
    uint64_t o = 0;
    if (id < n_threads) {
      const uint64_t c = id / span, d = RX_A ? id % span : id % span + 1;
      const uint64_t c0 = cuts[c], c1 = cuts[c + 1];
      if (RX_A ? (d ? d <= c1 - c0 : c1 - c0 > reach) : d <= c1 - c0) {
        o = (!RX_A || d) ? c1 - d : c0;               // c0 <= o < c1 <= N
        uint64_t k = c;
        if constexpr (RX_A) {
          uint32_t a = HMSE_REGEXA_EDGE;              // the kind of the byte in front of o
          if (o > c0) a = rxa_kind(raw[raw_off[slot[c]] + (o - 1 - c0)]);
          else if (o > first) {                       // some chunk in front of c is not empty
            uint64_t f = c - 1;
            while (f > 0 && cuts[f] == cuts[f + 1]) f--;
            a = rxa_kind(raw[raw_off[slot[f]] + (o - 1 - cuts[f])]);
          }
          uint32_t s = s_start[a];
          for (uint32_t i = 0; i <= reach; i++) {     // the read at i = reach is look-ahead only
            const uint64_t q = o + i;
            uint32_t cl = nc - 1;                     // the EDGE: its column leads to state 0
            if (q < n) {
              while (q >= cuts[k + 1]) k++;           // q < N = cuts[n_chunks]: k stays below n_chunks
              cl = s_cm[raw[raw_off[slot[k]] + (q - cuts[k])]];
            }
            const uint32_t e = s_tab[s * nc + cl];
            if (e & HMSE_REGEX_ACCEPT) best = i;
            s = e & 0x7FFFu;
            if (s == 0) break;
          }
        } else {
          const uint64_t end = n - o < reach ? n : o + reach;       // o < N: at least one step
          uint32_t s = 1;
          for (uint64_t q = o; q < end; q++) {
            while (q >= cuts[k + 1]) k++;             // q < N = cuts[n_chunks]: k stays below n_chunks
            const uint32_t e = s_tab[s * nc + s_cm[raw[raw_off[slot[k]] + (q - cuts[k])]]];
            s = e & 0x7FFFu;
            if (s == 0) break;
            if (e & HMSE_REGEX_ACCEPT) best = (uint32_t)(q - o) + 1;
          }
        }
      }
    }
    uint32_t total;
    const uint32_t my = block_exclusive_scan<RX_NT>(best ? 1u : 0u, s_red, &total);
    total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
    if (total) {
      if (t == 0) {
        const unsigned long long base = atomicAdd(n_hits, (unsigned long long)total);
        atomicAdd(count, (unsigned long long)total);
        if (hits_cap && base + total > hits_cap) atomicOr(status, 1u);
        s_base = base;
      }
      __syncthreads();
      if (best && s_base + my < hits_cap) hits[s_base + my] = (o << 8) | (best - 1);
    }
    __syncthreads();                                  // the next trip overwrites s_base
  }
}

// ---- host side (the libraries only): the bodies of the entry points ----------------------------------------------------------
#ifdef __HIPCC__
static bool rx_starts_ok(const hmse_regex*) { return true; }
static bool rx_starts_ok(const hmse_regexa* rx) {
  for (int a = 0; a < 4; a++)
    if (rx->start[a] < 1 || rx->start[a] >= rx->n_states) return false;
  return true;
}
static RxDev rx_dev(const hmse_regex* rx) { return RxDev{rx->table, rx->classmap, rx->n_states, rx->n_classes, rx->reach}; }
static RxaDev rx_dev(const hmse_regexa* rx) {
  return RxaDev{rx->table, rx->classmap, rx->n_states, rx->n_classes, rx->reach, {rx->start[0], rx->start[1], rx->start[2], rx->start[3]}};
}

static int rx_header(const RxHeader* rx, RxX* X) {
  if (!rx || rx->struct_size != sizeof(RxHeader)) return HMSE_EINVAL;
  // (asserting: the EDGE class is one more)
  if (rx->n_states < 2 || rx->n_states > 32767 || rx->n_classes < (RX_A ? 2u : 1u) || rx->n_classes > 256) return HMSE_EINVAL;
  if ((uint64_t)rx->n_states * rx->n_classes > HMSE_REGEX_MAX_TABLE) return HMSE_EINVAL;
  if (rx->reach < 1 || rx->reach > HMSE_REGEX_MAX_LEN || !rx->table || !rx->classmap) return HMSE_EINVAL;
  if (!rx_starts_ok(rx)) return HMSE_EINVAL;
  *X = rx_dev(rx);
  return HMSE_OK;
}

static int rx_validate(const uint64_t* raw_off, uint64_t n_rec, uint64_t raw_bytes, const uint64_t* cuts, const uint64_t* slot,
                       uint64_t n_chunks, const RxX& X, uint32_t* status, hipStream_t stream) {
  uint64_t n = n_rec > n_chunks ? n_rec : n_chunks;
  const uint64_t n_tab = (uint64_t)X.n_states * X.n_classes;
  if (n < n_tab) n = n_tab;
  if (n < 256) n = 256;
  uint64_t nb = (n + RX_NT - 1) / RX_NT;
  if (nb > RX_MAX_BLOCKS) nb = RX_MAX_BLOCKS;
  RX_KERNEL(validate_kernel)<<<dim3((uint32_t)nb), dim3(RX_NT), 0, stream>>>(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, X, n, status);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

// hmse_regex_scan / hmse_regexa_scan
static int rx_scan(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint32_t* mult, const RxHeader* rx,
                   uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits, uint64_t* count, uint32_t* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RxX X;
  if (rx_header(rx, &X) != HMSE_OK || !n_hits || !count || !status) return HMSE_EINVAL;
  if (n_rec && (!raw_off || (raw_bytes && !raw))) return HMSE_EINVAL;
  if (raw_bytes >= (1ull << 56)) return HMSE_EINVAL;  // a hit is position << 8 | length - 1
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(n_hits, 0, 8, stream);
  HMSE_FILL(count, 0, 8, stream);
  if (n_rec == 0 || raw_bytes == 0) return HMSE_OK;
  if (!hits) hits_cap = 0;
  int rc = rx_validate(raw_off, n_rec, raw_bytes, nullptr, nullptr, 0, X, status, stream);
  if (rc != HMSE_OK) return rc;
  const uint64_t n_tiles = (raw_bytes + RX_TILE - 1) / RX_TILE;
  const dim3 grid((uint32_t)(n_tiles < RX_MAX_BLOCKS ? n_tiles : RX_MAX_BLOCKS)), block(RX_NT);
  PROF_BEGIN(HMSE_STAGE_FIND_SCAN, stream);
  RX_KERNEL(scan_kernel)<<<grid, block, 0, stream>>>(raw, raw_bytes, raw_off, n_rec, mult, X, (unsigned long long*)hits, hits_cap,
                                                     (unsigned long long*)n_hits, (unsigned long long*)count, status, n_tiles);
  PROF_END(HMSE_STAGE_FIND_SCAN, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

// hmse_regex_seams / hmse_regexa_seams
static int rx_seams(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts, const uint64_t* slot,
                    uint64_t n_chunks, const RxHeader* rx, uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits, uint64_t* count,
                    uint32_t* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RxX X;
  if (rx_header(rx, &X) != HMSE_OK || !n_hits || !count || !status) return HMSE_EINVAL;
  if (n_chunks && (!cuts || !slot || !raw_off || !raw)) return HMSE_EINVAL;
  if (n_chunks > (1ull << 40)) return HMSE_EINVAL;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(n_hits, 0, 8, stream);
  HMSE_FILL(count, 0, 8, stream);
  if (n_chunks == 0) return HMSE_OK;
  if (!hits) hits_cap = 0;
  int rc = rx_validate(raw_off, n_rec, raw_bytes, cuts, slot, n_chunks, X, status, stream);
  if (rc != HMSE_OK) return rc;
  if (!RX_A && X.reach < 2) return HMSE_OK;           // plain, reach = 1: every start is a scan start
  // plain: the last reach - 1 starts of every chunk; asserting: its first start and its last `reach` ones
  const uint64_t n_threads = n_chunks * (uint64_t)(RX_A ? X.reach + 1 : X.reach - 1);
  uint64_t nb = (n_threads + RX_NT - 1) / RX_NT;
  if (nb > RX_MAX_BLOCKS) nb = RX_MAX_BLOCKS;         // (the table is staged once per workgroup; the rest by the grid stride)
  PROF_BEGIN(HMSE_STAGE_FIND_PLACE, stream);
  RX_KERNEL(seams_kernel)<<<dim3((uint32_t)nb), dim3(RX_NT), 0, stream>>>(raw, raw_off, cuts, slot, n_chunks, X, (unsigned long long*)hits, hits_cap,
                                                                          (unsigned long long*)n_hits, (unsigned long long*)count, status, n_threads);
  PROF_END(HMSE_STAGE_FIND_PLACE, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
#endif
