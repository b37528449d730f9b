// tally_emu.cpp — the kernels of hmse_amd/csrc/tally.hip run on the CPU, one std::thread per lane and a per-wavefront barrier under
// __ballot and the lane reads (a loop that is not wave-uniform hangs it), against the definition of include/hmse_tally.h, byte by byte,
// on random chunk maps: chunks of 0, 1 and 2 bytes and of up to a few trips, a single chunk, exact dedupe of the chunks, junk in front
// of and behind the records in raw, every table and raw in heap blocks of exactly the declared size (a sanitizer sees a read one byte
// outside), outputs that start poisoned with a guard behind them, bad ranges, bad rep, inconsistent tables.  The corpus is periodic half
// of the time, with a few letters' case flipped, so that equal and almost equal texts lie under different chunk splits.  No GPU: this
// checks the kernels' LOGIC and bounds (build it with a sanitizer), not their code object.  Driven by tools/tally_emu.py, which cuts the
// kernels out of tally.hip (everything between the geometry constants and the entry points) into tally_kernels.inc; the validate kernel
// comes from hmse_amd/csrc/chunkmap.h and gets cuts as its chunk_out as well, as tally.hip's launcher hands it over.  tools/hip_on_cpu.h
// has no DPP: wave_sum is built here on its emu_readlane.  After the random cases the program prints the keys of fixed ranges of a fixed
// corpus ("KEY ..." lines), which tests/test_tally_host.py holds against the plain-Python restatement of the key.
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>
#include "hmse_tally.h"
#include "hip_on_cpu.h"
static inline uint32_t wave_sum(uint32_t v) {          // every lane of the wavefront calls it: 64 lane reads
  uint32_t s = 0;
  for (uint32_t j = 0; j < 64; j++) s += emu_readlane(v, j);
  return s;
}
#include "chunkmap.h"
#include "blockops.h"
#include "tally_kernels.inc"

static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }
template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a heap block of exactly v.size() elements
  std::unique_ptr<T[]> p(v.empty() ? nullptr : new T[v.size()]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

// the definition (include/hmse_tally.h), byte by byte
static uint32_t fold_ref(uint32_t b, bool fold) { return fold && b >= 'A' && b <= 'Z' ? b + 32 : b; }
static uint64_t key_ref(const std::vector<uint8_t>& C, uint64_t s, uint64_t e, bool fold, uint64_t seed, uint32_t bits) {
  uint32_t a1 = 0, a2 = 0, p1 = 1, p2 = 1;
  for (uint64_t q = s; q < e; q++) {
    const uint32_t b = fold_ref(C[q], fold) + 1;
    a1 += b * p1; a2 += b * p2;
    p1 *= HMSE_TALLY_M1; p2 *= HMSE_TALLY_M2;
  }
  uint64_t x = ((uint64_t)a1 | ((uint64_t)a2 << 32)) ^ ((e - s) * HMSE_TALLY_LEN) ^ (seed * HMSE_TALLY_SEED);
  x ^= x >> 33; x *= HMSE_TALLY_MIX1; x ^= x >> 33; x *= HMSE_TALLY_MIX2; x ^= x >> 33;
  return bits >= 64 ? x : x & ((1ull << bits) - 1);
}
static bool same_ref(const std::vector<uint8_t>& C, uint64_t s, uint64_t e, uint64_t s2, uint64_t e2, bool fold) {
  if (e - s != e2 - s2) return false;
  for (uint64_t t = 0; t < e - s; t++) if (fold_ref(C[s + t], fold) != fold_ref(C[s2 + t], fold)) return false;
  return true;
}

struct Map {                                             // a corpus laid out as records and a chunk map
  std::vector<uint64_t> cuts, slot, raw_off;
  std::vector<uint8_t> raw;
  uint64_t n_chunks = 0, n_rec = 0;
};
static Map lay_out(const std::vector<uint8_t>& C, std::vector<uint64_t> cuts, bool junk) {
  Map m;
  m.cuts = cuts;
  m.n_chunks = cuts.size() - 1;
  std::map<std::string, uint64_t> seen;
  if (junk) for (uint64_t g = R(20); g > 0; g--) m.raw.push_back((uint8_t)R(256));       // junk in front of the records
  m.raw_off.push_back(m.raw.size());
  for (uint64_t k = 0; k < m.n_chunks; k++) {
    const std::string s(C.begin() + cuts[k], C.begin() + cuts[k + 1]);
    auto f = seen.find(s);
    if (f == seen.end()) {
      f = seen.emplace(s, m.raw_off.size() - 1).first;
      m.raw.insert(m.raw.end(), s.begin(), s.end());
      m.raw_off.push_back(m.raw.size());
    }
    m.slot.push_back(f->second);
  }
  m.n_rec = m.raw_off.size() - 1;
  if (junk) for (uint64_t g = R(20); g > 0; g--) m.raw.push_back((uint8_t)R(256));       // and behind them
  return m;
}

static void run_keys(const Map& m, const uint8_t* RAW, const uint64_t* RO, const uint64_t* CU, const uint64_t* SL, const uint64_t* S,
                     const uint64_t* E, uint64_t n, uint32_t fold, uint64_t seed, uint32_t bits, uint64_t* KEY, uint32_t* status) {
  launch_waves<TALLY_NT>(1, [&] { tables_validate_kernel<TALLY_NT>(RO, m.n_rec, m.raw.size(), CU, SL, m.n_chunks, CU, status); });
  launch_waves<TALLY_NT>(1, [&] { tally_ranges_kernel(CU, m.n_chunks, S, E, nullptr, n, status); });
  launch_waves<TALLY_NT>((uint32_t)((n + TALLY_NT / 64 - 1) / (TALLY_NT / 64)), [&] {
    tally_keys_kernel(RAW, RO, CU, SL, m.n_chunks, S, E, n, fold, seed, bits, KEY, status);
  });
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 30;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  static const uint32_t BITS[] = {1, 2, 8, 32, 63, 64};
  static const uint64_t SEEDS[] = {0, 1, 2, 1ull << 63, 0xFFFFFFFFFFFFFFFFull};
  const uint64_t POISON = 0xA5A5A5A5A5A5A5A5ull;
  int fails = 0;
  uint64_t n_keys = 0, n_same = 0;
  for (int it = 0; it < iters && !fails; it++) {
    // ---- a corpus and its chunk map ----
    const uint64_t N = R(6) == 0 ? R(3) : 1 + R(5 * TALLY_TRIP);
    const uint64_t period = R(2) ? 1 + R(90) : 0;
    static const char ALPHA[] = "abABzZ@[`{\xC1\xE1";
    std::vector<uint8_t> base(period ? period : 1), C(N);
    for (auto& x : base) x = (uint8_t)ALPHA[R(12)];
    for (uint64_t q = 0; q < N; q++) {
      C[q] = period ? base[q % period] : (uint8_t)ALPHA[R(12)];
      if (period && R(40) == 0) C[q] ^= 0x20;            // a flipped case bit: of a letter, of '@' / '`', '[' / '{' and 0xC1 / 0xE1
    }
    const int mode = (int)R(4);                          // 0: chunks of 0 / 1 / 2 bytes, 1: 1..150, 2: one chunk, 3: a mix with empty ones
    std::vector<uint64_t> cuts{0};
    while (cuts.back() < N) {
      uint64_t l = mode == 0 ? R(3) : mode == 1 ? 1 + R(150) : mode == 2 ? N : (R(3) == 0 ? 0 : 1 + R(2 * TALLY_TRIP + 3));
      if (cuts.back() + l > N) l = N - cuts.back();
      cuts.push_back(cuts.back() + l);
    }
    for (uint64_t k = R(3); k > 0; k--) cuts.push_back(N);           // empty chunks at the end; with N == 0 maybe no chunk at all
    Map m = lay_out(C, cuts, true);
    // ---- inconsistent tables, one time in eight ----
    int broken = 0;
    if (m.n_chunks >= 2 && N >= 4 && R(8) == 0) {
      broken = 1 + (int)R(4);
      if (broken == 1) { uint64_t k = 1 + R(m.n_chunks - 1); m.cuts[k] = m.cuts[k + 1] + 1 + R(5); }   // cuts descend
      if (broken == 2) m.slot[R(m.n_chunks)] = m.n_rec + R(3);                                         // a record outside the index
      if (broken == 3) { m.cuts[m.n_chunks] += 1 + R(100); }                                           // the last chunk is longer than its record
      if (broken == 4) m.cuts[0] = 1;                                                                  // the corpus does not start at 0
    }
    auto RAW = exact(m.raw); auto RO = exact(m.raw_off); auto CU = exact(m.cuts); auto SL = exact(m.slot);

    // ---- ranges: any, empty ones, the whole corpus, and (periodic corpus) a range and its copy some periods on ----
    const uint64_t n = R(6) == 0 ? 0 : 1 + R(11);
    std::vector<uint64_t> s(n), e(n), rep(n);
    for (uint64_t i = 0; i < n; i++) {
      const uint64_t x = R(N + 1), y = R(4) == 0 ? x : R(N + 1);
      s[i] = x < y ? x : y; e[i] = x < y ? y : x;
      if (R(7) == 0) { s[i] = 0; e[i] = N; }
      rep[i] = R(4) == 0 ? i : R(n);
      if (period && i > 0 && R(2)) {                     // a copy of range i - 1, shifted by whole periods (where it fits); sometimes one byte longer
        const uint64_t room = (N - e[i - 1]) / period, sh = room ? (1 + R(room)) * period : 0;
        s[i] = s[i - 1] + sh; e[i] = e[i - 1] + sh;
        if (R(6) == 0 && e[i] < N) e[i]++;
        rep[i] = i - 1;
      }
    }
    const bool fold = R(2);
    // ---- keys ----
    {
      std::vector<uint64_t> s2 = s, e2 = e;
      uint32_t want_status = broken ? 2u : 0u;
      const int refuse = n && !broken && R(6) == 0 ? 1 + (int)R(2) : 0;
      if (refuse == 1) { const uint64_t i = R(n); e2[i] = N + 1 + R(9); if (s2[i] > e2[i]) s2[i] = 0; want_status = 2; }     // leaves the corpus
      if (refuse == 2) { const uint64_t i = R(n); if (e2[i] > s2[i]) { std::swap(s2[i], e2[i]); want_status = 2; } }           // descends
      const uint64_t seed = SEEDS[R(5)];
      const uint32_t bits = BITS[R(6)];
      auto S = exact(s2); auto E = exact(e2);
      std::vector<uint64_t> key(n + 2, POISON);
      auto KEY = exact(key);
      uint32_t status = 0;
      run_keys(m, RAW.get(), RO.get(), CU.get(), SL.get(), S.get(), E.get(), n, fold, seed, bits, KEY.get(), &status);
      if (status != want_status) { printf("it %d: keys status %u, want %u (refuse %d, broken %d)\n", it, status, want_status, refuse, broken); fails++; }
      for (uint64_t i = 0; i < n && !fails; i++) {
        const uint64_t w = want_status ? 0 : key_ref(C, s2[i], e2[i], fold, seed, bits);
        if (KEY[i] != w) {
          printf("it %d: key of [%llu, %llu) (N %llu, fold %d, seed %llx, bits %u, chunks mode %d, broken %d, refuse %d): got %llx, want %llx\n", it,
                 (unsigned long long)s2[i], (unsigned long long)e2[i], (unsigned long long)N, (int)fold, (unsigned long long)seed, bits, mode, broken, refuse,
                 (unsigned long long)KEY[i], (unsigned long long)w);
          fails++;
        }
      }
      for (uint64_t i = n; i < n + 2; i++) if (KEY[i] != POISON) { printf("it %d: a key was written behind the end\n", it); fails++; }
      n_keys += n;
    }
    // ---- same ----
    {
      std::vector<uint64_t> s2 = s, e2 = e, rep2 = rep;
      uint32_t want_status = broken ? 2u : 0u;
      const int refuse = n && !broken && R(6) == 0 ? 1 + (int)R(3) : 0;
      if (refuse == 1) { const uint64_t i = R(n); e2[i] = N + 1 + R(9); if (s2[i] > e2[i]) s2[i] = 0; want_status = 2; }
      if (refuse == 2) { const uint64_t i = R(n); if (e2[i] > s2[i]) { std::swap(s2[i], e2[i]); want_status = 2; } }
      if (refuse == 3) { rep2[R(n)] = n + R(3) * (1ull << 40); want_status = 2; }                                              // a rep outside the ranges
      auto S = exact(s2); auto E = exact(e2); auto REP = exact(rep2);
      std::vector<uint8_t> sm(n + 2, 0xA5);
      auto SM = exact(sm);
      uint32_t status = 0;
      launch_waves<TALLY_NT>(1, [&] { tables_validate_kernel<TALLY_NT>(RO.get(), m.n_rec, m.raw.size(), CU.get(), SL.get(), m.n_chunks, CU.get(), &status); });
      launch_waves<TALLY_NT>(1, [&] { tally_ranges_kernel(CU.get(), m.n_chunks, S.get(), E.get(), REP.get(), n, &status); });
      launch_waves<TALLY_NT>((uint32_t)((n + TALLY_NT / 64 - 1) / (TALLY_NT / 64)), [&] {
        tally_same_kernel(RAW.get(), RO.get(), CU.get(), SL.get(), m.n_chunks, S.get(), E.get(), REP.get(), n, fold, SM.get(), &status);
      });
      if (status != want_status) { printf("it %d: same status %u, want %u (refuse %d, broken %d)\n", it, status, want_status, refuse, broken); fails++; }
      for (uint64_t i = 0; i < n && !fails; i++) {
        const uint8_t w = want_status ? 0 : (uint8_t)same_ref(C, s2[i], e2[i], s2[rep2[i]], e2[rep2[i]], fold);
        if (SM[i] != w) {
          printf("it %d: same of [%llu, %llu) and its rep %llu [%llu, %llu) (N %llu, fold %d, chunks mode %d, broken %d, refuse %d): got %u, want %u\n", it,
                 (unsigned long long)s2[i], (unsigned long long)e2[i], (unsigned long long)rep2[i], (unsigned long long)(want_status ? 0 : s2[rep2[i]]),
                 (unsigned long long)(want_status ? 0 : e2[rep2[i]]), (unsigned long long)N, (int)fold, mode, broken, refuse, SM[i], w);
          fails++;
        }
        n_same += !want_status && w;
      }
      for (uint64_t i = n; i < n + 2; i++) if (SM[i] != 0xA5) { printf("it %d: a same byte was written behind the end\n", it); fails++; }
    }
    if (!fails && (it % 20 == 19 || it + 1 == iters)) printf("it %d ok: %llu keys, %llu equal pairs so far\n", it, (unsigned long long)n_keys, (unsigned long long)n_same);
  }
  // ---- the keys of fixed ranges of a fixed corpus, for the plain-Python restatement: C[q] = (q * 37 + 11) & 0xFF, cut every 50 bytes ----
  if (!fails) {
    std::vector<uint8_t> C(300);
    for (uint64_t q = 0; q < C.size(); q++) C[q] = (uint8_t)(q * 37 + 11);
    std::vector<uint64_t> cuts;
    for (uint64_t q = 0; q <= C.size(); q += 50) cuts.push_back(q);
    Map m = lay_out(C, cuts, false);
    auto RAW = exact(m.raw); auto RO = exact(m.raw_off); auto CU = exact(m.cuts); auto SL = exact(m.slot);
    static const uint64_t LEN[] = {0, 1, 63, 64, 65, 128}, START[] = {0, 7, 49, 172};
    std::vector<uint64_t> s, e;
    for (uint64_t st : START) for (uint64_t l : LEN) { s.push_back(st); e.push_back(st + l); }
    const uint64_t n = s.size();
    auto S = exact(s); auto E = exact(e);
    for (uint64_t seed : {0ull, 1ull, 1ull << 63}) for (uint32_t fold = 0; fold < 2; fold++) for (uint32_t bits : {64u, 8u}) {
      std::vector<uint64_t> key(n, POISON);
      uint32_t status = 0;
      run_keys(m, RAW.get(), RO.get(), CU.get(), SL.get(), S.get(), E.get(), n, fold, seed, bits, key.data(), &status);
      for (uint64_t i = 0; i < n; i++)
        printf("KEY %llu %llu %u %llu %u %016llx\n", (unsigned long long)s[i], (unsigned long long)e[i], fold, (unsigned long long)seed, bits, (unsigned long long)key[i]);
      if (status) { printf("the fixed ranges were refused: status %u\n", status); fails++; }
    }
  }
  printf(fails ? "FAILED\n" : "ALL OK: %llu keys equal the definition, %llu equal pairs among the compared\n", (unsigned long long)n_keys, (unsigned long long)n_same);
  return fails;
}
