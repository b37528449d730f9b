// order_emu.cpp — the kernels of hmse_amd/csrc/order.hip run on the CPU, one std::thread per lane and a per-wavefront barrier under
// __ballot (a loop that is not wave-uniform hangs it), against the definition of include/hmse_order.h, byte by byte, on random chunk
// maps: chunks of 0, 1 and 2 bytes and of up to a few trips, a single chunk, mixes with empty chunks, exact dedupe of the chunks, junk in
// front of and behind the records in raw, every table and raw in heap blocks of exactly the declared size (a sanitizer sees a read one
// byte outside), outputs that start poisoned with a guard behind them, and every refusal: bad ranges, a depth beyond the text, a rep
// outside the ranges, a from beyond the shorter text, inconsistent tables.  The corpus is periodic half of the time, with a few letters'
// case flipped, so that long common prefixes lie under different chunk splits; the bytes in front of from[i] are NOT promised equal in
// the LCP cases, so a kernel that looked at them would answer differently from the definition.  No GPU: this checks the kernels' LOGIC
// and bounds (build it with a sanitizer), not their code object.  Driven by tools/order_emu.py, which cuts the kernels out of order.hip
// (everything between the geometry constants and the entry points) into order_kernels.inc; the validate kernel comes from
// hmse_amd/csrc/chunkmap.h and gets cuts as its chunk_out as well, as order.hip's launcher hands it over.  After the random cases the
// program prints the keys of fixed ranges of a fixed corpus ("KEY ..." lines), which tests/test_order_host.py holds against the
// plain-Python restatement of the key.
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
#include "hmse_order.h"
#include "hip_on_cpu.h"
#include "chunkmap.h"
#include "order_kernels.inc"

static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }
template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a heap block of exactly v.size() elements
  std::unique_ptr<T[]> p(v.empty() ? nullptr : new T[v.size()]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

// the definition (include/hmse_order.h), byte by byte
static uint32_t fold_ref(uint32_t b, bool fold) { return fold && b >= 'A' && b <= 'Z' ? b + 32 : b; }
static uint64_t key_ref(const std::vector<uint8_t>& C, uint64_t s, uint64_t e, uint64_t d, bool fold) {
  const uint64_t L = e - s;
  uint64_t k = 0;
  for (uint64_t j = 0; j < 7; j++) k = (k << 8) | (d + j < L ? fold_ref(C[s + d + j], fold) : 0);
  return (k << 4) | (L - d < 8 ? L - d : 8);
}
static uint64_t lcp_ref(const std::vector<uint8_t>& C, uint64_t s, uint64_t e, uint64_t s2, uint64_t e2, uint64_t from, bool self, bool fold) {
  if (self) return e - s;
  const uint64_t m = e - s < e2 - s2 ? e - s : e2 - s2;
  uint64_t t = from;
  while (t < m && fold_ref(C[s + t], fold) == fold_ref(C[s2 + t], fold)) t++;
  return t;
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
                     const uint64_t* E, const uint64_t* D, uint64_t n, uint32_t fold, uint64_t* KEY, uint32_t* status) {
  const uint32_t blocks = (uint32_t)((n + ORDER_NT - 1) / ORDER_NT);
  launch_waves<ORDER_NT>(1, [&] { tables_validate_kernel<ORDER_NT>(RO, m.n_rec, m.raw.size(), CU, SL, m.n_chunks, CU, status); });
  launch_waves<ORDER_NT>(blocks, [&] { order_ranges_kernel(CU, m.n_chunks, S, E, D, nullptr, nullptr, n, status); });
  launch_waves<ORDER_NT>(blocks, [&] { order_keys_kernel(RAW, RO, CU, SL, m.n_chunks, S, E, D, n, fold, KEY, status); });
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 30;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  const uint64_t POISON = 0xA5A5A5A5A5A5A5A5ull;
  int fails = 0;
  uint64_t n_keys = 0, n_lcp = 0, n_long = 0, refused = 0;
  for (int it = 0; it < iters && !fails; it++) {
    // ---- a corpus and its chunk map ----
    const uint64_t N = R(6) == 0 ? R(3) : 1 + R(5 * ORDER_TRIP);
    const uint64_t period = R(2) ? 1 + R(90) : 0;
    static const char ALPHA[] = "abABzZ@[`{\xC1\xE1\x00\xFF";
    std::vector<uint8_t> base(period ? period : 1), C(N);
    for (auto& x : base) x = (uint8_t)ALPHA[R(14)];
    for (uint64_t q = 0; q < N; q++) {
      C[q] = period ? base[q % period] : (uint8_t)ALPHA[R(14)];
      if (period && R(40) == 0) C[q] ^= 0x20;            // a flipped case bit: of a letter, of '@' / '`', '[' / '{' and 0xC1 / 0xE1
    }
    const int mode = (int)R(4);                          // 0: chunks of 0 / 1 / 2 bytes, 1: 1..150, 2: one chunk, 3: a mix with empty ones
    std::vector<uint64_t> cuts{0};
    while (cuts.back() < N) {
      uint64_t l = mode == 0 ? R(3) : mode == 1 ? 1 + R(150) : mode == 2 ? N : (R(3) == 0 ? 0 : 1 + R(2 * ORDER_TRIP + 3));
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
      std::vector<uint64_t> s2 = s, e2 = e, d(n);
      for (uint64_t i = 0; i < n; i++) {                 // depth 0, the end, within nine bytes of the end, anywhere
        const uint64_t L = e[i] - s[i], w = R(4);
        d[i] = w == 0 ? 0 : w == 1 ? L : w == 2 ? L - R((L < 9 ? L : 9) + 1) : R(L + 1);
      }
      uint32_t want_status = broken ? 2u : 0u;
      const int refuse = n && !broken && R(5) == 0 ? 1 + (int)R(3) : 0;
      if (refuse == 1) { const uint64_t i = R(n); e2[i] = N + 1 + R(9); if (s2[i] > e2[i]) s2[i] = 0; want_status = 2; }     // leaves the corpus
      if (refuse == 2) { const uint64_t i = R(n); if (e2[i] > s2[i]) { std::swap(s2[i], e2[i]); want_status = 2; } }           // descends
      if (refuse == 3) { const uint64_t i = R(n); d[i] = e2[i] - s2[i] + 1 + R(3) * (1ull << 40); want_status = 2; }           // a depth beyond the text
      auto S = exact(s2); auto E = exact(e2); auto D = exact(d);
      std::vector<uint64_t> key(n + 2, POISON);
      auto KEY = exact(key);
      uint32_t status = 0;
      run_keys(m, RAW.get(), RO.get(), CU.get(), SL.get(), S.get(), E.get(), D.get(), n, fold, KEY.get(), &status);
      if (status != want_status) { printf("it %d: keys status %u, want %u (refuse %d, broken %d)\n", it, status, want_status, refuse, broken); fails++; }
      for (uint64_t i = 0; i < n && !fails; i++) {
        const uint64_t w = want_status ? 0 : key_ref(C, s2[i], e2[i], d[i], fold);
        if (KEY[i] != w) {
          printf("it %d: key of [%llu, %llu) at depth %llu (N %llu, fold %d, chunks mode %d, broken %d, refuse %d): got %llx, want %llx\n", it,
                 (unsigned long long)s2[i], (unsigned long long)e2[i], (unsigned long long)d[i], (unsigned long long)N, (int)fold, mode, broken, refuse,
                 (unsigned long long)KEY[i], (unsigned long long)w);
          fails++;
        }
      }
      for (uint64_t i = n; i < n + 2; i++) if (KEY[i] != POISON) { printf("it %d: a key was written behind the end\n", it); fails++; }
      n_keys += n;
      refused += want_status != 0;
    }
    // ---- lcp ----
    {
      std::vector<uint64_t> s2 = s, e2 = e, rep2 = rep, from(n);
      for (uint64_t i = 0; i < n; i++) {                 // from: 0, the shorter text's length, anywhere up to it — whatever lies in front of it
        const uint64_t Li = e[i] - s[i], Lr = e[rep[i]] - s[rep[i]], mn = Li < Lr ? Li : Lr, w = R(3);
        from[i] = w == 0 ? 0 : w == 1 ? mn : R(mn + 1);
      }
      uint32_t want_status = broken ? 2u : 0u;
      const int refuse = n && !broken && R(5) == 0 ? 1 + (int)R(4) : 0;
      if (refuse == 1) { const uint64_t i = R(n); e2[i] = N + 1 + R(9); if (s2[i] > e2[i]) s2[i] = 0; want_status = 2; }
      if (refuse == 2) { const uint64_t i = R(n); if (e2[i] > s2[i]) { std::swap(s2[i], e2[i]); want_status = 2; } }
      if (refuse == 3) { rep2[R(n)] = n + R(3) * (1ull << 40); want_status = 2; }                                              // a rep outside the ranges
      if (refuse == 4) {                                                                                                       // a from beyond the shorter text
        const uint64_t i = R(n), Li = e2[i] - s2[i], Lr = e2[rep2[i]] - s2[rep2[i]];
        from[i] = (Li < Lr ? Li : Lr) + 1 + R(3) * (1ull << 40); want_status = 2;
      }
      auto S = exact(s2); auto E = exact(e2); auto REP = exact(rep2); auto FROM = exact(from);
      std::vector<uint64_t> out(n + 2, POISON);
      auto OUT = exact(out);
      uint32_t status = 0;
      const uint32_t blocks = (uint32_t)((n + ORDER_NT - 1) / ORDER_NT);
      launch_waves<ORDER_NT>(1, [&] { tables_validate_kernel<ORDER_NT>(RO.get(), m.n_rec, m.raw.size(), CU.get(), SL.get(), m.n_chunks, CU.get(), &status); });
      launch_waves<ORDER_NT>(blocks, [&] { order_ranges_kernel(CU.get(), m.n_chunks, S.get(), E.get(), nullptr, REP.get(), FROM.get(), n, &status); });
      launch_waves<ORDER_NT>((uint32_t)((n + ORDER_NT / 64 - 1) / (ORDER_NT / 64)), [&] {
        order_lcp_kernel(RAW.get(), RO.get(), CU.get(), SL.get(), m.n_chunks, S.get(), E.get(), REP.get(), FROM.get(), n, fold, OUT.get(), &status);
      });
      if (status != want_status) { printf("it %d: lcp status %u, want %u (refuse %d, broken %d)\n", it, status, want_status, refuse, broken); fails++; }
      for (uint64_t i = 0; i < n && !fails; i++) {
        const uint64_t w = want_status ? 0 : lcp_ref(C, s2[i], e2[i], s2[rep2[i]], e2[rep2[i]], from[i], rep2[i] == i, fold);
        if (OUT[i] != w) {
          printf("it %d: lcp of [%llu, %llu) and its rep %llu from %llu (N %llu, fold %d, chunks mode %d, broken %d, refuse %d): got %llu, want %llu\n", it,
                 (unsigned long long)s2[i], (unsigned long long)e2[i], (unsigned long long)rep2[i], (unsigned long long)from[i], (unsigned long long)N,
                 (int)fold, mode, broken, refuse, (unsigned long long)OUT[i], (unsigned long long)w);
          fails++;
        }
        n_long += !want_status && rep2[i] != i && w >= from[i] + ORDER_TRIP;
      }
      for (uint64_t i = n; i < n + 2; i++) if (OUT[i] != POISON) { printf("it %d: an lcp was written behind the end\n", it); fails++; }
      n_lcp += n;
      refused += want_status != 0;
    }
    if (!fails && (it % 20 == 19 || it + 1 == iters))
      printf("it %d ok: %llu keys, %llu lcps (%llu of over a trip), %llu refused calls so far\n", it, (unsigned long long)n_keys, (unsigned long long)n_lcp,
             (unsigned long long)n_long, (unsigned long long)refused);
  }
  // ---- the keys of fixed ranges of a fixed corpus, for the plain-Python restatement: C[q] = (q * 37 + 11) & 0xFF with 0x00 and 0xFF
  // planted where windows end, cut every 5 bytes: "KEY start end depth fold key" ----
  if (!fails) {
    std::vector<uint8_t> C(300);
    for (uint64_t q = 0; q < C.size(); q++) C[q] = (uint8_t)(q * 37 + 11);
    C[7 + 6] = 0x00; C[49 + 6] = 0xFF; C[172 + 7] = 0x00; C[172 + 8] = 0xFF;
    std::vector<uint64_t> cuts;
    for (uint64_t q = 0; q <= C.size(); q += 5) cuts.push_back(q);
    Map m = lay_out(C, cuts, false);
    auto RAW = exact(m.raw); auto RO = exact(m.raw_off); auto CU = exact(m.cuts); auto SL = exact(m.slot);
    static const uint64_t LEN[] = {0, 1, 6, 7, 8, 9, 15, 16, 64}, START[] = {0, 7, 49, 172};
    std::vector<uint64_t> s, e, d;
    for (uint64_t st : START) for (uint64_t l : LEN) for (uint64_t back : {100ull, 101ull, 0ull, 6ull, 7ull, 8ull, 9ull}) {     // depth 0, 1, and L - back
      const uint64_t dp = back == 100 ? 0 : back == 101 ? 1 : l - back;
      if ((back >= 100 ? dp : back) > l) continue;
      s.push_back(st); e.push_back(st + l); d.push_back(dp);
    }
    const uint64_t n = s.size();
    auto S = exact(s); auto E = exact(e); auto D = exact(d);
    for (uint32_t fold = 0; fold < 2; fold++) {
      std::vector<uint64_t> key(n, POISON);
      uint32_t status = 0;
      run_keys(m, RAW.get(), RO.get(), CU.get(), SL.get(), S.get(), E.get(), D.get(), n, fold, key.data(), &status);
      for (uint64_t i = 0; i < n; i++)
        printf("KEY %llu %llu %llu %u %016llx\n", (unsigned long long)s[i], (unsigned long long)e[i], (unsigned long long)d[i], fold, (unsigned long long)key[i]);
      if (status) { printf("the fixed ranges were refused: status %u\n", status); fails++; }
    }
  }
  printf(fails ? "FAILED\n" : "ALL OK: %llu keys and %llu lcps equal the definition (%llu lcps of over a trip, %llu refused calls)\n", (unsigned long long)n_keys,
         (unsigned long long)n_lcp, (unsigned long long)n_long, (unsigned long long)refused);
  return fails;
}
