// lines_emu.cpp — the kernels of hmse_amd/csrc/lines.hip run on the CPU, one std::thread per lane and a per-wavefront barrier under
// __ballot (a loop that is not wave-uniform hangs it), against the brute-force definition of include/hmse.h on random chunk maps:
// chunks of 0, 1 and 2 bytes and of up to a few trips, exact dedupe of the chunks, junk in front of and behind the records in raw, every
// table and raw in heap blocks of exactly the declared size (a sanitizer sees a read one byte outside), outputs that start poisoned
// with a guard behind them, bad positions, inconsistent tables, refused gathers.  No GPU: this checks the kernels' LOGIC and bounds
// (build it with a sanitizer), not their code object.  Driven by tools/lines_emu.py, which cuts the kernels out of lines.hip
// (everything between the geometry constants and the entry points) into lines_kernels.inc; the validate kernel comes from
// hmse_amd/csrc/chunkmap.h and gets cuts as its chunk_out as well, as lines.hip's launcher hands it over; the gather kernel's per-piece
// copy is wave_copy of hmse_amd/csrc/blockops.h, included as it is (the same function gc.hip's record gather runs).
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
#include "hmse.h"
#include "hip_on_cpu.h"
#include "chunkmap.h"
#include "blockops.h"
#include "lines_kernels.inc"

static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }
template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a heap block of exactly v.size() elements
  std::unique_ptr<T[]> p(v.empty() ? nullptr : new T[v.size()]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

// the definition (include/hmse.h), byte by byte
static void extent_ref(const std::vector<uint8_t>& C, uint64_t o, uint32_t d, uint32_t b, uint32_t a, uint64_t Rr, uint64_t* st, uint64_t* en, uint8_t* fl) {
  const uint64_t N = C.size();
  const uint64_t lo = o > Rr ? o - Rr : 0, hi = o + Rr < N ? o + Rr : N;
  uint64_t need = (uint64_t)b + 1;
  *st = lo; *en = hi; *fl = 0;
  bool found = false;
  for (uint64_t p = o; p > lo && !found; p--)
    if (C[p - 1] == d && --need == 0) { *st = p; found = true; }
  if (!found && o > Rr) *fl |= HMSE_LINES_START_CUT;
  need = (uint64_t)a + 1; found = false;
  for (uint64_t p = o; p < hi && !found; p++)
    if (C[p] == d && --need == 0) { *en = p; found = true; }
  if (!found && o + Rr < N) *fl |= HMSE_LINES_END_CUT;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 30;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  static const uint32_t REACH[] = {1, 2, 3, LINES_TRIP - 1, LINES_TRIP, LINES_TRIP + 1, 3 * LINES_TRIP + 5, HMSE_LINES_MAX_REACH};
  static const uint32_t DELIM[] = {0x0A, 0x00, 0xFF, 'd'};
  int fails = 0;
  uint64_t n_pos = 0, n_rng = 0;
  for (int it = 0; it < iters && !fails; it++) {
    // ---- a corpus and its chunk map ----
    const uint32_t d = DELIM[R(4)];
    const uint64_t N = R(6) == 0 ? R(3) : 1 + R(5 * LINES_TRIP);
    static const uint32_t DENS[] = {2, 5, 20, 70, 1000000};
    const uint32_t dens = DENS[R(5)];
    std::vector<uint8_t> C(N);
    for (auto& x : C) x = R(dens) == 0 ? (uint8_t)d : (uint8_t)"ab"[R(2)];
    const int mode = (int)R(4);                          // 0: chunks of 0 / 1 / 2 bytes, 1: 1..150, 2: one chunk, 3: a mix with empty ones
    std::vector<uint64_t> cuts{0};
    while (cuts.back() < N) {
      uint64_t l = mode == 0 ? R(3) : mode == 1 ? 1 + R(150) : mode == 2 ? N : (R(3) == 0 ? 0 : 1 + R(2 * LINES_TRIP + 3));
      if (cuts.back() + l > N) l = N - cuts.back();
      cuts.push_back(cuts.back() + l);
    }
    for (uint64_t k = R(3); k > 0; k--) cuts.push_back(N);           // empty chunks at the end; with N == 0 maybe no chunk at all
    const uint64_t n_chunks = cuts.size() - 1;
    std::map<std::string, uint64_t> seen;
    std::vector<uint64_t> slot, raw_off;
    std::vector<uint8_t> raw;
    for (uint64_t g = R(20); g > 0; g--) raw.push_back(R(3) == 0 ? (uint8_t)d : (uint8_t)R(256));   // junk in front of the records
    raw_off.push_back(raw.size());
    for (uint64_t k = 0; k < n_chunks; k++) {
      const std::string s(C.begin() + cuts[k], C.begin() + cuts[k + 1]);
      auto f = seen.find(s);
      if (f == seen.end()) {
        f = seen.emplace(s, raw_off.size() - 1).first;
        raw.insert(raw.end(), s.begin(), s.end());
        raw_off.push_back(raw.size());
      }
      slot.push_back(f->second);
    }
    uint64_t n_rec = raw_off.size() - 1;
    for (uint64_t g = R(20); g > 0; g--) raw.push_back(R(3) == 0 ? (uint8_t)d : (uint8_t)R(256));   // and behind them
    // ---- inconsistent tables, one time in eight ----
    int broken = 0;
    if (n_chunks >= 2 && N >= 4 && R(8) == 0) {
      broken = 1 + (int)R(4);
      if (broken == 1) { uint64_t k = 1 + R(n_chunks - 1); cuts[k] = cuts[k + 1] + 1 + R(5); }        // cuts descend
      if (broken == 2) slot[R(n_chunks)] = n_rec + R(3);                                            // a record outside the index
      if (broken == 3) { cuts[n_chunks] += 1 + R(100); }                                            // the last chunk is longer than its record
      if (broken == 4) cuts[0] = 1;                                                                  // the corpus does not start at 0
    }
    auto RAW = exact(raw); auto RO = exact(raw_off); auto CU = exact(cuts); auto SL = exact(slot);
    const uint64_t raw_bytes = raw.size();

    // ---- extent ----
    {
      const uint64_t n = R(6) == 0 ? 0 : 1 + R(13);
      const uint32_t b = R(5) == 0 ? 0xFFFFFFFFu : (uint32_t)R(4), a = R(5) == 0 ? 0xFFFFFFFFu : (uint32_t)R(4), reach = REACH[R(8)];
      std::vector<uint64_t> pos(n);
      for (auto& p : pos) p = R(7) == 0 ? N + R(3) * (1ull << 40) : R(N);
      if (n && N && R(2)) pos[0] = R(2) ? 0 : N - 1;
      auto POS = exact(pos);
      std::vector<uint64_t> st(n + 2, 0xA5A5A5A5A5A5A5A5ull), en(n + 2, 0xA5A5A5A5A5A5A5A5ull);
      std::vector<uint8_t> fl(n + 2, 0xA5);
      auto ST = exact(st); auto EN = exact(en); auto FL = exact(fl);
      uint32_t status = 0, want_status = broken ? 2u : 0u;
      launch_waves<LINES_NT>(1, [&] { tables_validate_kernel<LINES_NT>(RO.get(), n_rec, raw_bytes, CU.get(), SL.get(), n_chunks, CU.get(), &status); });
      launch_waves<LINES_NT>((uint32_t)((n + LINES_NT / 64 - 1) / (LINES_NT / 64)), [&] {
        lines_extent_kernel(RAW.get(), RO.get(), CU.get(), SL.get(), n_chunks, POS.get(), n, d, b, a, reach, ST.get(), EN.get(), FL.get(), &status);
      });
      for (uint64_t i = 0; i < n && !fails; i++) {
        uint64_t ws = 0, we = 0; uint8_t wf = HMSE_LINES_BAD;
        if (!broken && pos[i] < N) extent_ref(C, pos[i], d, b, a, reach, &ws, &we, &wf);
        else if (!broken) want_status |= 1u;
        if (ST[i] != ws || EN[i] != we || FL[i] != wf) {
          printf("it %d: pos %llu (N %llu, d %u, b %u, a %u, reach %u, chunks mode %d, broken %d): got %llu %llu %u, want %llu %llu %u\n", it,
                 (unsigned long long)pos[i], (unsigned long long)N, d, b, a, reach, mode, broken, (unsigned long long)ST[i],
                 (unsigned long long)EN[i], FL[i], (unsigned long long)ws, (unsigned long long)we, wf);
          fails++;
        }
      }
      for (uint64_t i = n; i < n + 2; i++)
        if (ST[i] != 0xA5A5A5A5A5A5A5A5ull || EN[i] != 0xA5A5A5A5A5A5A5A5ull || FL[i] != 0xA5) { printf("it %d: an output was written behind its end\n", it); fails++; }
      if (status != want_status) { printf("it %d: extent status %u, want %u (broken %d)\n", it, status, want_status, broken); fails++; }
      n_pos += n;
    }

    // ---- gather ----
    {
      const uint64_t n = R(6) == 0 ? 0 : 1 + R(9);
      std::vector<uint64_t> s(n), e(n), off(n + 1, 0);
      for (uint64_t i = 0; i < n; i++) {
        const uint64_t x = R(N + 1), y = R(4) == 0 ? x : R(N + 1);
        s[i] = x < y ? x : y; e[i] = x < y ? y : x;
        if (R(5) == 0) { s[i] = 0; e[i] = N; }
        off[i + 1] = off[i] + (e[i] - s[i]);
      }
      const uint64_t total = off[n];
      std::vector<uint8_t> want(total);
      for (uint64_t i = 0; i < n; i++) for (uint64_t p = s[i]; p < e[i]; p++) want[off[i] + (p - s[i])] = C[p];
      uint64_t out_cap = total;
      uint32_t want_status = broken ? 2u : 0u;
      const int refuse = n && !broken && R(4) == 0 ? 1 + (int)R(4) : 0;
      if (refuse == 1) { if (total) { out_cap = total - 1; want_status = 1; } }
      if (refuse == 2) { const uint64_t i = R(n); e[i] = N + 1 + R(9); want_status = 2; }                       // leaves the corpus (and its length disagrees)
      if (refuse == 3) { const uint64_t i = R(n); if (e[i] > s[i]) { std::swap(s[i], e[i]); want_status = 2; } } // descends
      if (refuse == 4) { const uint64_t i = R(n); off[i + 1] += 1; want_status = 2; if (i + 1 == n) out_cap = off[n]; }      // not the prefix sum
      auto S = exact(s); auto E = exact(e); auto OFF = exact(off);
      const uint64_t mis = R(16);
      std::unique_ptr<uint8_t[]> OUT(new uint8_t[mis + out_cap + 1]);      // (+ 1: a block of its own also when nothing is to be written)
      memset(OUT.get(), 0xA5, mis + out_cap + 1);
      uint32_t status = 0;
      launch_waves<LINES_NT>(1, [&] { tables_validate_kernel<LINES_NT>(RO.get(), n_rec, raw_bytes, CU.get(), SL.get(), n_chunks, CU.get(), &status); });
      launch_waves<LINES_NT>(1, [&] { lines_ranges_kernel(CU.get(), n_chunks, S.get(), E.get(), OFF.get(), n, out_cap, &status); });
      launch_waves<LINES_NT>((uint32_t)((n + LINES_NT / 64 - 1) / (LINES_NT / 64)), [&] {
        lines_gather_kernel(RAW.get(), RO.get(), CU.get(), SL.get(), n_chunks, S.get(), E.get(), OFF.get(), n, OUT.get() + mis, &status);
      });
      if (status != want_status) { printf("it %d: gather status %u, want %u (refuse %d, broken %d)\n", it, status, want_status, refuse, broken); fails++; }
      for (uint64_t k = 0; k < mis + out_cap + 1 && !fails; k++) {
        const bool body = !want_status && k >= mis && k < mis + total;
        const uint8_t w = body ? want[k - mis] : 0xA5;
        if (OUT[k] != w) { printf("it %d: out[%lld] = %u, want %u (refuse %d, broken %d, mis %llu)\n", it, (long long)k - (long long)mis, OUT[k], w, refuse, broken, (unsigned long long)mis); fails++; }
      }
      n_rng += n;
    }
    if (!fails && (it % 20 == 19 || it + 1 == iters)) printf("it %d ok: %llu positions, %llu ranges so far\n", it, (unsigned long long)n_pos, (unsigned long long)n_rng);
  }
  printf(fails ? "FAILED\n" : "ALL OK: %llu positions and %llu ranges equal the definition\n", (unsigned long long)n_pos, (unsigned long long)n_rng);
  return fails;
}
