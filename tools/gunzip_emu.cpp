// gunzip_emu.cpp — the kernels of hmse_amd/csrc/gunzip.hip run on the CPU, one std::thread per lane, a std::barrier under __syncthreads
// and one per wavefront under __ballot, readlane and readfirstlane (tools/hip_on_cpu.h: a loop that is not wave-uniform hangs here, a
// value that is not uniform gives a wrong answer).  The candidate passes against the byte filter written out below, on buffers of every
// length around the 20 bytes of room and the tile size, with the magic planted across every thread and tile boundary, cap below, at and
// above the count; the measure kernel — with ifl::Bits, build_table and decode_sym of inflate_core.h as they are — against known answers
// that tools/gunzip_emu.py takes from zlib (tests/gunzip_ref.py: headers of every flag combination, stored / fixed / dynamic streams,
// BGZF blocks, truncated and mutated members, candidates inside other members).  Every input is a heap block of exactly the declared
// size (a sanitizer sees a read one byte outside); outputs start poisoned.  No GPU: this checks the kernels' LOGIC and bounds, not their
// code object.
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <random>
#include <thread>
#include <vector>
#include "hmse_gunzip.h"
#include "hip_on_cpu.h"
#include "blockops.h"
#include "inflate_core.h"
#include "gunzip_kernels.inc"

static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }
template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a heap block of exactly v.size() elements
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

static std::vector<uint64_t> filter_ref(const std::vector<uint8_t>& d) {
  std::vector<uint64_t> out;
  for (uint64_t p = 0; p + 20 <= d.size(); p++)
    if (d[p] == 0x1f && d[p + 1] == 0x8b && d[p + 2] == 8 && (d[p + 3] & 0xE0) == 0) out.push_back(p);
  return out;
}

static int run_candidates(const std::vector<uint8_t>& data, uint64_t cap, const char* what) {
  const uint64_t n = data.size();
  const auto want = filter_ref(data);
  const uint64_t nb = n < 20 ? 0 : (n - 20 + 1 + GZ_TILE - 1) / GZ_TILE;
  auto D = exact(data);
  std::vector<uint32_t> bsum(nb + 1, 0xA5A5A5A5u);
  std::vector<uint64_t> out(cap + 2, 0xA5A5A5A5A5A5A5A5ull);
  auto OUT = exact(out);
  uint64_t count = 0;                                 // (the entry point clears count and status)
  uint32_t status = 0;
  if (nb) {
    launch_block<GZ_NT>((uint32_t)nb, [&] { gz::candidates_count_kernel(D.get(), n, bsum.data()); });
    launch_block<GZ_SCAN_NT>(1, [&] { block_sums_scan_kernel<GZ_SCAN_NT>(bsum.data(), nb, &count, nullptr); });
    launch_block<GZ_NT>((uint32_t)nb, [&] { gz::candidates_compact_kernel(D.get(), n, bsum.data(), OUT.get(), cap, &count, &status); });
  }
  int fails = 0;
  if (count != want.size() || status != (want.size() > cap ? 1u : 0u)) {
    printf("%s: n %llu cap %llu: count %llu (want %zu), status %u\n", what, (unsigned long long)n, (unsigned long long)cap, (unsigned long long)count, want.size(), status);
    fails++;
  }
  for (uint64_t i = 0; i < cap + 2 && !fails; i++) {
    const uint64_t w = i < cap && i < want.size() ? want[i] : 0xA5A5A5A5A5A5A5A5ull;
    if (OUT[i] != w) { printf("%s: n %llu cap %llu: cand_off[%llu] = %llu, want %llu\n", what, (unsigned long long)n, (unsigned long long)cap, (unsigned long long)i, (unsigned long long)OUT[i], (unsigned long long)w); fails++; }
  }
  return fails;
}

static void plant(std::vector<uint8_t>& d, uint64_t p, uint8_t flg) {
  static const uint8_t M[3] = {0x1f, 0x8b, 8};
  for (int i = 0; i < 3; i++) if (p + i < d.size()) d[p + i] = M[i];
  if (p + 3 < d.size()) d[p + 3] = flg;
}

struct Want { uint64_t off, stream_off, end, raw_len; uint32_t crc, flags; };

// the file of tools/gunzip_emu.py: per case u32 n, n bytes, u32 n_cand, n_cand x (u64 off, u64 stream_off, u64 end, u64 raw_len, u32 crc, u32 flags)
static int known_answers(const char* path, uint64_t* n_done) {
  FILE* f = fopen(path, "rb");
  if (!f) { printf("no known answers at %s\n", path); return 1; }
  int cases = 0, bad = 0;
  uint32_t n;
  while (fread(&n, 4, 1, f) == 1) {
    std::vector<uint8_t> data(n);
    uint32_t nc;
    if ((n && fread(data.data(), 1, n, f) != n) || fread(&nc, 4, 1, f) != 1) { bad++; break; }
    std::vector<Want> want(nc);
    std::vector<uint64_t> cand(nc);
    for (uint32_t k = 0; k < nc; k++) {
      Want& w = want[k];
      if (fread(&w.off, 8, 1, f) != 1 || fread(&w.stream_off, 8, 1, f) != 1 || fread(&w.end, 8, 1, f) != 1 || fread(&w.raw_len, 8, 1, f) != 1 ||
          fread(&w.crc, 4, 1, f) != 1 || fread(&w.flags, 4, 1, f) != 1) { bad++; break; }
      cand[k] = w.off;
    }
    auto D = exact(data); auto C = exact(cand);
    std::vector<uint64_t> so(nc + 1, 0xA5), en(nc + 1, 0xA5), rl(nc + 1, 0xA5);
    std::vector<uint32_t> crc(nc + 1, 0xA5), fl(nc + 1, 0xA5);
    uint32_t counter = 0;
    gz::MeasureArgs a;
    a.data = D.get(); a.n = n; a.cand_off = C.get(); a.n_cand = nc;
    a.stream_off = so.data(); a.end = en.data(); a.raw_len = rl.data(); a.crc = crc.data(); a.flags = fl.data(); a.counter = &counter;
    launch_waves<GZ_NT>(1 + (uint32_t)(cases & 1), [&] { gz::measure_kernel(a); });
    for (uint32_t k = 0; k < nc; k++) {
      const Want& w = want[k];
      const uint32_t why = w.flags >> HMSE_GZIP_WHY_SHIFT, got = fl[k] >> HMSE_GZIP_WHY_SHIFT;
      bool ok = (fl[k] & 3u) == (w.flags & 3u);
      if (w.flags & HMSE_GZIP_VALID) ok = ok && got == 0 && so[k] == w.stream_off && en[k] == w.end && rl[k] == w.raw_len && crc[k] == w.crc;
      else ok = ok && en[k] == w.off && rl[k] == 0 && crc[k] == 0 &&
                ((why == HMSE_GZIP_WHY_HEADER || why == HMSE_GZIP_WHY_LENGTH) ? got == why : (got == HMSE_GZIP_WHY_STREAM || got == HMSE_GZIP_WHY_BOUNDS));
      if (!ok) {
        printf("case %d candidate %u at %llu: flags %#x stream_off %llu end %llu raw_len %llu crc %08x, want %#x %llu %llu %llu %08x\n", cases, k,
               (unsigned long long)w.off, fl[k], (unsigned long long)so[k], (unsigned long long)en[k], (unsigned long long)rl[k], crc[k], w.flags,
               (unsigned long long)w.stream_off, (unsigned long long)w.end, (unsigned long long)w.raw_len, w.crc);
        bad++;
      }
    }
    if (so[nc] != 0xA5 || en[nc] != 0xA5 || rl[nc] != 0xA5 || crc[nc] != 0xA5 || fl[nc] != 0xA5) { printf("case %d: an output behind the candidates was written\n", cases); bad++; }
    *n_done += nc;
    cases++;
  }
  fclose(f);
  printf("known answers (zlib): %d cases, %llu candidates, %d wrong\n", cases, (unsigned long long)*n_done, bad);
  return bad || cases == 0;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 6;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  int fails = 0;
  uint64_t n_bufs = 0, n_meas = 0;
  // ---- hmse_gzip_candidates ----
  for (uint64_t n : {0, 1, 19, 20, 21, 35, 36, 37}) {      // nothing but 1f 8b 08 00
    std::vector<uint8_t> d(n);
    for (uint64_t i = 0; i < n; i++) d[i] = (uint8_t)(0x00088B1Fu >> (8 * (i & 3)));
    const uint64_t c = filter_ref(d).size();
    for (uint64_t cap : {c, c ? c - 1 : 0, c + 3, (uint64_t)0}) { fails += run_candidates(d, cap, "all magic"); n_bufs++; }
  }
  for (int it = 0; it < iters && !fails; it++) {
    const uint64_t T = GZ_TILE, W = GZ_NT * GZ_PER;
    static const uint64_t NS[] = {T - 1, T, T + 1, T + 19, T + 20, T + 21, T + 22, 2 * T + 19 + 5, W + 19, W + 20, W + 35, 3 * T - 7, 40, 5000};
    const uint64_t n = NS[it % (sizeof NS / sizeof *NS)] + (it >= 14 ? R(300) : 0);
    std::vector<uint8_t> d(n);
    const int fill = (int)R(3);
    for (auto& x : d) x = fill == 0 ? (uint8_t)R(256) : fill == 1 ? 0x1f : 0x8b;
    for (uint64_t b : {(uint64_t)16, W, T, 2 * T})     // across a thread's 16 positions, a trip, a tile: the magic split at each of its points
      for (int s = 0; s <= 4; s++) if (b >= (uint64_t)s) plant(d, b - s, (uint8_t)R(32));
    if (n >= 20) { plant(d, n - 20, 0); if (R(2)) plant(d, n - 19 + R(19), 0); }       // the last position with room; behind it: none
    plant(d, R(n), 0x20); plant(d, R(n), 0xE0); plant(d, R(n), 0x1F);                  // reserved FLG bits, all the others
    for (int k = 0; k < 20; k++) plant(d, R(n), (uint8_t)R(256));
    const uint64_t c = filter_ref(d).size();
    for (uint64_t cap : {c, c / 2, c + 1}) { fails += run_candidates(d, cap, "planted"); n_bufs++; }
    if (!fails) printf("it %d ok: n %llu, %llu candidates\n", it, (unsigned long long)n, (unsigned long long)c);
  }
  // ---- hmse_gzip_measure ----
  if (!fails && argc > 3) fails += known_answers(argv[3], &n_meas);
  printf(fails ? "FAILED\n" : "ALL OK: %llu candidate runs equal the byte filter, %llu measured candidates equal zlib\n", (unsigned long long)n_bufs, (unsigned long long)n_meas);
  return fails;
}
