// sync_emu.cpp — the kernel of hmse_amd/csrc/sync.hip run on the CPU, one std::thread per lane and a per-wavefront barrier under __ballot,
// against memcmp: random record tables over two blobs of exactly the declared size (a sanitizer sees a read one byte outside), every pair of
// misalignments, lengths around 0, 16 and the 1 KiB trip, differences planted at the first and last byte and at the trip boundary, candidates
// that are missing, out of range or out of bounds, and an output buffer that starts poisoned.  No GPU: this checks the kernel's LOGIC and
// its bounds (build it with a sanitizer), not its code object.  Driven by tools/sync_emu.py, which cuts the kernel out of sync.hip
// (everything in front of its entry point) into sync_kernels.inc.
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
#include "hmse.h"
#include "hip_on_cpu.h"
#include "sync_kernels.inc"

static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 30;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  static const uint32_t LEN[] = {0, 1, 15, 16, 17, 31, 63, 64, 1023, 1024, 1025, 1039, 1040, 2047, 2048, 2049, 4097, 3000, 33, 5};
  int fails = 0;
  for (int it = 0; it < iters && !fails; it++) {
    const uint64_t n_b = R(4) == 0 ? 0 : 1 + R(12), n = R(8) == 0 ? 0 : 1 + R(14);
    // store b: records at random misalignments, junk between them, the last one ends at the end of the allocation
    std::vector<uint8_t> bv;
    std::vector<uint64_t> b_off; std::vector<uint32_t> b_len;
    for (uint64_t j = 0; j < n_b; j++) {
      for (uint64_t g = R(17); g > 0; g--) bv.push_back((uint8_t)R(256));
      const uint32_t l = LEN[R(sizeof LEN / sizeof *LEN)];
      b_off.push_back(bv.size()); b_len.push_back(l);
      for (uint32_t i = 0; i < l; i++) bv.push_back((uint8_t)R(256));
    }
    // store a: per record a copy of a record of b (equal, or with one planted difference), a record of its own, or a broken entry
    std::vector<uint8_t> av;
    std::vector<uint64_t> a_off; std::vector<uint32_t> a_len; std::vector<int64_t> cand;
    for (uint64_t k = 0; k < n; k++) {
      for (uint64_t g = R(17); g > 0; g--) av.push_back((uint8_t)R(256));
      const int mode = (int)R(10);
      int64_t c = n_b ? (int64_t)R(n_b) : -1;
      uint32_t l = LEN[R(sizeof LEN / sizeof *LEN)];
      a_off.push_back(av.size());
      if (n_b && mode < 6) {                                  // a copy of b's record
        l = b_len[c];
        av.insert(av.end(), bv.begin() + b_off[c], bv.begin() + b_off[c] + l);
        if (l && mode >= 2) {                                 // one difference: first byte, last byte, around the trip boundary, anywhere
          static const uint32_t AT[] = {0, 1023, 1024, 15, 16};
          uint32_t at = mode == 2 ? 0 : mode == 3 ? l - 1 : mode == 4 ? AT[R(5)] : (uint32_t)R(l);
          if (at >= l) at = (uint32_t)R(l);
          av[a_off[k] + at] ^= (uint8_t)(1 + R(255));
        }
      } else {
        for (uint32_t i = 0; i < l; i++) av.push_back((uint8_t)R(256));
        if (mode == 7) c = -1 - (int64_t)R(3);
        if (mode == 8) c = (int64_t)(n_b + R(3));
      }
      a_len.push_back(l); cand.push_back(c);
    }
    const uint64_t a_bytes = av.size(), b_bytes = bv.size();
    // broken ranges: an entry that ends past its blob, an offset past it, a length near 2^32
    if (n && R(3) == 0) { const uint64_t k = R(n); const int w = (int)R(3); if (w == 0) a_len[k] = (uint32_t)(a_bytes - a_off[k] + 1 + R(40)); else if (w == 1) a_off[k] = a_bytes + 1 + R(1000); else a_len[k] = 0xFFFFFFF0u; }
    if (n_b && R(3) == 0) { const uint64_t j = R(n_b); if (R(2)) b_len[j] = (uint32_t)(b_bytes - b_off[j] + 1 + R(40)); else b_off[j] = ~0ull - R(8); }
    // exact-size heap copies: a read one byte outside either blob is a sanitizer report
    std::unique_ptr<uint8_t[]> A(a_bytes ? new uint8_t[a_bytes] : nullptr), B(b_bytes ? new uint8_t[b_bytes] : nullptr);
    if (a_bytes) memcpy(A.get(), av.data(), a_bytes);
    if (b_bytes) memcpy(B.get(), bv.data(), b_bytes);
    std::unique_ptr<uint8_t[]> same(new uint8_t[n + 8]);
    memset(same.get(), 0xA5, n + 8);
    uint32_t status = 0, want_status = 0;
    launch_waves<SYNC_NT>((uint32_t)((n + SYNC_NT / 64 - 1) / (SYNC_NT / 64)),
           [&] { sync_match_kernel(A.get(), a_bytes, a_off.data(), a_len.data(), n, B.get(), b_bytes, b_off.data(), b_len.data(), n_b, cand.data(), same.get(), &status); });
    uint64_t n_same = 0;
    for (uint64_t k = 0; k < n && !fails; k++) {
      uint8_t want = 0;
      const int64_t c = cand[k];
      if (c >= 0) {
        if ((uint64_t)c >= n_b) want_status = 1;
        else if (a_off[k] > a_bytes || a_len[k] > a_bytes - a_off[k] || b_off[c] > b_bytes || b_len[c] > b_bytes - b_off[c]) want_status = 1;
        else want = a_len[k] == b_len[c] && (a_len[k] == 0 || memcmp(A.get() + a_off[k], B.get() + b_off[c], a_len[k]) == 0);
      }
      n_same += want;
      if (same[k] != want) { printf("it %d: record %llu of %llu: same %u, want %u (cand %lld, len %u)\n", it, (unsigned long long)k, (unsigned long long)n, same[k], want, (long long)c, a_len[k]); fails++; }
    }
    for (uint64_t k = n; k < n + 8; k++) if (same[k] != 0xA5) { printf("it %d: same[%llu] behind the array was written\n", it, (unsigned long long)k); fails++; }
    if (status != want_status) { printf("it %d: status %u, want %u\n", it, status, want_status); fails++; }
    if (!fails) printf("it %d ok: n=%llu n_b=%llu same=%llu status=%u\n", it, (unsigned long long)n, (unsigned long long)n_b, (unsigned long long)n_same, status);
  }
  printf(fails ? "FAILED\n" : "ALL OK\n");
  return fails;
}
