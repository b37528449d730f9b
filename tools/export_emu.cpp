// export_emu.cpp — the kernels of hmse_amd/csrc/export.hip run on the CPU, one std::thread per lane and a std::barrier under
// __syncthreads, against the definitions of include/hmse.h: the CRC-32 bit by bit (checked first against known answers that
// tools/export_emu.py takes from zlib), the combination by an independently written modular product, the members byte by byte.
// Ranges of every length around the strip sizes (64 * 16 k bytes) and the tile size (8192), empty ranges, odd starts, junk in front of
// and behind the data, contents random / 0x00 / 0xFF, every table and buffer a heap block of exactly the declared size (a sanitizer sees
// a read one byte outside), outputs that start poisoned with a guard behind them, refused calls that must write nothing.  No GPU: this
// checks the kernels' LOGIC and bounds (build it with a sanitizer), not their code object.  Driven by tools/export_emu.py, which cuts
// the kernels out of export.hip (everything between the geometry constants and the entry points) into export_kernels.inc;
// wave_copy comes from hmse_amd/csrc/blockops.h as it is.
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
#include "blockops.h"
#include "export_kernels.inc"

static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }
template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a heap block of exactly v.size() elements
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

// ---- the definitions ----
static uint32_t crc_ref(const uint8_t* p, uint64_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint64_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int b = 0; b < 8; b++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return ~c;
}
// the product modulo the polynomial, term by term of a (bit 31 = x^0)
static uint32_t mul_ref(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
// x^(8 n): x^8 squared along the bits of n
static uint32_t xpow8_ref(uint64_t n) {
  uint32_t sq = 1u << 23, p = 1u << 31;               // x^8, x^0
  for (; n; n >>= 1) { if (n & 1) p = mul_ref(p, sq); sq = mul_ref(sq, sq); }
  return p;
}

static int known_answers(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { printf("no known answers at %s\n", path); return 1; }
  int n = 0, bad = 0;
  uint32_t len, want;
  while (fread(&len, 4, 1, f) == 1) {
    std::vector<uint8_t> b(len);
    if ((len && fread(b.data(), 1, len, f) != len) || fread(&want, 4, 1, f) != 1) { bad++; break; }
    bad += crc_ref(b.data(), len) != want;
    n++;
  }
  fclose(f);
  printf("known answers (zlib): %d, %d wrong\n", n, bad);
  return bad || n == 0;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 12;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  int fails = argc > 3 ? known_answers(argv[3]) : 0;
  static const uint64_t LENS[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 7167, 7168, 7169,
                                  8191, 8192, 8193, 8194, 16383, 16384, 16385, 24576 + 5, 32767, 32768, 40001};
  const int n_lens = (int)(sizeof LENS / sizeof *LENS);
  uint64_t n_ranges = 0, n_comb = 0, n_mem = 0;
  for (int it = 0; it < iters && !fails; it++) {
    // ---- hmse_crc32 ----
    {
      const int fill = (int)R(4);                        // 0, 1: random, 2: 0x00, 3: 0xFF
      const uint64_t n_chunks = R(8) == 0 ? 0 : 1 + R(9);
      std::vector<uint64_t> cuts{R(20)};                 // junk in front: odd starts
      for (uint64_t k = 0; k < n_chunks; k++) {
        uint64_t l = R(3) == 0 ? R(3000) : LENS[(it * 7 + k * 3 + R(2)) % n_lens];
        if (R(6) == 0) l = 0;
        cuts.push_back(cuts.back() + l);
      }
      const uint64_t n = cuts.back() + R(20);            // and behind
      std::vector<uint8_t> data(n);
      for (auto& x : data) x = fill == 2 ? 0x00 : fill == 3 ? 0xFF : (uint8_t)R(256);
      for (uint64_t p = 0; p < cuts[0]; p++) data[p] = (uint8_t)(0x11 + R(200));
      for (uint64_t p = cuts.back(); p < n; p++) data[p] = (uint8_t)(0x11 + R(200));
      std::vector<uint32_t> want(n_chunks);
      for (uint64_t k = 0; k < n_chunks; k++) want[k] = crc_ref(data.data() + cuts[k], cuts[k + 1] - cuts[k]);
      int broken = 0;
      if (n_chunks >= 2 && R(6) == 0) {
        broken = 1 + (int)R(2);
        if (broken == 1) { const uint64_t k = 1 + R(n_chunks - 1); cuts[k] = cuts[k + 1] + 1 + R(5); if (k == n_chunks) broken = 2; }
        if (broken == 2) cuts[n_chunks] = n + 1 + R(1000);
      }
      auto D = exact(data); auto CU = exact(cuts);
      std::vector<uint32_t> out(n_chunks + 2, 0xA5A5A5A5u);
      auto OUT = exact(out);
      uint32_t status = 0;
      if (n_chunks) {
        launch_block<EX_CNT>(1 + (uint32_t)R(2), [&] { crc32_validate_kernel(CU.get(), n_chunks, n, &status); });
        launch_block<EX_NT>(1 + (uint32_t)R(n_chunks < 3 ? n_chunks : 3), [&] { crc32_kernel(D.get(), CU.get(), n_chunks, OUT.get(), &status); });
      }
      if (status != (broken ? 1u : 0u)) { printf("it %d: crc status %u (broken %d)\n", it, status, broken); fails++; }
      for (uint64_t k = 0; k < n_chunks + 2 && !fails; k++) {
        const uint32_t w = (k < n_chunks && !broken) ? want[k] : 0xA5A5A5A5u;
        if (OUT[k] != w) {
          printf("it %d: crc[%llu] = %08x, want %08x (start %llu, len %llu, fill %d, broken %d)\n", it, (unsigned long long)k, OUT[k], w,
                 (unsigned long long)cuts[k < n_chunks ? k : 0], (unsigned long long)(k < n_chunks ? cuts[k + 1] - cuts[k] : 0), fill, broken);
          fails++;
        }
      }
      n_ranges += n_chunks;
    }
    // ---- hmse_crc32_combine ----
    {
      const uint64_t n = 1 + R(700);
      const bool huge = R(2);                            // fabricated lengths above 2^32: exponents only
      std::vector<uint32_t> crc(n);
      std::vector<uint64_t> len(n);
      std::vector<uint8_t> all;
      uint32_t want = 0;
      for (uint64_t k = 0; k < n; k++) {
        if (huge) { crc[k] = (uint32_t)rng(); len[k] = R(5) == 0 ? 0 : R(1ull << (20 + R(30))); }
        else {
          len[k] = R(4) == 0 ? 0 : R(40);
          const size_t o = all.size();
          for (uint64_t b = 0; b < len[k]; b++) all.push_back((uint8_t)R(256));
          crc[k] = crc_ref(all.data() + o, len[k]);
        }
      }
      if (huge) {
        uint64_t behind = 0;
        for (uint64_t k = n; k-- > 0;) { want ^= mul_ref(crc[k], xpow8_ref(behind)); behind += len[k]; }
      } else want = crc_ref(all.data(), all.size());
      auto CR = exact(crc); auto LE = exact(len);
      uint32_t out[2] = {0, 0xA5A5A5A5u};                // (the entry point clears out[0])
      launch_block<EX_CNT>((uint32_t)((n + EX_CNT - 1) / EX_CNT), [&] { crc32_combine_kernel(CR.get(), LE.get(), n, out); });
      if (out[0] != want || out[1] != 0xA5A5A5A5u) { printf("it %d: combine of %llu (huge %d) = %08x, want %08x\n", it, (unsigned long long)n, (int)huge, out[0], want); fails++; }
      n_comb += n;
    }
    // ---- hmse_gzip_members ----
    {
      const uint32_t flags = R(2) ? HMSE_GZIP_BGZF : 0u;
      const uint64_t H = flags ? 18 : 10;
      const uint64_t n_rec = 1 + R(6), n_chunks = 1 + R(9);
      std::vector<uint8_t> src[2];
      std::vector<uint64_t> src_off(n_rec), stream_len(n_rec), raw_off{R(50)}, slot(n_chunks), member_off{R(30)};
      std::vector<uint8_t> sel(n_rec);
      std::vector<uint32_t> crc(n_rec);
      for (int s = 0; s < 2; s++) for (uint64_t g = R(20); g > 0; g--) src[s].push_back((uint8_t)R(256));
      for (uint64_t r = 0; r < n_rec; r++) {
        sel[r] = (uint8_t)R(2);
        auto& S = src[sel[r]];
        src_off[r] = S.size();
        stream_len[r] = R(5) == 0 ? R(3) : 1 + R(300);
        for (uint64_t b = 0; b < stream_len[r]; b++) S.push_back((uint8_t)R(256));
        for (uint64_t g = R(4); g > 0; g--) S.push_back((uint8_t)R(256));
        crc[r] = (uint32_t)rng();
        raw_off.push_back(raw_off.back() + R(40000));
      }
      for (uint64_t i = 0; i < n_chunks; i++) { slot[i] = R(n_rec); member_off.push_back(member_off.back() + H + stream_len[slot[i]] + 8); }
      uint64_t dst_bytes = member_off.back();
      std::vector<uint8_t> want(dst_bytes, 0xA5);
      for (uint64_t i = 0; i < n_chunks; i++) {
        const uint64_t r = slot[i], sl = stream_len[r];
        uint8_t* m = want.data() + member_off[i];
        static const uint8_t G[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff}, B[8] = {6, 0, 0x42, 0x43, 2, 0, 0, 0};
        memcpy(m, G, 10);
        if (flags) { m[3] = 4; memcpy(m + 10, B, 8); const uint64_t bs = H + sl + 8 - 1; m[16] = (uint8_t)bs; m[17] = (uint8_t)(bs >> 8); }
        memcpy(m + H, src[sel[r]].data() + src_off[r], sl);
        const uint32_t rl = (uint32_t)(raw_off[r + 1] - raw_off[r]);
        for (int b = 0; b < 4; b++) { m[H + sl + b] = (uint8_t)(crc[r] >> (8 * b)); m[H + sl + 4 + b] = (uint8_t)(rl >> (8 * b)); }
      }
      uint32_t want_status = 0;
      const int refuse = R(4) == 0 ? 1 + (int)R(5) : 0;
      if (refuse == 1) { slot[R(n_chunks)] = n_rec + R(3); want_status = 1; }
      if (refuse == 2) { const uint64_t r = slot[R(n_chunks)]; src_off[r] = src[sel[r]].size() - stream_len[r] + 1; want_status = 1; }
      if (refuse == 3) { dst_bytes -= 1; want_status = 1; }
      if (refuse == 4) { member_off[n_chunks] += 1; dst_bytes += 1; want_status = 1; }
      if (refuse == 5) { const uint64_t r = slot[R(n_chunks)]; raw_off[r + 1] = raw_off[r] + (1ull << 32); want_status = 1;
                         for (uint64_t q = r + 2; q <= n_rec; q++) raw_off[q] += 1ull << 32; }
      auto S0 = exact(src[0]); auto S1 = exact(src[1]); auto SO = exact(src_off); auto SLn = exact(stream_len); auto SE = exact(sel);
      auto CR = exact(crc); auto RO = exact(raw_off); auto SL = exact(slot); auto MO = exact(member_off);
      std::unique_ptr<uint8_t[]> DST(new uint8_t[dst_bytes + 1]);
      memset(DST.get(), 0xA5, dst_bytes + 1);
      uint32_t status = 0;
      launch_block<EX_CNT>(1, [&] {
        gzip_validate_kernel(src[0].size(), src[1].size(), SO.get(), SLn.get(), SE.get(), RO.get(), n_rec, SL.get(), n_chunks, MO.get(), flags, dst_bytes, &status);
      });
      launch_block<EX_CNT>((uint32_t)((n_chunks + EX_CNT / 64 - 1) / (EX_CNT / 64)), [&] {
        gzip_members_kernel(S0.get(), S1.get(), SO.get(), SLn.get(), SE.get(), CR.get(), RO.get(), SL.get(), n_chunks, MO.get(), flags, DST.get(), &status);
      });
      if (status != want_status) { printf("it %d: members status %u, want %u (refuse %d)\n", it, status, want_status, refuse); fails++; }
      for (uint64_t k = 0; k < dst_bytes + 1 && !fails; k++) {
        const uint8_t w = (!want_status && k < want.size()) ? want[k] : 0xA5;
        if (DST[k] != w) { printf("it %d: dst[%llu] = %u, want %u (flags %u, refuse %d)\n", it, (unsigned long long)k, DST[k], w, flags, refuse); fails++; }
      }
      n_mem += n_chunks;
    }
    if (!fails && (it % 10 == 9 || it + 1 == iters))
      printf("it %d ok: %llu ranges, %llu combined entries, %llu members so far\n", it, (unsigned long long)n_ranges, (unsigned long long)n_comb, (unsigned long long)n_mem);
  }
  // a BGZF member above 65536 bytes: status bit 1, nothing written
  if (!fails) {
    const uint64_t sl = 65536, n_rec = 1;
    std::vector<uint8_t> s0(sl, 7);
    uint64_t src_off = 0, raw_off[2] = {0, 5}, slot = 0, member_off[2] = {0, 18 + sl + 8};
    uint8_t sel = 0; uint32_t crc = 1, status = 0;
    std::vector<uint8_t> dst(member_off[1], 0xA5);
    launch_block<EX_CNT>(1, [&] { gzip_validate_kernel(sl, 0, &src_off, &sl, &sel, raw_off, n_rec, &slot, 1, member_off, HMSE_GZIP_BGZF, member_off[1], &status); });
    launch_block<EX_CNT>(1, [&] { gzip_members_kernel(s0.data(), nullptr, &src_off, &sl, &sel, &crc, raw_off, &slot, 1, member_off, HMSE_GZIP_BGZF, dst.data(), &status); });
    bool clean = true;
    for (auto b : dst) clean &= b == 0xA5;
    if (status != 2u || !clean) { printf("a BGZF member of %llu bytes: status %u, clean %d\n", (unsigned long long)member_off[1], status, (int)clean); fails++; }
  }
  printf(fails ? "FAILED\n" : "ALL OK: %llu ranges, %llu combined entries and %llu members equal the definition\n", (unsigned long long)n_ranges,
         (unsigned long long)n_comb, (unsigned long long)n_mem);
  return fails;
}
