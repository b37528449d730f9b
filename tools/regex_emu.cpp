// regex_emu.cpp — the kernels of hmse_amd/csrc/regex_core.h run on the CPU, one std::thread per lane and a barrier for __syncthreads,
// against a brute-force walk of the same automaton.  One source for both forms of the regex search, compiled twice: -DRX_ASSERTING=0 (the
// plain form, tools/regex_emu.py) and -DRX_ASSERTING=1 (with assertions, tools/regexa_emu.py: the walk sees the real context bytes).
// Random corpora (asserting: with newlines, word and other bytes) with tiny and empty chunks, deduplicated into records with junk around
// them in raw, runs of one byte over tile edges, full / short / no hit lists; then place_kernel<8> (hmse_amd/csrc/chunkmap.h) over the
// sorted scan hits and the seams over the same chunk map, and a damaged automaton that the validate kernel must refuse (asserting: one
// per cause).  No GPU: this checks the kernels' LOGIC and their bounds (build it with a sanitizer), not their code objects.  The
// driving script writes the automata (compiled by hmse_amd/regex.py) into a file; the header is included as it is, nothing is cut out.
#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <vector>
#include "hmse.h"
#include "hmse_regexa.h"
#include "hip_on_cpu.h"
#include "chunkmap.h"
constexpr bool RX_A = RX_ASSERTING;
#if RX_ASSERTING
using RxX = struct RxaDev;
#define RX_KERNEL(name) regexa_##name
#else
using RxX = struct RxDev;
#define RX_KERNEL(name) regex_##name
#endif
#include "regex_core.h"
typedef unsigned long long ull;
static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }
#if RX_ASSERTING
static const uint8_t ALPHA[] = {'a', '\n', '-', 'b', ' ', 'c', 'A', '_', 'q', '7'};
static const uint64_t LENGTHS[] = {0, 1, 2, 3, 1, 7, 30, 200, 255, 256, 257, 258, 3000, 40000};      // of the chunks; the last two in long corpora only
#else
static const uint8_t ALPHA[] = {'a', 'b', 'c', '\n', 'A', 'q', ' ', 'B'};
static const uint64_t LENGTHS[] = {0, 1, 2, 3, 1, 7, 30, 200, 255, 256, 257, 3000, 40000};
#endif
constexpr int N_LENGTHS = sizeof LENGTHS / sizeof *LENGTHS;

struct Auto { uint32_t ns, nc, reach, start[4]; std::vector<uint8_t> cm; std::vector<uint16_t> tab; };   // (start: asserting only)
static uint32_t kind(uint8_t b) { return b == '\n' ? 1u : ((b >= '0' && b <= '9') || (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z') || b == '_') ? 2u : 3u; }
// the definition: the text is d[lo, hi); the longest match of 1 .. min(reach, hi - o) bytes from o (asserting: in its context), or 0
static uint32_t walk(const Auto& A, const uint8_t* d, uint64_t lo, uint64_t hi, uint64_t o) {
  uint32_t best = 0;
  if constexpr (RX_A) {
    uint32_t s = A.start[o == lo ? 0u : kind(d[o - 1])];
    for (uint32_t i = 0; i <= A.reach; i++) {
      const uint32_t e = A.tab[s * A.nc + (o + i < hi ? A.cm[d[o + i]] : A.nc - 1)];
      if (i && (e & HMSE_REGEX_ACCEPT)) best = i;
      s = e & 0x7FFFu;
      if (!s || o + i >= hi) break;
    }
  } else {
    uint32_t s = 1;
    for (uint32_t i = 0; i < A.reach && o + i < hi; i++) {
      const uint32_t e = A.tab[s * A.nc + A.cm[d[o + i]]];
      s = e & 0x7FFFu;
      if (!s) break;
      if (e & HMSE_REGEX_ACCEPT) best = i + 1;
    }
  }
  return best;
}
static RxX dev(const Auto& A) {
#if RX_ASSERTING
  return RxaDev{A.tab.data(), A.cm.data(), A.ns, A.nc, A.reach, {A.start[0], A.start[1], A.start[2], A.start[3]}};
#else
  return RxDev{A.tab.data(), A.cm.data(), A.ns, A.nc, A.reach};
#endif
}
// a damaged automaton, one cause per `what`
static Auto damaged(const Auto& A, int what) {
  Auto D = A;
  if (what == 0) D.tab[R(D.tab.size())] = (uint16_t)(D.ns + R(100)) | (R(2) ? 0x8000u : 0u);         // an entry >= n_states
  else if (what == 1) D.tab[R(D.nc)] = R(2) ? 1 : 0x8000u;                                            // a non-zero dead row
  else if constexpr (RX_A) {
    if (what == 2) D.cm[R(256)] = (uint8_t)std::min<uint32_t>(255, D.nc - 1 + R(5));                  // a byte in the EDGE class or beyond
    else if (what == 3) D.cm['a'] = D.cm['\n'];                                                       // a class that mixes kinds
    else D.tab[(1 + R(D.ns - 1)) * D.nc + D.nc - 1] |= 1 + R(D.ns - 1);                               // the EDGE column leads somewhere
  } else {
    D.cm[R(256)] = (uint8_t)std::min<uint32_t>(255, D.nc + R(5));                                     // a byte in no class
    if (D.nc == 256) D = A, D.tab[0] = 1;
  }
  return D;
}

int main(int argc, char** argv) {
  int iters = argc > 1 ? atoi(argv[1]) : 20;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  std::vector<Auto> autos;
  {
    FILE* f = fopen(argc > 3 ? argv[3] : "automata.txt", "r");
    int n = 0;
    if (!f || fscanf(f, "%d", &n) != 1) { printf("no automata\n"); return 2; }
    for (int a = 0; a < n; a++) {
      Auto A; unsigned v;
      if (fscanf(f, "%u %u %u", &A.ns, &A.nc, &A.reach) != 3) return 2;
      for (int i = 0; i < 4; i++) { A.start[i] = 1; if (RX_A && fscanf(f, "%u", &A.start[i]) != 1) return 2; }
      for (int i = 0; i < 256; i++) { if (fscanf(f, "%u", &v) != 1) return 2; A.cm.push_back(v); }
      for (uint32_t i = 0; i < A.ns * A.nc; i++) { if (fscanf(f, "%u", &v) != 1) return 2; A.tab.push_back(v); }
      autos.push_back(A);
    }
    fclose(f);
  }
  int fails = 0, ran = 0;
  for (int it = 0; it < iters && !fails; it++) {
    const Auto& A = autos[it < (int)autos.size() ? it : R(autos.size())];
    const int nalpha = RX_A ? 3 + R(sizeof ALPHA - 2) : 2 + R(sizeof ALPHA - 1);
    uint64_t n = R(3) == 0 ? R(400) : (R(3) == 0 ? RX_TILE + R(RX_TILE) : R(6000));
    std::vector<uint8_t> corpus(n);
    for (auto& c : corpus) c = ALPHA[R(nalpha)];
    if (n > 700 && R(2)) {
      uint64_t o = R(n - 700);
      for (uint64_t i = 0; i < 300 + R(400); i++) corpus[o + i] = RX_A ? (R(8) ? 'a' : "b\n-"[R(3)]) : (R(2) ? 'a' : 'b');
    }
    if (n > RX_TILE + 700 && R(2)) for (uint64_t i = RX_TILE - 300; i < RX_TILE + 300; i++) corpus[i] = 'b';   // a run over a tile edge
    std::vector<uint64_t> cuts{0};
    while (cuts.back() < n) cuts.push_back(std::min(n, cuts.back() + LENGTHS[R(n > 10000 ? N_LENGTHS : N_LENGTHS - 2)]));
    for (int k = R(3); k > 0; k--) cuts.push_back(n);
    const uint64_t n_chunks = cuts.size() - 1;
    std::map<std::string, uint64_t> seen;
    std::vector<std::string> recs;
    std::vector<uint64_t> slot;
    for (uint64_t k = 0; k < n_chunks; k++) {
      std::string c(corpus.begin() + cuts[k], corpus.begin() + cuts[k + 1]);
      auto f = seen.find(c);
      if (f == seen.end()) { seen[c] = recs.size(); slot.push_back(recs.size()); recs.push_back(c); } else slot.push_back(f->second);
    }
    if (R(2)) recs.push_back(std::string(R(50), 'a'));
    const uint64_t lead = R(2) ? R(300) : 0, tail = R(2) ? R(300) : 0;
    std::vector<uint8_t> raw(lead, RX_A ? '\n' : 'a');   // junk in front of the records (asserting: a kernel that looked at it would see a line start)
    std::vector<uint64_t> raw_off{lead};
    for (auto& r : recs) { raw.insert(raw.end(), r.begin(), r.end()); raw_off.push_back(raw.size()); }
    for (uint64_t i = 0; i < tail; i++) raw.push_back(ALPHA[R(nalpha)]);
    const uint64_t raw_bytes = raw.size(), n_rec = recs.size();
    std::vector<uint32_t> mult(n_rec, 0);
    for (auto s : slot) mult[s]++;
    const RxX X = dev(A);
    const uint64_t nv = std::max<uint64_t>({n_rec, n_chunks, (uint64_t)A.ns * A.nc, 256});
    // ---- scan: the scan starts of every record (asserting: the byte in front and the look-ahead byte lie in the record) ----
    std::vector<ull> want;
    ull wc = 0;
    for (uint64_t r = 0; r < n_rec; r++)
      for (uint64_t p = raw_off[r] + RX_A; p + A.reach + RX_A <= raw_off[r + 1]; p++) {
        const uint32_t l = walk(A, raw.data(), raw_off[r], raw_off[r + 1], p);
        if (l) { want.push_back((p << 8) | (l - 1)); wc += mult[r]; }
      }
    const uint64_t cap = R(3) == 0 ? 0 : (R(2) ? want.size() : R(want.size() + 1));
    std::vector<ull> hits(cap + 8, ~0ull);
    ull nh = 0, cnt = 0; uint32_t status = 0;
    launch_block<RX_NT>(2, [&] { RX_KERNEL(validate_kernel)(raw_off.data(), n_rec, raw_bytes, nullptr, nullptr, 0, X, nv, &status); });
    if (status) { printf("it %d: validate status %u\n", it, status); fails++; break; }
    const uint64_t n_tiles = (raw_bytes + RX_TILE - 1) / RX_TILE;
    auto scan = [&](const RxX& G, ull* h, uint64_t c, ull* pn, ull* cn, uint32_t* st) {
      launch_block<RX_NT>((uint32_t)std::min<uint64_t>(n_tiles, 1 + R(2)), [&] { RX_KERNEL(scan_kernel)(raw.data(), raw_bytes, raw_off.data(), n_rec, mult.data(), G, c ? h : nullptr, c, pn, cn, st, n_tiles); });
    };
    if (n_rec && raw_bytes) scan(X, hits.data(), cap, &nh, &cnt, &status);
    bool ok = nh == want.size() && cnt == wc && ((status & 1) != 0) == (cap && want.size() > cap) && !(status & 6);
    for (uint64_t i = cap; i < cap + 8; i++) ok = ok && hits[i] == ~0ull;
    std::vector<ull> got(hits.begin(), hits.begin() + std::min<uint64_t>(cap, nh));
    std::sort(got.begin(), got.end());
    if (cap >= want.size() && cap) ok = ok && got == want;
    else for (auto g : got) ok = ok && std::binary_search(want.begin(), want.end(), g);
    if (!ok) { printf("it %d: SCAN mismatch n=%llu reach=%u nh=%llu want=%zu cnt=%llu/%llu status=%u cap=%llu\n", it, (ull)n, A.reach, nh, want.size(), cnt, wc, status, (ull)cap); fails++; break; }
    // ---- a damaged automaton: refused by the validate kernel, the scan behind it writes nothing (asserting: five causes, the first
    //      five cases take them in turn; plain: three) ----
    if (n_rec && raw_bytes) {
      const int what = RX_A ? (it < 5 ? it : (int)R(5)) : (int)R(3);
      const Auto D = damaged(A, what);
      const RxX Y = dev(D);
      uint32_t st = 0; ull dn = 0, dc = 0;
      std::vector<ull> dh(want.size() + 8, ~0ull);
      launch_block<RX_NT>(1, [&] { RX_KERNEL(validate_kernel)(raw_off.data(), n_rec, raw_bytes, nullptr, nullptr, 0, Y, nv, &st); });
      scan(Y, dh.data(), want.size(), &dn, &dc, &st);
      bool dok = st == 4 && dn == 0 && dc == 0;
      for (auto v : dh) dok = dok && v == ~0ull;
      if (!dok) { printf("it %d: DAMAGED automaton (%d) not refused: status=%u nh=%llu\n", it, what, st, dn); fails++; break; }
    }
    // ---- the corpus: scan starts placed + seam starts = every occurrence once.  A seam start: plain, fewer than reach bytes of its chunk
    //      lie behind it; asserting, the chunk's first start and its last `reach` ones ----
    std::vector<ull> win, wseam;
    for (uint64_t k = 0; k < n_chunks; k++)
      for (uint64_t o = cuts[k]; o < cuts[k + 1]; o++) {
        const uint32_t l = walk(A, corpus.data(), 0, n, o);
        const bool seam = RX_A ? o == cuts[k] || cuts[k + 1] - o <= A.reach : cuts[k + 1] - o < A.reach;
        if (l) (seam ? wseam : win).push_back((o << 8) | (l - 1));
      }
    if (n_chunks) {
      const uint64_t scap = R(4) == 0 ? R(wseam.size() + 1) : wseam.size();
      std::vector<ull> sh(scap + 8, ~0ull);
      ull snh = 0, sc = 0; status = 0;
      launch_block<RX_NT>(2, [&] { RX_KERNEL(validate_kernel)(raw_off.data(), n_rec, raw_bytes, cuts.data(), slot.data(), n_chunks, X, nv, &status); });
      if (status) { printf("it %d: validate(seams) status %u\n", it, status); fails++; break; }
      if (RX_A || A.reach > 1) {                         // (as the entry point: plain, reach = 1 has no seam start)
        const uint64_t nt = n_chunks * (RX_A ? A.reach + 1 : A.reach - 1);
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nt + RX_NT - 1) / RX_NT, 1 + R(3));
        launch_block<RX_NT>(grid, [&] { RX_KERNEL(seams_kernel)(raw.data(), raw_off.data(), cuts.data(), slot.data(), n_chunks, X, scap ? sh.data() : nullptr, scap, &snh, &sc, &status, nt); });
      }
      std::vector<ull> gs(sh.begin(), sh.begin() + std::min<uint64_t>(snh, scap));
      std::sort(gs.begin(), gs.end());
      bool sok = snh == wseam.size() && sc == snh && ((status & 1) != 0) == (scap && wseam.size() > scap) && !(status & 6);
      if (scap >= wseam.size()) sok = sok && (scap == 0 || gs == wseam);
      else for (auto g : gs) sok = sok && std::binary_search(wseam.begin(), wseam.end(), g);
      for (uint64_t i = scap; i < scap + 8; i++) sok = sok && sh[i] == ~0ull;
      if (!sok) { printf("it %d: SEAMS mismatch n=%llu chunks=%llu reach=%u got=%llu want=%zu status=%u\n", it, (ull)n, (ull)n_chunks, A.reach, snh, wseam.size(), status); fails++; break; }
      // place (needs the full sorted scan list): place_kernel<8> passes the low byte through
      std::vector<uint64_t> per(n_rec, 0), chunk_out{0};
      for (auto w : want) { uint64_t r = std::upper_bound(raw_off.begin(), raw_off.end(), w >> 8) - raw_off.begin() - 1; per[r]++; }
      for (uint64_t k = 0; k < n_chunks; k++) chunk_out.push_back(chunk_out.back() + per[slot[k]]);
      const uint64_t total = chunk_out.back();
      std::vector<ull> out(total + 8, ~0ull);
      status = 0;
      launch_block<RX_NT>((uint32_t)std::max<uint64_t>(1, (total + RX_NT - 1) / RX_NT), [&] { place_kernel<8, RX_NT>(want.data(), want.size(), raw_off.data(), cuts.data(), slot.data(), n_chunks, chunk_out.data(), out.data(), total, &status); });
      bool pok = status == 0 && total == win.size() && total == wc;
      for (uint64_t i = 0; pok && i < total; i++) pok = out[i] == win[i];
      for (uint64_t i = total; i < total + 8; i++) pok = pok && out[i] == ~0ull;
      if (!pok) { printf("it %d: PLACE mismatch total=%llu want=%zu status=%u\n", it, (ull)total, win.size(), status); fails++; break; }
    }
    ran++;
    printf("it %d ok: n=%llu rec=%llu chunks=%llu reach=%u scan=%zu seam=%zu\n", it, (ull)n, (ull)n_rec, (ull)n_chunks, A.reach, want.size(), wseam.size());
  }
  printf("%d cases ran\n", ran);
  printf(fails ? "FAILED\n" : "ALL OK\n");
  return fails;
}
