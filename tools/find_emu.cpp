// find_emu.cpp — the kernels of hmse_amd/csrc/find.hip run on the CPU, one std::thread per lane and a barrier for __syncthreads, against a
// brute-force search: random corpora with tiny and empty chunks, deduplicated into records with junk around them in raw, 1..32 patterns of
// 1..256 bytes, both filters, both case modes, full / short / no hit lists; then seams and place over the same chunk map.  No GPU: this
// checks the kernels' LOGIC and their bounds (build it with a sanitizer), not their code objects.  Driven by tools/find_emu.py, which cuts
// the kernels out of find.hip (everything in front of its entry points) into find_kernels.inc; the validate and place kernels come
// from hmse_amd/csrc/chunkmap.h, included as it is.
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
#include "hip_on_cpu.h"
#include "chunkmap.h"
#include "find_kernels.inc"
typedef unsigned long long ull;
static uint32_t foldb(uint32_t b) { return (b >= 'A' && b <= 'Z') ? b + 32 : b; }
static bool eq(const uint8_t* a, const uint8_t* b, uint32_t m, bool ic) { for (uint32_t i = 0; i < m; i++) if ((ic ? foldb(a[i]) : a[i]) != (ic ? foldb(b[i]) : b[i])) return false; return true; }

static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }
static const uint8_t ALPHA[] = {'a', 'b', 'A', 'B', 'c', 0xC1, 0xE1, '@', '`', 'Z', 'z', '[', '{'};

static FindPats mkpats(const std::vector<std::string>& ps, std::vector<uint8_t>& flat, uint32_t lead) {
  FindPats P; memset(&P, 0, sizeof P);
  flat.assign(lead, 7);
  P.n = ps.size(); P.max_len = 0; P.off[0] = lead;
  for (size_t j = 0; j < ps.size(); j++) { flat.insert(flat.end(), ps[j].begin(), ps[j].end()); P.off[j + 1] = flat.size(); P.max_len = std::max<uint32_t>(P.max_len, ps[j].size()); }
  for (size_t j = ps.size() + 1; j <= HMSE_FIND_MAX_PATTERNS; j++) P.off[j] = P.off[ps.size()];
  return P;
}

int main(int argc, char** argv) {
  int iters = argc > 1 ? atoi(argv[1]) : 30;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  int fails = 0;
  for (int it = 0; it < iters && !fails; it++) {
    const bool ic = R(2);
    const int nalpha = 2 + R(sizeof ALPHA - 1);
    // corpus and chunk map
    uint64_t n = R(3) == 0 ? R(400) : (R(3) == 0 ? FIND_TILE + R(FIND_TILE * 2) : R(5000));
    std::vector<uint8_t> corpus(n);
    for (auto& c : corpus) c = ALPHA[R(nalpha)];
    std::vector<uint64_t> cuts{0};
    while (cuts.back() < n) {
      static const uint64_t L[] = {0, 1, 2, 3, 1, 7, 30, 200, 3000, 40000};
      uint64_t l = L[R(n > 10000 ? 10 : 8)];
      cuts.push_back(std::min(n, cuts.back() + l));
    }
    for (int k = R(3); k > 0; k--) cuts.push_back(n);
    const uint64_t n_chunks = cuts.size() - 1;
    // dedupe to records, with junk in front of / behind the records in raw
    std::map<std::string, uint64_t> seen;
    std::vector<std::string> recs;
    std::vector<uint64_t> slot;
    for (uint64_t k = 0; k < n_chunks; k++) {
      std::string c(corpus.begin() + cuts[k], corpus.begin() + cuts[k + 1]);
      auto f = seen.find(c);
      if (f == seen.end()) { seen[c] = recs.size(); slot.push_back(recs.size()); recs.push_back(c); } else slot.push_back(f->second);
    }
    if (R(2)) recs.push_back(std::string(R(50), 'a'));   // a record no chunk names
    const uint64_t lead = R(2) ? R(300) : 0, tail = R(2) ? R(300) : 0;
    std::vector<uint8_t> raw(lead, 'a');
    std::vector<uint64_t> raw_off{lead};
    for (auto& r : recs) { raw.insert(raw.end(), r.begin(), r.end()); raw_off.push_back(raw.size()); }
    for (uint64_t i = 0; i < tail; i++) raw.push_back(ALPHA[R(nalpha)]);
    const uint64_t raw_bytes = raw.size(), n_rec = recs.size();
    raw.resize(raw_bytes + 64, 'a');                     // readable junk behind raw_bytes: must not matter
    std::vector<uint32_t> mult(n_rec, 0);
    for (auto s : slot) mult[s]++;
    // patterns
    const uint32_t np = R(3) == 0 ? 1 + R(4) : 1 + R(32);
    std::vector<std::string> ps;
    for (uint32_t j = 0; j < np; j++) {
      static const uint32_t M[] = {1, 2, 3, 4, 5, 16, 17, 255, 256, 9, 2, 1};
      uint32_t m = M[R(12)];
      std::string p;
      if (n >= m && R(4)) { uint64_t o = R(n - m + 1); p.assign(corpus.begin() + o, corpus.begin() + o + m); }
      else for (uint32_t i = 0; i < m; i++) p.push_back(ALPHA[R(nalpha)]);
      if (ic) for (auto& ch : p) if (R(2)) ch = (ch >= 'a' && ch <= 'z') ? ch - 32 : (ch >= 'A' && ch <= 'Z') ? ch + 32 : ch;
      ps.push_back(p);
    }
    std::vector<uint8_t> flat;
    FindPats P = mkpats(ps, flat, R(2) ? R(20) : 0);
    // ---- scan ----
    std::vector<std::pair<uint64_t, uint32_t>> want;
    std::vector<ull> wc(np, 0);
    for (uint64_t r = 0; r < n_rec; r++)
      for (uint32_t j = 0; j < np; j++) {
        uint32_t m = ps[j].size();
        for (uint64_t p = raw_off[r]; p + m <= raw_off[r + 1]; p++)
          if (eq(&raw[p], (const uint8_t*)ps[j].data(), m, ic)) { want.push_back({p, j}); wc[j] += mult[r]; }
      }
    std::sort(want.begin(), want.end());
    const uint64_t cap = R(3) == 0 ? 0 : (R(2) ? want.size() : R(want.size() + 1));
    std::vector<ull> hits(cap + 8, ~0ull), counts(np, 0);
    ull nh = 0; uint32_t status = 0;
    launch_block<FIND_NT>(1, [&] { tables_validate_kernel<FIND_NT>(raw_off.data(), n_rec, raw_bytes, nullptr, nullptr, 0, nullptr, &status); });
    if (status) { printf("it %d: validate status %u\n", it, status); fails++; break; }
    if (n_rec && raw_bytes) {
      const uint64_t n_tiles = (raw_bytes + FIND_TILE - 1) / FIND_TILE;
      const uint32_t grid = (uint32_t)std::min<uint64_t>(n_tiles, 1 + R(3));
      const bool few = np <= FIND_FEW;
      auto call = [&](auto F, auto I) { launch_block<FIND_NT>(grid, [&] { find_scan_kernel<decltype(F)::value, decltype(I)::value>(raw.data(), raw_bytes, raw_off.data(), n_rec, mult.data(), flat.data(), P, cap ? hits.data() : nullptr, cap, &nh, counts.data(), &status, n_tiles); }); };
      if (few) { if (ic) call(std::true_type{}, std::true_type{}); else call(std::true_type{}, std::false_type{}); }
      else { if (ic) call(std::false_type{}, std::true_type{}); else call(std::false_type{}, std::false_type{}); }
    }
    bool ok = nh == want.size() && counts == wc && ((status & 1) != 0) == (cap && want.size() > cap);
    for (uint64_t i = cap; i < cap + 8; i++) ok = ok && hits[i] == ~0ull;
    std::vector<std::pair<uint64_t, uint32_t>> got;
    for (uint64_t i = 0; i < std::min<uint64_t>(cap, nh); i++) got.push_back({hits[i] >> 8, (uint32_t)(hits[i] & 255)});
    std::sort(got.begin(), got.end());
    if (cap >= want.size() && cap) ok = ok && got == want;
    else for (auto& g : got) ok = ok && std::binary_search(want.begin(), want.end(), g);
    if (!ok) { printf("it %d: SCAN mismatch n=%llu np=%u ic=%d nh=%llu want=%zu status=%u cap=%llu\n", it, (ull)n, np, ic, nh, want.size(), status, (ull)cap); fails++; break; }
    // ---- seams and place ----
    std::vector<std::pair<uint64_t, uint32_t>> win, wseam;
    for (uint32_t j = 0; j < np; j++) {
      uint32_t m = ps[j].size();
      for (uint64_t o = 0; o + m <= n; o++)
        if (eq(&corpus[o], (const uint8_t*)ps[j].data(), m, ic)) {
          uint64_t k = std::upper_bound(cuts.begin(), cuts.end(), o) - cuts.begin() - 1;
          (o + m <= cuts[k + 1] ? win : wseam).push_back({o, j});
        }
    }
    std::sort(win.begin(), win.end()); std::sort(wseam.begin(), wseam.end());
    if (n_chunks) {
      std::vector<ull> sh(wseam.size() + 8, ~0ull), sc(np, 0);
      ull snh = 0; status = 0;
      launch_block<FIND_NT>(2, [&] { tables_validate_kernel<FIND_NT>(raw_off.data(), n_rec, raw_bytes, cuts.data(), slot.data(), n_chunks, nullptr, &status); });
      if (status) { printf("it %d: validate(seams) status %u\n", it, status); fails++; break; }
      if (P.max_len >= 2) {
        const uint64_t nt = n_chunks * (P.max_len - 1);
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nt + FIND_NT - 1) / FIND_NT, 1 + R(3));
        if (ic) launch_block<FIND_NT>(grid, [&] { find_seams_kernel<true>(raw.data(), raw_off.data(), cuts.data(), slot.data(), n_chunks, flat.data(), P, sh.data(), wseam.size(), &snh, sc.data(), &status, nt); });
        else launch_block<FIND_NT>(grid, [&] { find_seams_kernel<false>(raw.data(), raw_off.data(), cuts.data(), slot.data(), n_chunks, flat.data(), P, sh.data(), wseam.size(), &snh, sc.data(), &status, nt); });
      }
      std::vector<std::pair<uint64_t, uint32_t>> gs;
      for (uint64_t i = 0; i < std::min<uint64_t>(snh, wseam.size()); i++) gs.push_back({sh[i] >> 8, (uint32_t)(sh[i] & 255)});
      std::sort(gs.begin(), gs.end());
      if (snh != wseam.size() || gs != wseam || status) { printf("it %d: SEAMS mismatch n=%llu chunks=%llu np=%u ic=%d got=%llu want=%zu status=%u\n", it, (ull)n, (ull)n_chunks, np, ic, snh, wseam.size(), status); fails++; break; }
      // place (needs the full sorted scan list)
      std::vector<ull> hs;
      for (auto& w : want) hs.push_back((w.first << 8) | w.second);
      std::vector<uint64_t> chunk_out{0};
      for (uint64_t k = 0; k < n_chunks; k++) {
        uint64_t c = 0;
        for (auto& w : want) c += w.first >= raw_off[slot[k]] && w.first < raw_off[slot[k] + 1];
        chunk_out.push_back(chunk_out.back() + c);
      }
      const uint64_t total = chunk_out.back();
      std::vector<ull> out(total + 8, ~0ull);
      status = 0;
      launch_block<FIND_NT>(1, [&] { tables_validate_kernel<FIND_NT>(raw_off.data(), n_rec, ~0ull, cuts.data(), slot.data(), n_chunks, chunk_out.data(), &status); });
      launch_block<FIND_NT>((uint32_t)std::max<uint64_t>(1, (total + FIND_NT - 1) / FIND_NT), [&] { place_kernel<8, FIND_NT>(hs.data(), hs.size(), raw_off.data(), cuts.data(), slot.data(), n_chunks, chunk_out.data(), out.data(), total, &status); });
      bool pok = status == 0 && total == win.size();
      for (uint64_t i = 0; pok && i < total; i++) pok = (out[i] >> 8) == win[i].first && (out[i] & 255) == win[i].second;
      for (uint64_t i = total; i < total + 8; i++) pok = pok && out[i] == ~0ull;
      if (!pok) { printf("it %d: PLACE mismatch total=%llu want=%zu status=%u\n", it, (ull)total, win.size(), status); fails++; break; }
    }
    printf("it %d ok: n=%llu rec=%llu chunks=%llu np=%u ic=%d scan=%zu seam=%zu\n", it, (ull)n, (ull)n_rec, (ull)n_chunks, np, ic, want.size(), wseam.size());
  }
  printf(fails ? "FAILED\n" : "ALL OK\n");
  return fails;
}
