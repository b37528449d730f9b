// findset_emu.cpp — the kernels of hmse_amd/csrc/findset.hip run on the CPU, one std::thread per lane and a barrier for __syncthreads,
// against a brute-force search: random corpora with tiny and empty chunks, deduplicated into records with junk around them in raw, sets of
// 1..300 patterns of 4..256 bytes (nested prefixes, shared keys), both case modes, full / short / no hit lists; then seams and place over
// the same chunk map, and a damaged set that the validate kernel must refuse.  No GPU: this checks the kernels' LOGIC and their bounds
// (build it with a sanitizer), not their code objects.  Driven by tools/findset_emu.py, which cuts the kernels out of findset.hip
// (everything in front of its entry points) into findset_kernels.inc; the table rules and the place kernel come from
// hmse_amd/csrc/chunkmap.h, included as it is.
#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <random>
#include <set>
#include <string>
#include <thread>
#include <tuple>
#include <vector>
#include "hmse.h"
#include "hip_on_cpu.h"
#include "chunkmap.h"
#include "findset_kernels.inc"
typedef unsigned long long ull;
static uint32_t foldb(uint32_t b) { return (b >= 'A' && b <= 'Z') ? b + 32 : b; }
static bool eq(const uint8_t* a, const uint8_t* b, uint32_t m, bool ic) { for (uint32_t i = 0; i < m; i++) if ((ic ? foldb(a[i]) : a[i]) != (ic ? foldb(b[i]) : b[i])) return false; return true; }

static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }
static const uint8_t ALPHA[] = {'a', 'b', 'A', 'B', 'c', 0xC1, 0xE1, '@', '`', 'Z', 'z', '[', '{'};

// The compiled set, as include/hmse.h describes it (what hmse_amd/find.py PatternSet builds with numpy).
struct Set {
  std::vector<uint8_t> upat; std::vector<uint32_t> uoff, ukey, uid, dir, bitmap;
  FsetDev F;
};
static void build(const std::vector<std::string>& ps, bool ic, Set& S) {
  std::vector<std::tuple<uint32_t, uint32_t, uint32_t, std::string, uint32_t>> e;
  uint32_t max_len = 0;
  for (uint32_t j = 0; j < ps.size(); j++) {
    uint32_t key; memcpy(&key, ps[j].data(), 4);
    e.push_back({key * HMSE_FINDSET_HASH, key, (uint32_t)ps[j].size(), ps[j], j});
    max_len = std::max<uint32_t>(max_len, ps[j].size());
  }
  std::sort(e.begin(), e.end());
  uint32_t bits = 1;
  while ((1ull << bits) < 2 * e.size()) bits++;
  S.upat.clear(); S.uoff.assign(1, 0); S.ukey.clear(); S.uid.clear();
  S.dir.assign((1u << bits) + 1, 0); S.bitmap.assign(1u << (HMSE_FINDSET_BITMAP_BITS - 5), 0);
  for (auto& [h, key, m, s, j] : e) {
    S.upat.insert(S.upat.end(), s.begin(), s.end()); S.uoff.push_back(S.upat.size()); S.ukey.push_back(key); S.uid.push_back(j);
    S.dir[(h >> (32 - bits)) + 1]++;
    S.bitmap[(h >> 13) >> 5] |= 1u << ((h >> 13) & 31);
  }
  for (size_t c = 1; c < S.dir.size(); c++) S.dir[c] += S.dir[c - 1];
  S.F = FsetDev{S.upat.data(), S.uoff.data(), S.ukey.data(), S.uid.data(), S.dir.data(), S.bitmap.data(), S.upat.size(), (uint32_t)e.size(),
                (uint32_t)ps.size(), bits, max_len, ic ? 1u : 0u};
}

int main(int argc, char** argv) {
  int iters = argc > 1 ? atoi(argv[1]) : 20;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  int fails = 0, ran = 0;
  const uint64_t IDM = (1ull << HMSE_FINDSET_ID_BITS) - 1;
  for (int it = 0; it < iters && !fails; it++) {
    const bool ic = R(2);
    const int nalpha = 2 + R(sizeof ALPHA - 1);
    // corpus and chunk map
    uint64_t n = R(3) == 0 ? R(400) : (R(4) == 0 ? FSET_TILE + R(FSET_TILE) : R(6000));
    std::vector<uint8_t> corpus(n);
    for (auto& c : corpus) c = ALPHA[R(nalpha)];
    if (n > 600 && R(2)) { uint64_t o = R(n - 600); for (uint64_t i = 0; i < 300 + R(300); i++) corpus[o + i] = 'a'; }   // a run of one byte
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
    // (no readable junk behind raw_bytes: under a sanitizer a read past it is an error)
    std::vector<uint32_t> mult(n_rec, 0);
    for (auto s : slot) mult[s]++;
    // patterns: distinct after folding, 4..256 bytes
    const uint32_t want_np = R(3) == 0 ? 1 + R(4) : 1 + R(300);
    std::set<std::string> uniq;
    for (uint32_t j = 0; j < want_np; j++) {
      static const uint32_t M[] = {4, 5, 16, 17, 255, 256, 9, 6, 4, 7, 8, 12};
      uint32_t m = M[R(12)];
      std::string p;
      if (n >= m && R(4)) { uint64_t o = R(n - m + 1); p.assign(corpus.begin() + o, corpus.begin() + o + m); }
      else for (uint32_t i = 0; i < m; i++) p.push_back(ALPHA[R(nalpha)]);
      if (R(8) == 0) for (uint32_t l = 4; l < m; l += 1 + R(5)) { std::string q = p.substr(0, l); if (ic) for (auto& ch : q) ch = foldb((uint8_t)ch); uniq.insert(q); }   // nested prefixes
      if (ic) for (auto& ch : p) ch = foldb((uint8_t)ch);
      uniq.insert(p);
    }
    std::vector<std::string> ps(uniq.begin(), uniq.end());
    std::shuffle(ps.begin(), ps.end(), rng);
    const uint32_t np = ps.size();
    Set S;
    build(ps, ic, S);
    const FsetDev F = S.F;
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
    const uint64_t nv = std::max<uint64_t>({n_rec, (uint64_t)F.n, 1ull << F.bits});
    launch_block<FSET_NT>(2, [&] { findset_validate_kernel(raw_off.data(), n_rec, raw_bytes, nullptr, nullptr, 0, nullptr, F, nv, &status); });
    if (status) { printf("it %d: validate status %u\n", it, status); fails++; break; }
    const uint64_t n_tiles = (raw_bytes + FSET_TILE - 1) / FSET_TILE;
    auto scan = [&](const FsetDev& G, ull* h, uint64_t c, ull* pn, ull* cn, uint32_t* st) {
      const uint32_t grid = (uint32_t)std::min<uint64_t>(n_tiles, 1 + R(2));
      if (ic) launch_block<FSET_NT>(grid, [&] { findset_scan_kernel<true>(raw.data(), raw_bytes, raw_off.data(), n_rec, mult.data(), G, c ? h : nullptr, c, pn, cn, st, n_tiles); });
      else launch_block<FSET_NT>(grid, [&] { findset_scan_kernel<false>(raw.data(), raw_bytes, raw_off.data(), n_rec, mult.data(), G, c ? h : nullptr, c, pn, cn, st, n_tiles); });
    };
    if (n_rec && raw_bytes) scan(F, hits.data(), cap, &nh, counts.data(), &status);
    bool ok = nh == want.size() && counts == wc && ((status & 1) != 0) == (cap && want.size() > cap);
    for (uint64_t i = cap; i < cap + 8; i++) ok = ok && hits[i] == ~0ull;
    std::vector<std::pair<uint64_t, uint32_t>> got;
    for (uint64_t i = 0; i < std::min<uint64_t>(cap, nh); i++) got.push_back({hits[i] >> HMSE_FINDSET_ID_BITS, (uint32_t)(hits[i] & IDM)});
    std::sort(got.begin(), got.end());
    if (cap >= want.size() && cap) ok = ok && got == want;
    else for (auto& g : got) ok = ok && std::binary_search(want.begin(), want.end(), g);
    if (!ok) { printf("it %d: SCAN mismatch n=%llu np=%u ic=%d nh=%llu want=%zu status=%u cap=%llu\n", it, (ull)n, np, ic, nh, want.size(), status, (ull)cap); fails++; break; }
    // ---- a damaged set: refused by the validate kernel, the scan behind it writes nothing ----
    if (n_rec && raw_bytes && F.n >= 2) {
      Set D = S;
      D.F = FsetDev{D.upat.data(), D.uoff.data(), D.ukey.data(), D.uid.data(), D.dir.data(), D.bitmap.data(), D.upat.size(), F.n, F.n_ids, F.bits, F.max_len, F.folded};
      const int what = R(5);
      const uint32_t i = R(F.n);
      if (what == 0) { D.dir[1 + R(D.dir.size() - 2)] = F.n + 5; }
      else if (what == 1) D.uid[i] = np + R(100);
      else if (what == 2) D.ukey[i] ^= 1u << R(32);
      else if (what == 3) D.uoff[i + 1] = D.uoff[i] + (R(2) ? 3 : 257 + R(1000));
      else D.uoff[F.n] = D.upat.size() + 1 + R(1000);
      uint32_t st = 0; ull dn = 0;
      std::vector<ull> dh(want.size() + 8, ~0ull), dc(np, 0);
      launch_block<FSET_NT>(1, [&] { findset_validate_kernel(raw_off.data(), n_rec, raw_bytes, nullptr, nullptr, 0, nullptr, D.F, nv, &st); });
      scan(D.F, dh.data(), want.size(), &dn, dc.data(), &st);
      bool dok = (st & 2) && dn == 0;
      for (auto v : dh) dok = dok && v == ~0ull;
      for (auto v : dc) dok = dok && v == 0;
      if (!dok) { printf("it %d: DAMAGED set (%d) not refused: status=%u nh=%llu\n", it, what, st, dn); fails++; break; }
    }
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
      const uint64_t scap = R(4) == 0 ? R(wseam.size() + 1) : wseam.size();
      std::vector<ull> sh(scap + 8, ~0ull), sc(np, 0);
      ull snh = 0; status = 0;
      const uint64_t nv2 = std::max<uint64_t>(nv, n_chunks);
      launch_block<FSET_NT>(2, [&] { findset_validate_kernel(raw_off.data(), n_rec, raw_bytes, cuts.data(), slot.data(), n_chunks, nullptr, F, nv2, &status); });
      if (status) { printf("it %d: validate(seams) status %u\n", it, status); fails++; break; }
      const uint64_t nt = n_chunks * (F.max_len - 1);
      const uint32_t grid = (uint32_t)std::min<uint64_t>((nt + FSET_NT - 1) / FSET_NT, 1 + R(3));
      if (ic) launch_block<FSET_NT>(grid, [&] { findset_seams_kernel<true>(raw.data(), raw_off.data(), cuts.data(), slot.data(), n_chunks, F, scap ? sh.data() : nullptr, scap, &snh, sc.data(), &status, nt); });
      else launch_block<FSET_NT>(grid, [&] { findset_seams_kernel<false>(raw.data(), raw_off.data(), cuts.data(), slot.data(), n_chunks, F, scap ? sh.data() : nullptr, scap, &snh, sc.data(), &status, nt); });
      std::vector<std::pair<uint64_t, uint32_t>> gs;
      for (uint64_t i = 0; i < std::min<uint64_t>(snh, scap); i++) gs.push_back({sh[i] >> HMSE_FINDSET_ID_BITS, (uint32_t)(sh[i] & IDM)});
      std::sort(gs.begin(), gs.end());
      bool sok = snh == wseam.size() && ((status & 1) != 0) == (scap && wseam.size() > scap) && !(status & 2);
      if (scap >= wseam.size()) sok = sok && (scap == 0 || gs == wseam);
      else for (auto& g : gs) sok = sok && std::binary_search(wseam.begin(), wseam.end(), g);
      for (uint64_t i = scap; i < scap + 8; i++) sok = sok && sh[i] == ~0ull;
      std::vector<ull> wsc(np, 0);
      for (auto& w : wseam) wsc[w.second]++;
      sok = sok && sc == wsc;
      if (!sok) { printf("it %d: SEAMS mismatch n=%llu chunks=%llu np=%u ic=%d got=%llu want=%zu status=%u\n", it, (ull)n, (ull)n_chunks, np, ic, snh, wseam.size(), status); fails++; break; }
      // place (needs the full sorted scan list)
      std::vector<ull> hs;
      for (auto& w : want) hs.push_back((w.first << HMSE_FINDSET_ID_BITS) | w.second);
      std::vector<uint64_t> per(n_rec, 0), chunk_out{0};
      for (auto& w : want) { uint64_t r = std::upper_bound(raw_off.begin(), raw_off.end(), w.first) - raw_off.begin() - 1; while (raw_off[r + 1] <= w.first) r++; per[r]++; }
      for (uint64_t k = 0; k < n_chunks; k++) chunk_out.push_back(chunk_out.back() + per[slot[k]]);
      const uint64_t total = chunk_out.back();
      std::vector<ull> out(total + 8, ~0ull);
      status = 0;
      FsetDev none; memset(&none, 0, sizeof none);
      launch_block<FSET_NT>(1, [&] { findset_validate_kernel(raw_off.data(), n_rec, ~0ull, cuts.data(), slot.data(), n_chunks, chunk_out.data(), none, std::max(n_rec, n_chunks), &status); });
      launch_block<FSET_NT>((uint32_t)std::max<uint64_t>(1, (total + FSET_NT - 1) / FSET_NT), [&] { place_kernel<HMSE_FINDSET_ID_BITS, FSET_NT>(hs.data(), hs.size(), raw_off.data(), cuts.data(), slot.data(), n_chunks, chunk_out.data(), out.data(), total, &status); });
      bool pok = status == 0 && total == win.size();
      for (uint64_t i = 0; pok && i < total; i++) pok = (out[i] >> HMSE_FINDSET_ID_BITS) == win[i].first && (out[i] & IDM) == win[i].second;
      for (uint64_t i = total; i < total + 8; i++) pok = pok && out[i] == ~0ull;
      if (!pok) { printf("it %d: PLACE mismatch total=%llu want=%zu status=%u\n", it, (ull)total, win.size(), status); fails++; break; }
    }
    ran++;
    printf("it %d ok: n=%llu rec=%llu chunks=%llu np=%u ic=%d scan=%zu seam=%zu\n", it, (ull)n, (ull)n_rec, (ull)n_chunks, np, ic, want.size(), wseam.size());
  }
  printf("%d cases ran\n", ran);
  printf(fails ? "FAILED\n" : "ALL OK\n");
  return fails;
}
