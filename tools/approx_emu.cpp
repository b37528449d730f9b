// approx_emu.cpp — the kernels of hmse_amd/csrc/approx.hip run on the CPU, one std::thread per lane and a barrier for __syncthreads,
// against Sellers' dynamic programme (plain columns, no bit tricks): random corpora with planted noisy copies of the patterns, tiny and
// empty chunks, deduplicated into records with junk around them in raw, full / short / no hit lists; then place_kernel<8>
// (hmse_amd/csrc/chunkmap.h) over the sorted scan hits, the seams over the same chunk map, the spans of every hit (and of hits that
// cannot be), and tables the validate kernel must refuse.  No GPU: this checks the kernels' LOGIC and their bounds (build it with a
// sanitizer), not their code objects.  Driven by tools/approx_emu.py, which cuts the kernels out.
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
#include "approx_kernels.inc"
typedef unsigned long long ull;
static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }
static const uint8_t ALPHA[] = {'a', 'b', 'A', 'B', '\n', 0xC1, 0xE1, '@', '[', '`', '{', 'z', 'Z'};
static uint8_t fold(uint8_t b, bool ic) { return ic && b >= 'A' && b <= 'Z' ? b | 0x20 : b; }

struct Pat { std::vector<uint8_t> p; uint32_t k; };
// d(e) for e = 1 .. n over text[0, n): the column D[0] = 0, D[i] = i in front of the first byte
static std::vector<uint32_t> distances(const Pat& P, const uint8_t* text, uint64_t n, bool ic) {
  const size_t m = P.p.size();
  std::vector<uint32_t> col(m + 1), nw(m + 1), out(n);
  for (size_t i = 0; i <= m; i++) col[i] = i;
  for (uint64_t e = 0; e < n; e++) {
    nw[0] = 0;
    for (size_t i = 1; i <= m; i++)
      nw[i] = std::min({col[i - 1] + (fold(P.p[i - 1], ic) != fold(text[e], ic)), col[i] + 1, nw[i - 1] + 1});
    col.swap(nw);
    out[e] = col[m];
  }
  return out;
}
// the span's start: the anchored column (D[0][t] = t) of the reversed pattern over C[o], C[o - 1], ..., at most m + d bytes; o + 1 if none
static uint64_t span(const Pat& P, const uint8_t* C, uint64_t o, uint32_t d, bool ic) {
  const size_t m = P.p.size();
  std::vector<uint32_t> col(m + 1), nw(m + 1);
  for (size_t i = 0; i <= m; i++) col[i] = i;
  for (uint64_t s = 0; s < m + d && s <= o; s++) {
    nw[0] = s + 1;
    for (size_t i = 1; i <= m; i++)
      nw[i] = std::min({col[i - 1] + (fold(P.p[m - i], ic) != fold(C[o - s], ic)), col[i] + 1, nw[i - 1] + 1});
    col.swap(nw);
    if (col[m] == d) return o - s;
  }
  return o + 1;
}

int main(int argc, char** argv) {
  int iters = argc > 1 ? atoi(argv[1]) : 20;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  int fails = 0, ran = 0;
  for (int it = 0; it < iters && !fails; it++) {
    const bool ic = R(2);
    const int nalpha = 2 + R(sizeof ALPHA - 1);
    // ---- the patterns: 1 .. 8 of them, the lengths at which the column changes shape, k up to min(m - 1, 16) ----
    static const uint32_t LEN[] = {1, 2, 3, 5, 8, 16, 31, 63, 64};
    const uint32_t n_pat = it == 0 ? 8 : 1 + R(8);
    std::vector<Pat> pats(n_pat);
    std::vector<uint8_t> pat;
    std::vector<uint32_t> pat_off{0};
    uint32_t wmax = 1;
    for (uint32_t j = 0; j < n_pat; j++) {
      const uint32_t m = LEN[it == 0 ? j + 1 : R(9)];
      for (uint32_t i = 0; i < m; i++) pats[j].p.push_back(R(8) == 0 && m == 64 ? 'a' : ALPHA[R(nalpha)]);
      if (R(6) == 0) std::fill(pats[j].p.begin(), pats[j].p.end(), 'a');       // a run: the carry walks through the whole column
      const uint32_t kmax = std::min<uint32_t>(m - 1, HMSE_APPROX_MAX_K);
      pats[j].k = R(3) == 0 ? kmax : R(std::min<uint32_t>(kmax, 3) + 1);
      if (j && R(8) == 0) pats[j] = pats[j - 1];                              // equal patterns are answered each on its own
      pat.insert(pat.end(), pats[j].p.begin(), pats[j].p.end());
      pat_off.push_back(pat.size());
      wmax = std::max<uint32_t>(wmax, pats[j].p.size() + pats[j].k);
    }
    AxPats P{};
    P.n = n_pat; P.wmax = wmax; P.ic = ic;
    for (uint32_t j = 0; j <= AX_P; j++) P.off[j] = pat_off[std::min(j, n_pat)];
    for (uint32_t j = 0; j < AX_P; j++) { P.m[j] = j < n_pat ? pats[j].p.size() : 1; P.k[j] = j < n_pat ? pats[j].k : 0; }
    // ---- the corpus, with noisy copies planted ----
    uint64_t n = R(4) == 0 ? R(400) : (R(3) == 0 ? AX_TILE + R(AX_TILE) : 4 * n_pat * 80 + R(6000));   // (mostly: room for a slot per copy)
    std::vector<uint8_t> corpus(n);
    for (auto& c : corpus) c = ALPHA[R(nalpha)];
    if (n > 700 && R(2)) { uint64_t o = R(n - 700); for (uint64_t i = 0; i < 300 + R(400); i++) corpus[o + i] = 'a'; }
    if (n > AX_TILE + 700 && R(2)) for (uint64_t i = AX_TILE - 300; i < AX_TILE + 300; i++) corpus[i] = 'a';   // a run over a tile edge
    // every copy in a slot of its own (no copy damages another), the first of every pattern unedited: where the slots hold the patterns,
    // every pattern has an occurrence
    const uint64_t slot_size = n / (4 * n_pat);
    bool fits = true;
    for (uint32_t j = 0; j < n_pat; j++) fits = fits && pats[j].p.size() <= slot_size;
    for (uint32_t j = 0; fits && j < n_pat; j++)
      for (int c = 0; c < 4; c++) {
        std::vector<uint8_t> s = pats[j].p;
        for (uint32_t e = c ? R(pats[j].k + 2) : 0; e > 0; e--) {
          const int op = R(3);
          if (op == 0 && !s.empty()) s[R(s.size())] = ALPHA[R(nalpha)];
          else if (op == 1) s.insert(s.begin() + R(s.size() + 1), ALPHA[R(nalpha)]);
          else if (!s.empty()) s.erase(s.begin() + R(s.size()));
        }
        if (s.size() > slot_size) s.resize(slot_size);
        std::copy(s.begin(), s.end(), corpus.begin() + (4 * j + c) * slot_size + R(slot_size - s.size() + 1));
      }
    std::vector<uint64_t> cuts{0};
    while (cuts.back() < n) {
      static const uint64_t L[] = {0, 1, 2, 3, 1, 7, 30, 79, 80, 81, 200, 3000, 40000};
      cuts.push_back(std::min(n, cuts.back() + L[R(n > 10000 ? 13 : 11)]));
    }
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
    // junk in front of the records — every third case more than a tile of it — and up to three EMPTY records first (no chunk maps to them)
    // (case 1 always has both: a tile that lies wholly in front of the records, whose first ones are empty)
    const uint64_t lead = (it == 1 || R(3) == 0) ? AX_TILE + R(AX_TILE + 300) : (R(2) ? R(300) : 0), tail = R(2) ? R(300) : 0;
    const uint64_t n_lead_empty = it == 1 ? 2 : (R(2) ? R(4) : 0);
    std::vector<uint8_t> raw(lead, 'a');
    std::vector<uint64_t> raw_off{lead};
    for (auto& s : slot) s += n_lead_empty;
    recs.insert(recs.begin(), n_lead_empty, std::string());
    for (auto& r : recs) { raw.insert(raw.end(), r.begin(), r.end()); raw_off.push_back(raw.size()); }
    for (uint64_t i = 0; i < tail; i++) raw.push_back(ALPHA[R(nalpha)]);
    const uint64_t raw_bytes = raw.size(), n_rec = recs.size();
    std::vector<uint32_t> mult(n_rec, 0);
    for (auto s : slot) mult[s]++;
    // ---- scan: the scan ends of every record, each record on its own ----
    std::vector<ull> want;
    std::vector<ull> wc(n_pat, 0);
    for (uint64_t r = 0; r < n_rec; r++)
      for (uint32_t j = 0; j < n_pat; j++) {
        const auto d = distances(pats[j], raw.data() + raw_off[r], raw_off[r + 1] - raw_off[r], ic);
        for (uint64_t e = 0; e < d.size(); e++)
          if (d[e] <= pats[j].k && e + 1 >= pats[j].p.size() + pats[j].k) { want.push_back(((raw_off[r] + e) << 8) | (d[e] << 3) | j); wc[j] += mult[r]; }
      }
    std::sort(want.begin(), want.end());
    const uint64_t cap = R(3) == 0 ? 0 : (R(2) ? want.size() : R(want.size() + 1));
    std::vector<ull> hits(cap + 8, ~0ull), cnt(n_pat + 1, 0);
    ull nh = 0; uint32_t status = 0;
    launch_block<AX_NT>(2, [&] { tables_validate_kernel<AX_NT>(raw_off.data(), n_rec, raw_bytes, nullptr, nullptr, 0, nullptr, &status); });
    if (status) { printf("it %d: validate status %u\n", it, status); fails++; break; }
    const uint64_t n_tiles = (raw_bytes + AX_TILE - 1) / AX_TILE;
    auto scan = [&](ull* h, uint64_t c, ull* pn, ull* cn, uint32_t* st) {
      const uint32_t grid = (uint32_t)std::min<uint64_t>(n_tiles, 1 + R(2));
      const uint32_t* mu = mult.data();
      if (n_pat == 1) launch_block<AX_NT>(grid, [&] { approx_scan_kernel<1>(raw.data(), raw_bytes, raw_off.data(), n_rec, mu, pat.data(), P, c ? h : nullptr, c, pn, cn, st, n_tiles); });
      else if (n_pat == 2) launch_block<AX_NT>(grid, [&] { approx_scan_kernel<2>(raw.data(), raw_bytes, raw_off.data(), n_rec, mu, pat.data(), P, c ? h : nullptr, c, pn, cn, st, n_tiles); });
      else if (n_pat <= 4) launch_block<AX_NT>(grid, [&] { approx_scan_kernel<4>(raw.data(), raw_bytes, raw_off.data(), n_rec, mu, pat.data(), P, c ? h : nullptr, c, pn, cn, st, n_tiles); });
      else launch_block<AX_NT>(grid, [&] { approx_scan_kernel<8>(raw.data(), raw_bytes, raw_off.data(), n_rec, mu, pat.data(), P, c ? h : nullptr, c, pn, cn, st, n_tiles); });
    };
    if (n_rec && raw_bytes) scan(hits.data(), cap, &nh, cnt.data(), &status);
    bool ok = nh == want.size() && ((status & 1) != 0) == (cap && want.size() > cap) && !(status & 2) && cnt[n_pat] == 0;
    for (uint32_t j = 0; j < n_pat; j++) ok = ok && cnt[j] == wc[j];
    for (uint64_t i = cap; i < cap + 8; i++) ok = ok && hits[i] == ~0ull;
    std::vector<ull> got(hits.begin(), hits.begin() + std::min<uint64_t>(cap, nh));
    std::sort(got.begin(), got.end());
    if (cap >= want.size() && cap) ok = ok && got == want;
    else for (auto g : got) ok = ok && std::binary_search(want.begin(), want.end(), g);
    if (!ok) { printf("it %d: SCAN mismatch n=%llu n_pat=%u wmax=%u nh=%llu want=%zu status=%u cap=%llu\n", it, (ull)n, n_pat, wmax, nh, want.size(), status, (ull)cap); fails++; break; }
    // ---- inconsistent tables: refused by the validate kernel, the scan behind it writes nothing ----
    if (n_rec > 1 && raw_bytes) {
      std::vector<uint64_t> bad_off = raw_off;
      bad_off[n_rec] = raw_bytes + 1 + R(100);
      uint32_t st = 0; ull dn = 0;
      std::vector<ull> dh(8, ~0ull), dc(n_pat, 0);
      launch_block<AX_NT>(1, [&] { tables_validate_kernel<AX_NT>(bad_off.data(), n_rec, raw_bytes, nullptr, nullptr, 0, nullptr, &st); });
      launch_block<AX_NT>(1, [&] { approx_scan_kernel<8>(raw.data(), raw_bytes, bad_off.data(), n_rec, nullptr, pat.data(), P, dh.data(), 8, &dn, dc.data(), &st, n_tiles); });
      bool dok = st == 2 && dn == 0;
      for (auto v : dh) dok = dok && v == ~0ull;
      if (!dok) { printf("it %d: BAD tables not refused: status=%u nh=%llu\n", it, st, dn); fails++; break; }
    }
    // ---- the corpus: scan ends placed + seam ends = every occurrence once ----
    std::vector<ull> win, wseam;
    std::vector<ull> wsc(n_pat, 0);
    {
      std::vector<uint64_t> chunk_of(n);
      for (uint64_t k = 0; k < n_chunks; k++) for (uint64_t o = cuts[k]; o < cuts[k + 1]; o++) chunk_of[o] = k;
      for (uint32_t j = 0; j < n_pat; j++) {
        const auto d = distances(pats[j], corpus.data(), n, ic);
        for (uint64_t e = 0; e < n; e++)
          if (d[e] <= pats[j].k) {
            const bool sc = e + 1 - cuts[chunk_of[e]] >= pats[j].p.size() + pats[j].k;
            (sc ? win : wseam).push_back((e << 8) | (d[e] << 3) | j);
            if (!sc) wsc[j]++;
          }
      }
      std::sort(win.begin(), win.end());
      std::sort(wseam.begin(), wseam.end());
    }
    bool planted = true;
    for (uint32_t j = 0; j < n_pat; j++) {
      bool any = !fits;                                                       // (a corpus too small for the slots: nothing was planted)
      for (auto w : win) any = any || (w & 7) == j;
      for (auto w : wseam) any = any || (w & 7) == j;
      planted = planted && any;
    }
    if (!planted) { printf("it %d: a pattern has no occurrence (the planting failed)\n", it); fails++; break; }
    if (n_chunks) {
      const uint64_t scap = R(4) == 0 ? R(wseam.size() + 1) : wseam.size();
      std::vector<ull> sh(scap + 8, ~0ull), sc(n_pat + 1, 0);
      ull snh = 0; status = 0;
      launch_block<AX_NT>(2, [&] { tables_validate_kernel<AX_NT>(raw_off.data(), n_rec, raw_bytes, cuts.data(), slot.data(), n_chunks, nullptr, &status); });
      if (status) { printf("it %d: validate(seams) status %u\n", it, status); fails++; break; }
      if (wmax > 1) {
        const uint64_t nt = n_chunks * AX_P;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nt + AX_NT - 1) / AX_NT, 1 + R(3));
        launch_block<AX_NT>(grid, [&] { approx_seams_kernel(raw.data(), raw_off.data(), cuts.data(), slot.data(), n_chunks, pat.data(), P, scap ? sh.data() : nullptr, scap, &snh, sc.data(), &status, nt); });
      }
      std::vector<ull> gs(sh.begin(), sh.begin() + std::min<uint64_t>(snh, scap));
      std::sort(gs.begin(), gs.end());
      bool sok = snh == wseam.size() && ((status & 1) != 0) == (scap && wseam.size() > scap) && !(status & 2) && sc[n_pat] == 0;
      for (uint32_t j = 0; j < n_pat; j++) sok = sok && sc[j] == wsc[j];
      if (scap >= wseam.size()) sok = sok && (scap == 0 || gs == wseam);
      else for (auto g : gs) sok = sok && std::binary_search(wseam.begin(), wseam.end(), g);
      for (uint64_t i = scap; i < scap + 8; i++) sok = sok && sh[i] == ~0ull;
      if (!sok) { printf("it %d: SEAMS mismatch n=%llu chunks=%llu wmax=%u got=%llu want=%zu status=%u\n", it, (ull)n, (ull)n_chunks, wmax, snh, wseam.size(), status); fails++; break; }
      // place (needs the full sorted scan list): place_kernel<8> passes the low byte through
      std::vector<uint64_t> per(n_rec, 0), chunk_out{0};
      ull wtot = 0;
      for (auto w : want) { uint64_t r = std::upper_bound(raw_off.begin(), raw_off.end(), w >> 8) - raw_off.begin() - 1; per[r]++; }
      for (uint64_t k = 0; k < n_chunks; k++) chunk_out.push_back(chunk_out.back() + per[slot[k]]);
      for (auto c : wc) wtot += c;
      const uint64_t total = chunk_out.back();
      std::vector<ull> out(total + 8, ~0ull);
      status = 0;
      launch_block<AX_NT>((uint32_t)std::max<uint64_t>(1, (total + AX_NT - 1) / AX_NT), [&] { place_kernel<8, AX_NT>(want.data(), want.size(), raw_off.data(), cuts.data(), slot.data(), n_chunks, chunk_out.data(), out.data(), total, &status); });
      bool pok = status == 0 && total == win.size() && total == wtot;
      for (uint64_t i = 0; pok && i < total; i++) pok = out[i] == win[i];
      for (uint64_t i = total; i < total + 8; i++) pok = pok && out[i] == ~0ull;
      if (!pok) { printf("it %d: PLACE mismatch total=%llu want=%zu status=%u\n", it, (ull)total, win.size(), status); fails++; break; }
      // ---- spans: every hit (at most 4000 of them), then hits that cannot be ----
      std::vector<ull> all(win);
      all.insert(all.end(), wseam.begin(), wseam.end());
      std::shuffle(all.begin(), all.end(), rng);
      if (all.size() > 4000) all.resize(4000);
      const size_t n_good = all.size();
      all.push_back((n << 8) | 0);                                             // an offset that is not below N
      all.push_back(((n + 1000) << 8) | (1 << 3));
      if (n) all.push_back(((n - 1) << 8) | 7 | (n_pat < 8 ? 0 : (31 << 3)));  // no such pattern (or, with eight of them, errors of 31)
      std::vector<ull> st_got(all.size() + 8, ~0ull), st_want;
      bool any_bad = false;
      for (size_t i = 0; i < all.size(); i++) {
        const uint64_t o = all[i] >> 8; const uint32_t d = (all[i] >> 3) & 31, j = all[i] & 7;
        const uint64_t s = (o < n && j < n_pat) ? span(pats[j], corpus.data(), o, d, ic) : o + 1;
        st_want.push_back(s);
        any_bad = any_bad || s == o + 1;
        if (i < n_good && (s > o || o + 1 - s + d < pats[j].p.size() || o + 1 - s > pats[j].p.size() + d)) { printf("it %d: a span of impossible length\n", it); fails++; }
      }
      status = 0;
      launch_block<AX_NT>(1 + R(2), [&] { approx_spans_kernel(raw.data(), raw_off.data(), cuts.data(), slot.data(), n_chunks, pat.data(), P, all.data(), all.size(), st_got.data(), &status); });
      bool spok = status == (any_bad ? 1u : 0u);
      for (size_t i = 0; i < all.size(); i++) spok = spok && st_got[i] == st_want[i];
      for (size_t i = all.size(); i < all.size() + 8; i++) spok = spok && st_got[i] == ~0ull;
      if (!spok) { printf("it %d: SPANS mismatch hits=%zu status=%u\n", it, all.size(), status); fails++; break; }
    }
    ran++;
    printf("it %d ok: n=%llu lead=%llu empty_first=%llu rec=%llu chunks=%llu n_pat=%u wmax=%u ic=%d planted=%d scan=%zu seam=%zu\n", it, (ull)n, (ull)lead, (ull)n_lead_empty, (ull)n_rec, (ull)n_chunks, n_pat, wmax, (int)ic, (int)fits, want.size(), wseam.size());
  }
  printf("%d cases ran\n", ran);
  printf(fails ? "FAILED\n" : "ALL OK\n");
  return fails;
}
