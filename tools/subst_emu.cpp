// subst_emu.cpp — the kernels of hmse_amd/csrc/subst.hip run on the CPU against the definition of include/hmse_subst.h (the naive splice),
// byte by byte.  subst_apply_kernel meets at one __syncthreads and its first wavefront at __ballot, so its launcher here gives a
// workgroup both barriers (one std::thread per lane; a loop that is not wave-uniform hangs it); subst_edits_kernel and the validate
// kernel of hmse_amd/csrc/chunkmap.h have no meeting point and run lane after lane on one thread.  The kernels are templates over the
// workgroup's shape: the product's <256, 4> runs the random lists, <64, 1> and <64, 2> (tiles of 1 and 2 KiB: several tiles at small
// sizes, and far fewer threads to start) run them as well and the sweep.
//   * random chunk maps: chunks of 0, 1 and 2 bytes, of up to a few strips, a single chunk, empty chunks at the end, exact dedupe of the
//     chunks, junk in front of and behind the records in raw; every table, raw, rep and the edits in heap blocks of exactly the declared
//     size (a sanitizer sees a read one byte outside); out poisoned, at every alignment, its block ending with out_cap;
//   * the sweep: every single edit (s, e) of a corpus of five strips + 7 bytes with replacement lengths 0, 1, 15, 16, 17 and two
//     strips + 1, and in fill mode (with iters < 100 every 41st pair only);
//   * outputs of a tile - 16 .. a tile + 18 bytes at every alignment of out, launched by the entry point's own grid arithmetic
//     (subst_grids, inside the cut): the last tile may exist only because of out's address;
//   * random edit lists with ties, insertions, deletions, touching edits, in both modes;
//   * refused input of every kind: status as the header says and not one byte of out written.
// No GPU: this checks the kernels' LOGIC and bounds (build it with a sanitizer), not their code object.  Driven by tools/subst_emu.py,
// which cuts the kernels out of subst.hip (everything between the geometry constants and the entry points) into subst_kernels.inc.
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
#include "hmse_subst.h"
#include "hip_on_cpu.h"
#include "chunkmap.h"
#include "subst_kernels.inc"

static std::mt19937_64 rng(12345);
static uint64_t R(uint64_t n) { return n ? rng() % n : 0; }
template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a heap block of exactly v.size() elements
  std::unique_ptr<T[]> p(v.empty() ? nullptr : new T[v.size()]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

// a workgroup with both meeting points: __syncthreads for all, __ballot per wavefront
template <int NT> static void launch_tile(uint32_t grid, const std::function<void()>& f) {
  gridDim.x = grid;
  for (uint32_t b = 0; b < grid; b++) {
    std::barrier<> bar(NT);
    g_bar = &bar;
    std::unique_ptr<std::barrier<>> wave[NT / 64];
    for (int w = 0; w < NT / 64; w++) { wave[w].reset(new std::barrier<>(64)); g_wave[w] = wave[w].get(); }
    memset(g_bits, 0, sizeof g_bits);
    std::vector<std::thread> th;
    for (int t = 0; t < NT; t++) th.emplace_back([&, t, b] { threadIdx.x = t; blockIdx.x = b; f(); bar.arrive_and_drop(); });
    for (auto& x : th) x.join();
  }
}
// lane after lane on this thread: for kernels whose lanes never meet
template <int NT> static void launch_serial(uint32_t grid, const std::function<void()>& f) {
  gridDim.x = grid;
  for (uint32_t b = 0; b < grid; b++)
    for (int t = 0; t < NT; t++) { threadIdx.x = t; blockIdx.x = b; f(); }
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
  if (junk) for (uint64_t g = R(20); g > 0; g--) m.raw.push_back((uint8_t)R(256));
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
  if (junk) for (uint64_t g = R(20); g > 0; g--) m.raw.push_back((uint8_t)R(256));
  return m;
}
static std::vector<uint64_t> random_cuts(uint64_t N, int mode) {      // 0: chunks of 0 / 1 / 2 bytes, 1: 1..150, 2: one chunk, 3: a mix with empty ones
  std::vector<uint64_t> cuts{0};
  while (cuts.back() < N) {
    uint64_t l = mode == 0 ? R(3) : mode == 1 ? 1 + R(150) : mode == 2 ? N : (R(3) == 0 ? 0 : 1 + R(40));
    if (cuts.back() + l > N) l = N - cuts.back();
    cuts.push_back(cuts.back() + l);
  }
  for (uint64_t k = R(3); k > 0; k--) cuts.push_back(N);               // empty chunks at the end; with N == 0 maybe no chunk at all
  return cuts;
}

struct Edits {
  std::vector<uint64_t> start, end, sel, rep_off{0}, out_off;
  std::vector<uint8_t> rep;
  uint64_t rep_bytes = 0;                                  // the declared size: rep may be followed by bytes no replacement names
  bool fill = false;
};
// the definition: the naive splice, and out_off as it goes
static std::vector<uint8_t> splice(const std::vector<uint8_t>& C, Edits& e) {
  std::vector<uint8_t> O;
  uint64_t at = 0;
  e.out_off.clear();
  for (size_t i = 0; i < e.start.size(); i++) {
    O.insert(O.end(), C.begin() + at, C.begin() + e.start[i]);
    e.out_off.push_back(O.size());
    const uint64_t r0 = e.rep_off[e.sel[i]], r1 = e.rep_off[e.sel[i] + 1];
    if (e.fill) O.insert(O.end(), e.end[i] - e.start[i], e.rep[r0]);
    else O.insert(O.end(), e.rep.begin() + r0, e.rep.begin() + r1);
    at = e.end[i];
  }
  O.insert(O.end(), C.begin() + at, C.end());
  e.out_off.push_back(O.size());
  return O;
}

static uint64_t g_calls = 0, g_bytes = 0, g_refused = 0;
static const uint8_t POISON = 0xA5;

// one call of the three kernels as hmse_subst_apply launches them, in the shape <NT, TRIPS>; -> the status; out is checked here
template <int NT, int TRIPS>
static bool run(const char* what, const Map& m, const Edits& e, const std::vector<uint8_t>* want, uint32_t want_status, uint64_t out_cap, uint32_t lead) {
  auto RAW = exact(m.raw); auto RO = exact(m.raw_off); auto CU = exact(m.cuts); auto SL = exact(m.slot);
  auto S = exact(e.start); auto E = exact(e.end); auto SEL = exact(e.sel); auto REP = exact(e.rep); auto RPO = exact(e.rep_off); auto OO = exact(e.out_off);
  const uint64_t n = e.start.size(), n_rep = e.rep_off.size() - 1;
  // out lies `lead` bytes into a 16-byte-aligned block that ends with out_cap: one byte more is the sanitizer's finding
  const size_t block_bytes = lead + out_cap ? lead + out_cap : 1;
  auto drop = [](uint8_t* p) { ::operator delete(p, std::align_val_t(16)); };
  std::unique_ptr<uint8_t, decltype(drop)> block((uint8_t*)::operator new(block_bytes, std::align_val_t(16)), drop);
  memset(block.get(), POISON, block_bytes);
  uint8_t* out = block.get() + lead;
  uint32_t status = 0;
  const SubstGrids g = subst_grids(m.n_rec, m.n_chunks, n, n_rep, out, out_cap, NT, (uint64_t)NT * SUBST_STRIP * TRIPS);   // the entry point's own arithmetic
  if (g.tables)
    launch_serial<NT>((uint32_t)g.tables, [&] { tables_validate_kernel<NT>(RO.get(), m.n_rec, m.raw.size(), CU.get(), SL.get(), m.n_chunks, CU.get(), &status); });
  launch_serial<NT>((uint32_t)g.edits, [&] {
    subst_edits_kernel<NT>(CU.get(), m.n_chunks, S.get(), E.get(), SEL.get(), n, e.rep_bytes, RPO.get(), n_rep, e.fill, OO.get(), out_cap, &status);
  });
  if (out_cap) {
    const uint32_t blocks = (uint32_t)g.tiles;
    if (e.fill) launch_tile<NT>(blocks, [&] { subst_apply_kernel<NT, TRIPS, true>(RAW.get(), RO.get(), CU.get(), SL.get(), m.n_chunks, S.get(), E.get(), SEL.get(), n, REP.get(), RPO.get(), OO.get(), out, &status); });
    else launch_tile<NT>(blocks, [&] { subst_apply_kernel<NT, TRIPS, false>(RAW.get(), RO.get(), CU.get(), SL.get(), m.n_chunks, S.get(), E.get(), SEL.get(), n, REP.get(), RPO.get(), OO.get(), out, &status); });
  }
  g_calls++;
  if (status != want_status) { printf("%s <%d, %d>: status %u, want %u\n", what, NT, TRIPS, status, want_status); return false; }
  const uint64_t written = status ? 0 : want->size();
  for (uint32_t j = 0; j < lead; j++) if (out[(int64_t)j - lead] != POISON) { printf("%s <%d, %d>: a byte in front of out was written\n", what, NT, TRIPS); return false; }
  for (uint64_t p = 0; p < written; p++)
    if (out[p] != (*want)[p]) {
      printf("%s <%d, %d>: output byte %llu of %llu is %02x, want %02x (lead %u, n %llu, fill %d)\n", what, NT, TRIPS, (unsigned long long)p,
             (unsigned long long)written, out[p], (*want)[p], lead, (unsigned long long)n, (int)e.fill);
      return false;
    }
  for (uint64_t p = written; p < out_cap; p++)
    if (out[p] != POISON) { printf("%s <%d, %d>: byte %llu behind the output (%llu bytes) was written, status %u\n", what, NT, TRIPS, (unsigned long long)p, (unsigned long long)written, status); return false; }
  g_bytes += written;
  g_refused += status != 0;
  return true;
}
static bool run_shapes(const char* what, const Map& m, const Edits& e, const std::vector<uint8_t>* want, uint32_t want_status, uint64_t out_cap, int shapes) {
  const uint32_t lead = (uint32_t)R(16);
  bool ok = true;
  if (shapes & 1) ok = ok && run<64, 1>(what, m, e, want, want_status, out_cap, lead);
  if (shapes & 2) ok = ok && run<64, 2>(what, m, e, want, want_status, out_cap, (uint32_t)R(16));
  if (shapes & 4) ok = ok && run<SUBST_NT, SUBST_TRIPS>(what, m, e, want, want_status, out_cap, (uint32_t)R(16));
  return ok;
}

// a random legal edit list over N bytes: ties, insertions, deletions, touching edits, runs of one-byte deletions
static Edits random_edits(uint64_t N, bool fill) {
  Edits e;
  e.fill = fill;
  const uint64_t n_rep = 1 + R(4);
  for (uint64_t r = 0; r < n_rep; r++) {
    const uint64_t len = fill ? 1 : (R(3) == 0 ? 0 : R(2) ? 1 + R(4) : 1 + R(40));
    for (uint64_t j = 0; j < len; j++) e.rep.push_back((uint8_t)('A' + R(26)));
    e.rep_off.push_back(e.rep.size());
  }
  e.rep_bytes = e.rep.size() + (R(2) ? R(5) : 0);
  for (uint64_t j = e.rep.size(); j < e.rep_bytes; j++) e.rep.push_back('#');
  const int kind = (int)R(4);                            // 0: sparse, 1: dense, 2: none or one, 3: a run of one-byte deletions among others
  uint64_t at = 0;
  const uint64_t n_max = kind == 2 ? R(2) : kind == 0 ? R(6) : R(60);
  for (uint64_t i = 0; i < n_max; i++) {
    const uint64_t gap = kind == 0 ? R(N + 1) : R(4) == 0 ? 0 : R(9);
    uint64_t s = at + gap;
    if (s > N) break;
    uint64_t len = R(3) == 0 ? 0 : kind == 3 ? 1 : 1 + R(kind == 0 ? 50 : 6);
    if (s + len > N) len = N - s;
    e.start.push_back(s); e.end.push_back(s + len); e.sel.push_back(R(n_rep));
    at = s + len;
    if (kind == 3 && R(3)) for (uint64_t k = R(40); k > 0 && at < N; k--) { e.start.push_back(at); e.end.push_back(at + 1); e.sel.push_back(R(n_rep)); at++; }
  }
  return e;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 30;
  if (argc > 2) rng.seed(strtoull(argv[2], nullptr, 10));
  int fails = 0;
  // ---- the sweep: every single edit of a corpus of five strips + 7 bytes ----
  {
    const uint64_t N = 5 * SUBST_STRIP + 7;
    std::vector<uint8_t> C(N);
    for (uint64_t q = 0; q < N; q++) C[q] = (uint8_t)('a' + q % 26);
    const Map maps[2] = {lay_out(C, random_cuts(N, 2), false), lay_out(C, random_cuts(N, 0), true)};
    static const uint64_t LEN[] = {0, 1, 15, 16, 17, 2 * SUBST_STRIP + 1};
    const uint64_t stride = iters >= 100 ? 1 : 41;
    uint64_t pair = 0, swept = 0;
    for (uint64_t s = 0; s <= N && !fails; s++)
      for (uint64_t en = s; en <= N && !fails; en++, pair++) {
        if (pair % stride) continue;
        for (int v = 0; v < 7 && !fails; v++) {          // six literal lengths, then fill
          Edits e;
          e.fill = v == 6;
          const uint64_t len = e.fill ? 1 : LEN[v];
          for (uint64_t j = 0; j < len; j++) e.rep.push_back((uint8_t)('A' + j % 26));
          e.rep_off.push_back(len);
          e.rep_bytes = len;
          e.start = {s}; e.end = {en}; e.sel = {0};
          const std::vector<uint8_t> want = splice(C, e);
          char what[96];
          snprintf(what, sizeof what, "sweep [%llu, %llu) variant %d", (unsigned long long)s, (unsigned long long)en, v);
          if (!run<64, 1>(what, maps[pair & 1], e, &want, 0, want.size(), (uint32_t)((s + 3 * en + v) % 16))) fails++;
          swept++;
        }
      }
    if (!fails) printf("sweep ok: %llu single edits over %llu bytes (every %llu. pair)\n", (unsigned long long)swept, (unsigned long long)N, (unsigned long long)stride);
  }
  // ---- output lengths around a tile's end at every alignment of out: the last tile exists only because of out's address ----
  for (int shape = 0; shape < 2 && !fails; shape++) {
    const uint64_t TILE = shape ? 2048 : 1024;           // <64, 2> and <64, 1>
    uint64_t swept = 0;
    for (uint64_t N = TILE - 16; N <= TILE + 16 && !fails; N++) {
      std::vector<uint8_t> C(N);
      for (uint64_t q = 0; q < N; q++) C[q] = (uint8_t)('a' + (q * 7) % 26);
      const Map m = lay_out(C, random_cuts(N, (int)(N % 4)), false);
      for (uint32_t lead = 0; lead < 16 && !fails; lead++)
        for (int v = 0; v < 3 && !fails; v++) {          // no edit; a byte near the end becomes three (the output ends two on); fill
          Edits e;
          e.fill = v == 2;
          e.rep = {(uint8_t)'X', (uint8_t)'Y', (uint8_t)'Z'};
          e.rep_off = {0, e.fill ? 1ull : 3ull};
          e.rep_bytes = 3;
          if (v) { e.start = {N - 5}; e.end = {N - 4}; e.sel = {0}; }
          const std::vector<uint8_t> want = splice(C, e);
          char what[96];
          snprintf(what, sizeof what, "tile end: N %llu, lead %u, variant %d", (unsigned long long)N, lead, v);
          const bool ok = shape ? run<64, 2>(what, m, e, &want, 0, want.size(), lead) : run<64, 1>(what, m, e, &want, 0, want.size(), lead);
          if (!ok) fails++;
          swept++;
        }
    }
    if (!fails) printf("tile ends ok: %llu calls with outputs of %llu - 16 .. %llu + 18 bytes at every alignment of out\n", (unsigned long long)swept,
                       (unsigned long long)TILE, (unsigned long long)TILE);
  }
  // ---- random chunk maps and edit lists, and refused input ----
  for (int it = 0; it < iters && !fails; it++) {
    const uint64_t N = R(8) == 0 ? R(3) : 1 + R(it % 3 == 0 ? 260 * SUBST_STRIP : 9 * SUBST_STRIP);      // every third: several tiles of the small shapes
    std::vector<uint8_t> C(N);
    for (auto& x : C) x = (uint8_t)('a' + R(26));
    const int mode = (int)R(4);
    Map m = lay_out(C, random_cuts(N, mode), true);
    const bool fill = R(2);
    Edits e = random_edits(N, fill);
    const std::vector<uint8_t> want = splice(C, e);
    char what[96];
    snprintf(what, sizeof what, "it %d (N %llu, chunks mode %d, n %zu, fill %d)", it, (unsigned long long)N, mode, e.start.size(), (int)fill);
    const int shapes = it % 10 == 0 ? 7 : 1 + (int)R(3);             // the product's shape every tenth time, the small ones always
    if (!run_shapes(what, m, e, &want, 0, want.size() + (R(2) ? R(40) : 0), shapes)) { fails++; break; }
    // refused: one thing wrong at a time
    const uint64_t n = e.start.size(), n_rep = e.rep_off.size() - 1;
    for (int kind = 0; kind < 14 && !fails; kind++) {
      Edits b = e;
      Map mb = m;
      uint32_t want_status = 2;
      uint64_t cap = want.size();
      bool made = false;
      switch (kind) {
        case 0: if (n >= 2) { const uint64_t i = 1 + R(n - 1); if (b.end[i - 1] > 0) { b.start[i] = b.end[i - 1] - 1; made = true; } } break;        // overlap
        case 1: if (n) { b.end[n - 1] = N + 1 + R(9); made = true; } break;                                                                // leaves the corpus
        case 2: if (n) { b.sel[R(n)] = n_rep + R(3) * (1ull << 40); made = true; } break;                                                  // no such replacement
        case 3: if (n_rep >= 2 && !fill) { const uint64_t r = 1 + R(n_rep - 1); b.rep_off[r] = b.rep_off[r + 1] + 1; made = true; } break;  // rep_off descends
        case 4: { b.rep_off[n_rep] = b.rep_bytes + 1; made = !fill || true; } break;                                                       // ends past rep_bytes
        case 5: { b.rep_off[0] = 1; made = true; } break;                                                                                 // does not start at 0
        case 6: if (fill) { b.rep_off[n_rep] += 1; b.rep.push_back('!'); b.rep_bytes = b.rep.size(); made = true; } break;                    // fill with two bytes
        case 7: if (n) { b.out_off[0] += 1; made = true; } break;
        case 8: if (n >= 3) { b.out_off[1 + R(n - 1)] += 1 + R(3); made = true; } break;
        case 9: { b.out_off[n] += 1; cap += 1; made = true; } break;
        case 10: if (mb.n_chunks >= 2 && N >= 4) { const uint64_t k = 1 + R(mb.n_chunks - 1); mb.cuts[k] = mb.cuts[k + 1] + 1 + R(5); made = true; } break;
        case 11: if (mb.n_chunks) { mb.slot[R(mb.n_chunks)] = mb.n_rec + R(3); made = true; } break;
        case 12: if (mb.n_chunks && N) { mb.cuts[0] = 1; made = true; } break;
        case 13: if (want.size()) { cap = want.size() - 1; want_status = 1; made = true; } break;                                            // one byte short
      }
      if (!made) continue;
      snprintf(what, sizeof what, "it %d refused kind %d (N %llu, n %zu, fill %d)", it, kind, (unsigned long long)N, e.start.size(), (int)fill);
      if (!run_shapes(what, mb, b, &want, want_status, cap, 1 << R(2))) fails++;
    }
    if (!fails && (it % 20 == 19 || it + 1 == iters))
      printf("it %d ok: %llu calls, %llu bytes equal the splice, %llu calls refused\n", it, (unsigned long long)g_calls, (unsigned long long)g_bytes, (unsigned long long)g_refused);
  }
  printf(fails ? "FAILED\n" : "ALL OK: %llu calls, %llu bytes equal the splice, %llu calls refused with out untouched\n", (unsigned long long)g_calls,
         (unsigned long long)g_bytes, (unsigned long long)g_refused);
  return fails;
}
