// inflate_emu.cpp — the two decoders of hmse_amd/csrc/l1_inflate.hip run on the CPU, one std::thread per lane (tools/hip_on_cpu.h):
// ifl::l1_inflate_kernel (one stream per wavefront, over inflate_core.h as it is: __ballot, readlane and readfirstlane meet at a barrier
// per wavefront, so a loop or a value that is not wave-uniform hangs or gives a wrong answer) as one workgroup of four wavefronts, and
// ifl::l1_inflate_lanes_kernel (one stream per lane) as one workgroup of one wavefront.  Both pull every record of the file that
// tools/inflate_emu.py writes — hand-built DEFLATE streams zlib's encoder never emits (tests/deflate_vectors.py), with zlib's decision and
// bytes for each; a record with a dictionary is a DELTA record whose base another lane or wavefront of the same group decodes.  Every
// buffer is a heap block of exactly the declared size (a sanitizer sees a read or write one byte outside); the output starts poisoned.
// No GPU: this checks the kernels' LOGIC and bounds, not their code object.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "hmse.h"
#include "hip_on_cpu.h"
#include "inflate_core.h"
namespace ifl {
#include "l1_inflate_kernels.inc"
}  // namespace ifl (the cut ends inside the namespace it opened last)

template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a heap block of exactly v.size() elements
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

struct Records {
  std::vector<uint8_t> streams, kind, want_ok, want_raw;
  std::vector<uint64_t> stream_off{0}, raw_off{0};
  std::vector<int64_t> base;
};

// the file of tools/inflate_emu.py: u32 n, then per record u32 stream bytes, the stream, u32 raw bytes, i32 base record or -1, u8 accepted,
// the raw bytes (zeros where zlib refuses: nothing is compared there)
static bool load(const char* path, Records& r) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint32_t n = 0;
  bool ok = fread(&n, 4, 1, f) == 1;
  for (uint32_t k = 0; ok && k < n; k++) {
    uint32_t sl, rl; int32_t b; uint8_t acc;
    ok = fread(&sl, 4, 1, f) == 1;
    if (!ok) break;
    const size_t s0 = r.streams.size();
    r.streams.resize(s0 + sl);
    ok = (sl == 0 || fread(r.streams.data() + s0, 1, sl, f) == sl) && fread(&rl, 4, 1, f) == 1 && fread(&b, 4, 1, f) == 1 && fread(&acc, 1, 1, f) == 1;
    if (!ok) break;
    const size_t r0 = r.want_raw.size();
    r.want_raw.resize(r0 + rl);
    ok = rl == 0 || fread(r.want_raw.data() + r0, 1, rl, f) == rl;
    r.stream_off.push_back(r.streams.size()); r.raw_off.push_back(r.want_raw.size());
    r.base.push_back(b); r.kind.push_back(b >= 0 ? HMSE_KIND_DELTA : HMSE_KIND_FULL); r.want_ok.push_back(acc);
  }
  fclose(f);
  return ok && n != 0;
}

static int run(const Records& r, bool lanes) {
  const uint32_t n = (uint32_t)r.kind.size();
  const char* name = lanes ? "l1_inflate_lanes_kernel" : "l1_inflate_kernel";
  auto S = exact(r.streams); auto SO = exact(r.stream_off); auto RO = exact(r.raw_off); auto K = exact(r.kind); auto B = exact(r.base);
  std::vector<uint8_t> poison(r.want_raw.size(), 0xA5), okp(n, 0xA5);
  auto OUT = exact(poison); auto OK = exact(okp);
  std::vector<uint32_t> zeros(n, 0);
  auto DONE = exact(zeros);
  uint32_t counter[64] = {0}, status = 0;
  ifl::Args a;
  a.streams = S.get(); a.streams_bytes = r.streams.size(); a.stream_off = SO.get(); a.stream_len = nullptr; a.kind = K.get(); a.base = B.get(); a.n_sel = n;
  a.raw_off = RO.get(); a.raw_out = OUT.get(); a.raw_cap = r.want_raw.size(); a.status = &status; a.ok = OK.get(); a.done = DONE.get(); a.counter = counter;
  a.dflags = 0; a.trace = nullptr;
  if (lanes) launch_waves<64>(1, [&] { ifl::l1_inflate_lanes_kernel(a); });
  else launch_waves<ifl::NT>(1, [&] { ifl::l1_inflate_kernel(a); });
  int wrong = 0; uint32_t refused = 0;
  for (uint32_t k = 0; k < n; k++) {
    bool same = OK[k] == r.want_ok[k] && DONE[k] == (r.want_ok[k] ? 1u : 2u);
    if (same && r.want_ok[k]) same = memcmp(OUT.get() + r.raw_off[k], r.want_raw.data() + r.raw_off[k], r.raw_off[k + 1] - r.raw_off[k]) == 0;
    refused += !r.want_ok[k];
    if (!same) { printf("%s: record %u: ok %u (zlib %u), done %u%s\n", name, k, OK[k], r.want_ok[k], DONE[k], OK[k] == r.want_ok[k] ? ", other bytes" : ""); wrong++; }
  }
  if (status != (refused ? 1u : 0u)) { printf("%s: status %u with %u refused records\n", name, status, refused); wrong++; }
  printf("%s: %u records, %d wrong (%u of them refused by zlib)\n", name, n, wrong, refused);
  return wrong;
}

int main(int argc, char** argv) {
  Records r;
  if (argc < 4 || !load(argv[3], r)) { printf("no records (run tools/inflate_emu.py)\n"); return 1; }
  if (r.streams.size() < 16 || r.want_raw.size() < 16) { printf("the lane kernel asks for 16 bytes of streams and of output at least\n"); return 1; }
  int fails = run(r, false);
  fails += run(r, true);
  printf(fails ? "FAILED\n" : "ALL OK: both kernels decide and decode as zlib does\n");
  return fails != 0;
}
