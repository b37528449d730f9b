// bandtable.hip — the L4 band-table sidecar (hmse_amd/bandtable.py write_band_tables) written on the GPU.
//
// Layout (little-endian, byte for byte that of the numpy writer):
//   "HMSEBAND" | u32 1 | u32 bands | u32 band_bits | u32 3 | u64 n
//   per band: u64 n_headers | {band_hash u16, count u16}[n_headers] | ids u8[3 n]
//   optional: "HMSESIGS" | u32 n_hashes | band keys u32[n][bands] | signatures u32[n][n_hashes]
// Per band: a stable LSD radix sort of the ids by bucket (= key & (2^band_bits - 1)), 8 bits a pass.  A pass ranks inside 256-id
// tiles with wave ballots and mbcnt (the digit's peers among the lanes below), writes the tile's 256-bin histogram digit-major,
// scans it across tiles and scatters stably — so the ids stay ascending inside a bucket and no atomic operation decides an
// output position.  Then: bucket starts are flagged and scanned (run index), a piece of up to 65535 ids starts every 65535
// ids of a run (a continuation header), the pieces are scanned (header index), and one thread per id writes its 3 bytes and,
// at a piece start, its header.  A band's size depends on its header count, which only the device knows: the running output
// offset lives in device memory and a one-thread kernel advances it after each band.  The only host sync is the caller's
// read of out_bytes.
#include "common.h"
#include "blockops.h"

constexpr int BT_NT = 256;
constexpr int BT_SCAN_NT = 1024;
constexpr uint32_t BT_PIECE = 65535u;
constexpr uint64_t BT_HEAD = 32;          // "HMSEBAND" + u32 x4 + u64

enum { BT_CURSOR = 0, BT_RUNS = 1, BT_HDRS = 2, BT_HIST = 3, BT_META = 4 };

extern "C" uint64_t hmse_band_tables_bound(uint64_t n, uint32_t bands, uint32_t band_bits, uint32_t n_hashes) {
  (void)band_bits;
  // a band holds at most n headers (a piece holds at least one id)
  return BT_HEAD + (uint64_t)bands * (8 + 7 * n) + (n_hashes ? 12 + 4 * n * ((uint64_t)bands + n_hashes) : 0);
}

extern "C" size_t hmse_band_tables_workspace_bytes(uint64_t n) {
  const uint64_t nt = hmse_blocks(n, BT_NT);
  const uint64_t scan_len = 256 * nt > n + 1 ? 256 * nt : n + 1;
  // bkt/id ping-pong (4 x n), run flags, piece flags, run starts (n + 1), histogram (256 per tile), block sums, meta
  return 6 * hmse_align_up(4 * (n + 1), 256) + hmse_align_up(4 * 256 * nt, 256) + hmse_align_up(4 * (hmse_blocks(scan_len, BT_NT) + 1), 256) +
         hmse_align_up(8 * BT_META, 256) + 256;
}

__device__ __forceinline__ void bt_put(uint8_t* p, uint64_t v, int bytes) {
  for (int k = 0; k < bytes; k++) p[k] = (uint8_t)(v >> (8 * k));
}

__global__ __launch_bounds__(64) void bt_head_kernel(uint8_t* out, uint32_t bands, uint32_t band_bits, uint64_t n, uint64_t* meta) {
  const uint32_t t = threadIdx.x;
  const uint8_t magic[8] = {'H', 'M', 'S', 'E', 'B', 'A', 'N', 'D'};
  if (t < 8) out[t] = magic[t];
  if (t == 0) {
    bt_put(out + 8, 1, 4); bt_put(out + 12, bands, 4); bt_put(out + 16, band_bits, 4); bt_put(out + 20, 3, 4); bt_put(out + 24, n, 8);
    meta[BT_CURSOR] = BT_HEAD;
  }
}

// (bucket, id) of band b in id order
__global__ __launch_bounds__(BT_NT) void bt_load_kernel(const uint32_t* __restrict__ keys, uint64_t n, uint32_t bands, uint32_t b, uint32_t mask,
                                                       uint32_t* __restrict__ bkt, uint32_t* __restrict__ ids) {
  const uint64_t i = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
  if (i < n) { bkt[i] = keys[i * bands + b] & mask; ids[i] = (uint32_t)i; }
}

// stable rank of this thread's digit among the tile's valid elements with the same digit; wh = LDS u32[4][256].
// Every lane of the workgroup calls it (the ballots run with all lanes active).
__device__ __forceinline__ uint32_t bt_tile_rank(uint32_t d, bool valid, uint32_t* wh) {
  const uint32_t wave = threadIdx.x >> 6;
  for (uint32_t k = threadIdx.x; k < 4 * 256; k += BT_NT) wh[k] = 0;
  __syncthreads();
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < 8; bit++) {
    const bool on = (d >> bit) & 1u;
    const uint64_t bal = __ballot(on);
    m &= on ? bal : ~bal;
  }
  const uint32_t r = mbcnt64(m);
  if (valid && r == 0) wh[wave * 256 + d] = (uint32_t)__builtin_popcountll(m);
  __syncthreads();
  uint32_t pre = 0;
  for (uint32_t w = 0; w < wave; w++) pre += wh[w * 256 + d];
  return pre + r;
}

__global__ __launch_bounds__(BT_NT) void bt_hist_kernel(const uint32_t* __restrict__ bkt, uint64_t n, uint32_t shift, uint64_t n_tiles,
                                                       uint32_t* __restrict__ hist) {
  __shared__ uint32_t wh[4 * 256];
  const uint64_t i = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
  const bool valid = i < n;
  const uint32_t d = valid ? (bkt[i] >> shift) & 255u : 0u;
  bt_tile_rank(d, valid, wh);
  const uint32_t t = threadIdx.x;
  hist[(uint64_t)t * n_tiles + blockIdx.x] = wh[t] + wh[256 + t] + wh[512 + t] + wh[768 + t];
}

__global__ __launch_bounds__(BT_NT) void bt_scatter_kernel(const uint32_t* __restrict__ bkt, const uint32_t* __restrict__ ids, uint64_t n,
                                                          uint32_t shift, uint64_t n_tiles, const uint32_t* __restrict__ hist,
                                                          uint32_t* __restrict__ bkt_out, uint32_t* __restrict__ ids_out) {
  __shared__ uint32_t wh[4 * 256];
  const uint64_t i = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
  const bool valid = i < n;
  const uint32_t v = valid ? bkt[i] : 0u;
  const uint32_t d = (v >> shift) & 255u;
  const uint32_t r = bt_tile_rank(d, valid, wh);
  if (valid) {
    const uint64_t dst = (uint64_t)hist[(uint64_t)d * n_tiles + blockIdx.x] + r;
    if (dst < n) { bkt_out[dst] = v; ids_out[dst] = ids[i]; }
  }
}

__device__ __forceinline__ bool bt_is_start(const uint32_t* bkt, uint64_t i) { return i == 0 || bkt[i] != bkt[i - 1]; }

__global__ __launch_bounds__(BT_NT) void bt_start_kernel(const uint32_t* __restrict__ bkt, uint64_t n, uint32_t* __restrict__ runf) {
  const uint64_t i = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
  if (i < n) runf[i] = bt_is_start(bkt, i) ? 1u : 0u;
}

// runf (scanned) -> run_start[r] = first position of run r, run_start[R] = n
__global__ __launch_bounds__(BT_NT) void bt_runs_kernel(const uint32_t* __restrict__ bkt, uint64_t n, const uint32_t* __restrict__ runf,
                                                       const uint64_t* __restrict__ meta, uint32_t* __restrict__ run_start) {
  const uint64_t i = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
  if (i >= n) return;
  if (bt_is_start(bkt, i)) run_start[runf[i]] = (uint32_t)i;
  if (i == 0) run_start[meta[BT_RUNS]] = (uint32_t)n;
}

// a piece (one header) starts at every 65535th id of a run
__global__ __launch_bounds__(BT_NT) void bt_piece_kernel(const uint32_t* __restrict__ bkt, uint64_t n, const uint32_t* __restrict__ runf,
                                                        const uint32_t* __restrict__ run_start, uint32_t* __restrict__ pf) {
  const uint64_t i = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = runf[i] + (bt_is_start(bkt, i) ? 1u : 0u) - 1u;
  pf[i] = ((uint32_t)i - run_start[r]) % BT_PIECE == 0 ? 1u : 0u;
}

__global__ __launch_bounds__(BT_NT) void bt_emit_kernel(const uint32_t* __restrict__ bkt, const uint32_t* __restrict__ ids, uint64_t n,
                                                       const uint32_t* __restrict__ runf, const uint32_t* __restrict__ run_start,
                                                       const uint32_t* __restrict__ pf, const uint64_t* __restrict__ meta,
                                                       uint8_t* __restrict__ out, uint64_t out_cap, uint32_t* status) {
  const uint64_t i = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
  if (i >= n) return;
  const uint64_t base = meta[BT_CURSOR], H = meta[BT_HDRS];
  if (base + 8 + 4 * H + 3 * n > out_cap) {
    if (i == 0) atomicOr(status, 4u);
    return;
  }
  bt_put(out + base + 8 + 4 * H + 3 * i, ids[i], 3);
  const uint32_t r = runf[i] + (bt_is_start(bkt, i) ? 1u : 0u) - 1u;
  const uint32_t s = run_start[r];
  if (((uint32_t)i - s) % BT_PIECE == 0) {
    const uint32_t left = run_start[r + 1] - (uint32_t)i;
    bt_put(out + base + 8 + 4 * (uint64_t)pf[i], bkt[i], 2);
    bt_put(out + base + 8 + 4 * (uint64_t)pf[i] + 2, left < BT_PIECE ? left : BT_PIECE, 2);
  }
}

// the band's header count in front of it; the cursor moves behind the band
__global__ __launch_bounds__(64) void bt_advance_kernel(uint64_t* meta, uint64_t n, uint8_t* out, uint64_t out_cap, uint32_t* status) {
  if (threadIdx.x != 0) return;
  const uint64_t base = meta[BT_CURSOR], H = n ? meta[BT_HDRS] : 0;
  if (base + 8 + 4 * H + 3 * n > out_cap) { atomicOr(status, 4u); meta[BT_CURSOR] = out_cap; return; }
  bt_put(out + base, H, 8);
  meta[BT_CURSOR] = base + 8 + 4 * H + 3 * n;
}

// "HMSESIGS" | u32 n_hashes | keys | signatures, then the total size; one u32 word per thread and iteration
__global__ __launch_bounds__(BT_NT) void bt_sigs_kernel(const uint32_t* __restrict__ keys, uint64_t n_keys, const uint32_t* __restrict__ sig,
                                                       uint64_t n_sig, uint32_t n_hashes, const uint64_t* __restrict__ meta,
                                                       uint8_t* __restrict__ out, uint64_t out_cap, uint32_t* status) {
  const uint64_t base = meta[BT_CURSOR];
  if (base + 12 + 4 * (n_keys + n_sig) > out_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 4u);
    return;
  }
  const uint64_t g = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
  if (g == 0) {
    const uint8_t magic[8] = {'H', 'M', 'S', 'E', 'S', 'I', 'G', 'S'};
    for (int k = 0; k < 8; k++) out[base + k] = magic[k];
    bt_put(out + base + 8, n_hashes, 4);
  }
  uint8_t* dst = out + base + 12;
  const uint64_t stride = (uint64_t)gridDim.x * BT_NT;
  for (uint64_t w = g; w < n_keys + n_sig; w += stride) bt_put(dst + 4 * w, w < n_keys ? keys[w] : sig[w - n_keys], 4);
}

__global__ __launch_bounds__(64) void bt_finish_kernel(const uint64_t* meta, uint64_t tail, uint64_t* out_bytes) {
  if (threadIdx.x == 0) *out_bytes = meta[BT_CURSOR] + tail;
}

__global__ __launch_bounds__(64) void bt_status_kernel(uint32_t* status, uint32_t bits, uint64_t* out_bytes) {
  if (threadIdx.x == 0) { *status = bits; *out_bytes = 0; }
}

extern "C" int hmse_band_tables_write(const uint32_t* band_keys, uint64_t n, uint32_t bands, uint32_t band_bits, const uint32_t* sig,
                                      uint32_t n_hashes, uint8_t* out, uint64_t out_cap, uint64_t* out_bytes, uint32_t* status, void* ws,
                                      size_t ws_bytes, void* stream_) {
  HMSE_WS_ALIGNED(ws);
  if (!out_bytes || !status || !out || bands == 0) return HMSE_EINVAL;
  if (n && !band_keys) return HMSE_EINVAL;
  if (n && n_hashes && !sig) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  const uint32_t bad = (n >= (1ull << 24) ? 1u : 0u) | (band_bits == 0 || band_bits > 16 ? 2u : 0u);
  if (bad) {   // the numpy writer refuses the same inputs: 3-byte ids, a u16 band_hash
    bt_status_kernel<<<dim3(1), dim3(64), 0, stream>>>(status, bad, out_bytes);
    HMSE_LAUNCH_CHECK();
    return HMSE_OK;
  }
  const uint32_t nh = n_hashes;            // 0: no signature section
  if (out_cap < BT_HEAD) return HMSE_ENOSPC;
  if (!ws || ws_bytes < hmse_band_tables_workspace_bytes(n)) return HMSE_ENOSPC;
  const uint64_t nt = hmse_blocks(n, BT_NT);
  WsCarver c(ws, ws_bytes);
  uint32_t* bkt_a = c.take<uint32_t>(n + 1);
  uint32_t* id_a = c.take<uint32_t>(n + 1);
  uint32_t* bkt_b = c.take<uint32_t>(n + 1);
  uint32_t* id_b = c.take<uint32_t>(n + 1);
  uint32_t* runf = c.take<uint32_t>(n + 1);
  uint32_t* run_start = c.take<uint32_t>(n + 1);
  uint32_t* hist = c.take<uint32_t>(256 * nt);
  const uint64_t scan_len = 256 * nt > n + 1 ? 256 * nt : n + 1;
  uint32_t* bsum = c.take<uint32_t>(hmse_blocks(scan_len, BT_NT) + 1);
  uint64_t* meta = c.take<uint64_t>(BT_META);
  if (!c.ok()) return HMSE_ENOSPC;
  uint32_t* pf = hist;            // the piece flags reuse the histogram (256 per tile >= n)
  HMSE_FILL(status, 0, 4, stream);
  HMSE_FILL(meta, 0, 8 * BT_META, stream);
  bt_head_kernel<<<dim3(1), dim3(64), 0, stream>>>(out, bands, band_bits, n, meta);
  HMSE_LAUNCH_CHECK();
  const uint32_t mask = (uint32_t)((1ull << band_bits) - 1);
  const int passes = band_bits > 8 ? 2 : 1;
  for (uint32_t b = 0; b < bands; b++) {
    if (n) {
      bt_load_kernel<<<dim3((uint32_t)nt), dim3(BT_NT), 0, stream>>>(band_keys, n, bands, b, mask, bkt_a, id_a);
      HMSE_LAUNCH_CHECK();
      uint32_t *bi = bkt_a, *ii = id_a, *bo = bkt_b, *io = id_b;
      for (int p = 0; p < passes; p++) {
        bt_hist_kernel<<<dim3((uint32_t)nt), dim3(BT_NT), 0, stream>>>(bi, n, 8u * p, nt, hist);
        HMSE_LAUNCH_CHECK();
        int rc = device_exclusive_scan<uint32_t, BT_NT, BT_SCAN_NT>(hist, 256 * nt, bsum, meta + BT_HIST, stream);
        if (rc != HMSE_OK) return rc;
        bt_scatter_kernel<<<dim3((uint32_t)nt), dim3(BT_NT), 0, stream>>>(bi, ii, n, 8u * p, nt, hist, bo, io);
        HMSE_LAUNCH_CHECK();
        uint32_t* tb = bi; bi = bo; bo = tb;
        uint32_t* ti = ii; ii = io; io = ti;
      }
      bt_start_kernel<<<dim3((uint32_t)nt), dim3(BT_NT), 0, stream>>>(bi, n, runf);
      HMSE_LAUNCH_CHECK();
      int rc = device_exclusive_scan<uint32_t, BT_NT, BT_SCAN_NT>(runf, n, bsum, meta + BT_RUNS, stream);
      if (rc != HMSE_OK) return rc;
      bt_runs_kernel<<<dim3((uint32_t)nt), dim3(BT_NT), 0, stream>>>(bi, n, runf, meta, run_start);
      HMSE_LAUNCH_CHECK();
      bt_piece_kernel<<<dim3((uint32_t)nt), dim3(BT_NT), 0, stream>>>(bi, n, runf, run_start, pf);
      HMSE_LAUNCH_CHECK();
      rc = device_exclusive_scan<uint32_t, BT_NT, BT_SCAN_NT>(pf, n, bsum, meta + BT_HDRS, stream);
      if (rc != HMSE_OK) return rc;
      bt_emit_kernel<<<dim3((uint32_t)nt), dim3(BT_NT), 0, stream>>>(bi, ii, n, runf, run_start, pf, meta, out, out_cap, status);
      HMSE_LAUNCH_CHECK();
    }
    bt_advance_kernel<<<dim3(1), dim3(64), 0, stream>>>(meta, n, out, out_cap, status);
    HMSE_LAUNCH_CHECK();
  }
  uint64_t tail = 0;
  if (nh) {
    const uint64_t nk = n * bands, ns = n * nh;
    uint64_t blocks = hmse_blocks(nk + ns, BT_NT);
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    bt_sigs_kernel<<<dim3((uint32_t)blocks), dim3(BT_NT), 0, stream>>>(band_keys, nk, sig, ns, nh, meta, out, out_cap, status);
    HMSE_LAUNCH_CHECK();
    tail = 12 + 4 * (nk + ns);
  }
  bt_finish_kernel<<<dim3(1), dim3(64), 0, stream>>>(meta, tail, out_bytes);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}

// ---- near-duplicate index (hmse_l4_index_build, include/hmse.h): per band the stored ids sorted stably by the whole 32-bit key —
// the kernels above with mask 0xFFFFFFFF and four 8-bit passes.
size_t hmse_l4_index_workspace_bytes_impl(uint64_t n) {
  const uint64_t nt = hmse_blocks(n, BT_NT);
  // key/id ping-pong partner (2 x n), histogram (256 per tile), block sums, meta
  return 2 * hmse_align_up(4 * (n + 1), 256) + hmse_align_up(4 * 256 * nt, 256) + hmse_align_up(4 * (hmse_blocks(256 * nt, BT_NT) + 1), 256) +
         hmse_align_up(8 * BT_META, 256) + 256;
}

// ids [0, n) sorted stably by keys[i * stride + col] -> (out_keys, out_ids); an even pass count leaves the result there
static int bt_sort_u32(const uint32_t* keys, uint64_t n, uint32_t stride, uint32_t col, uint32_t* out_keys, uint32_t* out_ids, void* ws,
                       size_t ws_bytes, hipStream_t stream) {
  if (n == 0) return HMSE_OK;
  const uint64_t nt = hmse_blocks(n, BT_NT);
  WsCarver c(ws, ws_bytes);
  uint32_t* bkt = c.take<uint32_t>(n + 1);
  uint32_t* ids = c.take<uint32_t>(n + 1);
  uint32_t* hist = c.take<uint32_t>(256 * nt);
  uint32_t* bsum = c.take<uint32_t>(hmse_blocks(256 * nt, BT_NT) + 1);
  uint64_t* meta = c.take<uint64_t>(BT_META);
  if (!c.ok()) return HMSE_ENOSPC;
  bt_load_kernel<<<dim3((uint32_t)nt), dim3(BT_NT), 0, stream>>>(keys, n, stride, col, 0xFFFFFFFFu, out_keys, out_ids);
  HMSE_LAUNCH_CHECK();
  uint32_t *bi = out_keys, *ii = out_ids, *bo = bkt, *io = ids;
  for (int p = 0; p < 4; p++) {
    bt_hist_kernel<<<dim3((uint32_t)nt), dim3(BT_NT), 0, stream>>>(bi, n, 8u * p, nt, hist);
    HMSE_LAUNCH_CHECK();
    int rc = device_exclusive_scan<uint32_t, BT_NT, BT_SCAN_NT>(hist, 256 * nt, bsum, meta + BT_HIST, stream);
    if (rc != HMSE_OK) return rc;
    bt_scatter_kernel<<<dim3((uint32_t)nt), dim3(BT_NT), 0, stream>>>(bi, ii, n, 8u * p, nt, hist, bo, io);
    HMSE_LAUNCH_CHECK();
    uint32_t* tb = bi; bi = bo; bo = tb;
    uint32_t* ti = ii; ii = io; io = ti;
  }
  return HMSE_OK;
}

extern "C" int hmse_l4_index_build(const uint32_t* keys, uint64_t n, uint32_t bands, uint32_t* sorted_keys, uint32_t* sorted_ids,
                                   uint32_t* status, void* ws, size_t ws_bytes, void* stream_) {
  HMSE_WS_ALIGNED(ws);
  if (!status || bands == 0 || bands > 16 || (bands & (bands - 1))) return HMSE_EINVAL;
  if (n >= (1ull << 32)) return HMSE_EINVAL;
  if (n && (!keys || !sorted_keys || !sorted_ids)) return HMSE_EINVAL;
  if (n && (!ws || ws_bytes < hmse_l4_index_workspace_bytes_impl(n))) return HMSE_ENOSPC;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  PROF_BEGIN(HMSE_STAGE_L4_INDEX, stream);
  for (uint32_t b = 0; b < bands && n; b++) {
    int rc = bt_sort_u32(keys, n, bands, b, sorted_keys + (uint64_t)b * n, sorted_ids + (uint64_t)b * n, ws, ws_bytes, stream);
    if (rc != HMSE_OK) return rc;
  }
  PROF_END(HMSE_STAGE_L4_INDEX, stream);
  return HMSE_OK;
}
