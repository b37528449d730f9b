// blockops.h — the copies and scans that more than one translation unit needs, once: a record copied by one wavefront (gc.hip,
// lines.hip) or by one workgroup (l1_inflate.hip, manifest_pack.hip), the scan of per-block sums by one workgroup (gc.hip, scrub.hip)
// and the device-wide exclusive scan built on it (bandtable.hip; l1_deflate.hip's u64 scan shares the block-sum kernel only).  The .hip files
// include this after common.h; tools/lines_emu.cpp includes it after tools/hip_on_cpu.h, so the device part uses only what both provide
// and the file includes nothing.  Everything here is a template or __forceinline__: several translation units include it and link
// into one library.
#pragma once

// ---- copies -------------------------------------------------------------------------------------------------------------------
// One wavefront copies len bytes.  head: the bytes up to the destination's next 16-byte boundary, one per lane; body: 16-byte stores at
// aligned destinations (loads from wherever the source starts); tail: the last < 16 bytes, one per lane.
__device__ __forceinline__ void wave_copy(uint8_t* d, const uint8_t* s, uint64_t len, uint32_t lane) {
  uint64_t head = (16 - ((uintptr_t)d & 15)) & 15;
  if (head > len) head = len;
  if (lane < head) d[lane] = s[lane];
  const uint64_t body = (len - head) & ~(uint64_t)15;
  const uint8_t* sb = s + head;
  uint4* db = (uint4*)(d + head);
  for (uint64_t o = (uint64_t)lane * 16; o < body; o += 64 * 16) db[o >> 4] = load_u4_unaligned(sb + o);
  const uint64_t t0 = head + body;
  if (t0 + lane < len) d[t0 + lane] = s[t0 + lane];
}

// One workgroup of NT threads copies len bytes (LEN: uint32_t or uint64_t), 16 per thread and trip from and to any alignment; the thread
// that meets the end copies the last < 16 bytes one by one.
template <int NT, typename LEN>
__device__ __forceinline__ void block_copy(uint8_t* dst, const uint8_t* src, LEN len) {
  for (LEN b = (LEN)threadIdx.x * 16; b < len; b += NT * 16) {
    if (b + 16 <= len) { const uint4 v = load_u4_unaligned(src + b); __builtin_memcpy(dst + b, &v, 16); }
    else for (LEN j = b; j < len; j++) dst[j] = src[j];
  }
}

// ---- scans --------------------------------------------------------------------------------------------------------------------
// Exclusive scan of nb block sums in place by ONE workgroup, *total = the sum >> SHR (the loop's trip count is a kernel argument, or
// with PER != 0 and n_dev != nullptr the blocks of PER elements that *n_dev elements fill).
template <int NT, int SHR = 0, typename T = uint32_t, int PER = 0>
__global__ __launch_bounds__(NT) void block_sums_scan_kernel(T* __restrict__ bsum, uint64_t nb, uint64_t* __restrict__ total,
                                                             const uint64_t* __restrict__ n_dev) {
  __shared__ T red[NT / 64 + 1];
  if (PER && n_dev) nb = (*n_dev + PER - 1) / PER;
  T carry = 0;
  for (uint64_t b0 = 0; b0 < nb; b0 += NT) {
    const uint64_t i = b0 + threadIdx.x;
    const T v = i < nb ? bsum[i] : (T)0;
    T tot;
    const T ex = block_exclusive_scan<NT>(v, red, &tot);
    if (i < nb) bsum[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry >> SHR;
}

// The device-wide exclusive scan of a[0, n) in place: block sums, one workgroup over them, then per block (trip counts: kernel arguments).
template <typename T, int NT>
__global__ __launch_bounds__(NT) void scan_reduce_kernel(const T* __restrict__ a, uint64_t n, T* __restrict__ bsum) {
  __shared__ T red[NT / 64 + 1];
  const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  T tot;
  block_exclusive_scan<NT>(i < n ? a[i] : (T)0, red, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

template <typename T, int NT>
__global__ __launch_bounds__(NT) void scan_apply_kernel(T* __restrict__ a, uint64_t n, const T* __restrict__ bsum) {
  __shared__ T red[NT / 64 + 1];
  const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  const T v = i < n ? a[i] : (T)0;
  T tot;
  const T ex = bsum[blockIdx.x] + block_exclusive_scan<NT>(v, red, &tot);
  if (i < n) a[i] = ex;
}

// ---- host side (the library only) ---------------------------------------------------------------------------------------------
#ifdef __HIPCC__
// bsum: hmse_blocks(n, NT) + 1 entries of T; *total (device) = the sum
template <typename T, int NT, int SCAN_NT>
static int device_exclusive_scan(T* a, uint64_t n, T* bsum, uint64_t* total, hipStream_t stream) {
  const uint64_t nb = hmse_blocks(n, NT);
  scan_reduce_kernel<T, NT><<<dim3((uint32_t)nb), dim3(NT), 0, stream>>>(a, n, bsum);
  HMSE_LAUNCH_CHECK();
  block_sums_scan_kernel<SCAN_NT, 0, T><<<dim3(1), dim3(SCAN_NT), 0, stream>>>(bsum, nb, total, nullptr);
  HMSE_LAUNCH_CHECK();
  scan_apply_kernel<T, NT><<<dim3((uint32_t)nb), dim3(NT), 0, stream>>>(a, n, bsum);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
#endif
