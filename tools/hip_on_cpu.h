// hip_on_cpu.h — what the emulators (find_emu, findset_emu, lines_emu, regex_emu in both its forms, approx_emu, export_emu, sync_emu, gunzip_emu, inflate_emu, tally_emu, order_emu) put under a HIP kernel to run it on the CPU:
// one std::thread per lane, a std::barrier under __syncthreads and one per wavefront under __ballot (a loop that is not wave-uniform hangs
// it), a plain prefix sum for block_exclusive_scan, and the launcher.  Include it after "hmse.h" and in front of hmse_amd/csrc/chunkmap.h,
// blockops.h and the kernels cut out of a .hip file.
#pragma once
#include <barrier>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __restrict__
#define __launch_bounds__(...)
struct Idx { uint32_t x; };
static thread_local Idx threadIdx, blockIdx;
static Idx gridDim;
static std::barrier<>* g_bar;                            // the workgroup's barrier, set by the emulator's launcher
static inline void __syncthreads() { g_bar->arrive_and_wait(); }
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t atomicXor(uint32_t* p, uint32_t v) { return __atomic_fetch_xor(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t emu_alignbyte(uint32_t hi, uint32_t lo, uint32_t b) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (b & 3))); }
#define __builtin_amdgcn_alignbyte emu_alignbyte
#define __builtin_amdgcn_readfirstlane(x) (x)
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
static inline uint4 load_u4_unaligned(const uint8_t* p) { uint4 v; memcpy(&v, p, 16); return v; }
static inline uint32_t load_u32_unaligned(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static inline uint32_t lane_id() { return threadIdx.x & 63u; }
static inline uint32_t mbcnt64(uint64_t m) { return (uint32_t)__builtin_popcountll(m & ((1ull << lane_id()) - 1ull)); }
template <int NT, typename T> static inline T block_exclusive_scan(T v, T*, T* total) {
  static T arr[NT];
  arr[threadIdx.x] = v;
  __syncthreads();
  T pre = 0, tot = 0;
  for (int i = 0; i < NT; i++) { if ((uint32_t)i < threadIdx.x) pre += arr[i]; tot += arr[i]; }
  __syncthreads();
  *total = tot;
  return pre;
}
// a ballot of the 64 lanes of one wavefront: every lane of the wavefront must arrive (the kernels' loops are wave-uniform, or this hangs)
static unsigned long long g_bits[16];
static std::barrier<>* g_wave[16];
static inline unsigned long long __ballot(int p) {
  const uint32_t w = threadIdx.x >> 6;
  if (p) __atomic_fetch_or(&g_bits[w], 1ull << lane_id(), __ATOMIC_SEQ_CST);
  g_wave[w]->arrive_and_wait();
  const unsigned long long v = __atomic_load_n(&g_bits[w], __ATOMIC_SEQ_CST);
  g_wave[w]->arrive_and_wait();
  if (lane_id() == 0) __atomic_store_n(&g_bits[w], 0ull, __ATOMIC_SEQ_CST);
  g_wave[w]->arrive_and_wait();
  return v;
}
// The wave-level reads of the one-stream-per-wavefront decoders (hmse_amd/csrc/inflate_core.h, gunzip.hip; launch_waves only): every lane
// publishes its value, the wavefront meets, every lane reads lane j's.  uni32 / uni64 (common.h: readfirstlane) are the same read of
// lane 0, so a value that is NOT uniform — or a loop that is not — shows here as a wrong result or a hang instead of passing unnoticed.
static uint32_t g_lanes[16][64];
static inline uint32_t emu_readlane(uint32_t v, uint32_t j) {
  const uint32_t w = threadIdx.x >> 6;
  g_lanes[w][lane_id()] = v;
  g_wave[w]->arrive_and_wait();
  const uint32_t r = g_lanes[w][j & 63u];
  g_wave[w]->arrive_and_wait();
  return r;
}
#define __builtin_amdgcn_readlane(v, j) ((int)emu_readlane((uint32_t)(v), (uint32_t)(j)))
static inline uint32_t uni32(uint32_t v) { return emu_readlane(v, 0); }
static inline uint64_t uni64(uint64_t v) { return ((uint64_t)uni32((uint32_t)(v >> 32)) << 32) | uni32((uint32_t)v); }
static inline uint64_t lanemask_lt() { return (1ull << lane_id()) - 1ull; }
static inline void emu_wave_barrier() { g_wave[threadIdx.x >> 6]->arrive_and_wait(); }
#define __builtin_amdgcn_wave_barrier emu_wave_barrier
#define __builtin_amdgcn_fence(...) __atomic_thread_fence(__ATOMIC_SEQ_CST)
#ifndef __clang__
static inline uint32_t emu_bitreverse32(uint32_t x) {
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
  return __builtin_bswap32(x);
}
#define __builtin_bitreverse32 emu_bitreverse32
#endif
static inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
// The scoped atomics and the sleep of the decoders' hand-off between streams (hmse_amd/csrc/l1_inflate.hip: a DELTA record polls its base's
// flag): sequentially consistent here, and a poll gives the core away.  (Its s_waitcnt and register-pinning asm statements and its
// ext_vector_type typedef are replaced where tools/inflate_emu.py cuts the kernels out.)
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __HIP_MEMORY_SCOPE_SYSTEM 0
#define __hip_atomic_load(p, order, scope) __atomic_load_n((p), __ATOMIC_SEQ_CST)
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n((p), (v), __ATOMIC_SEQ_CST)
static inline void emu_sleep(int) { std::this_thread::yield(); }
#define __builtin_amdgcn_s_sleep emu_sleep
// grid workgroups of NT threads, one after the other.  launch_block: for kernels that meet at __syncthreads (a thread that returns leaves
// the barrier: arrive_and_drop).  launch_waves: for kernels whose wavefronts meet only at __ballot and return as a whole.
template <int NT> static void launch_block(uint32_t grid, const std::function<void()>& f) {
  gridDim.x = grid;
  for (uint32_t b = 0; b < grid; b++) {
    std::barrier<> bar(NT);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (int t = 0; t < NT; t++) th.emplace_back([&, t, b] { threadIdx.x = t; blockIdx.x = b; f(); bar.arrive_and_drop(); });
    for (auto& x : th) x.join();
  }
}
template <int NT> static void launch_waves(uint32_t grid, const std::function<void()>& f) {
  gridDim.x = grid;
  for (uint32_t b = 0; b < grid; b++) {
    std::unique_ptr<std::barrier<>> wave[NT / 64];
    for (int w = 0; w < NT / 64; w++) { wave[w].reset(new std::barrier<>(64)); g_wave[w] = wave[w].get(); }
    memset(g_bits, 0, sizeof g_bits);
    std::vector<std::thread> th;
    for (int t = 0; t < NT; t++) th.emplace_back([&, t, b] { threadIdx.x = t; blockIdx.x = b; f(); });
    for (auto& x : th) x.join();
  }
}
