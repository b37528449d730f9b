// hip_on_cpu.h — what the search emulators (find_emu, findset_emu, lines_emu, regex_emu) put under a HIP kernel to run it on the CPU: one
// std::thread per lane.  Include it after "hmse.h" and in front of hmse_amd/csrc/chunkmap.h and the kernels cut out of a .hip file.
// What differs stays with each emulator: its launcher (which sets g_bar where the kernels use __syncthreads), its stand-in for
// block_exclusive_scan, and the per-wavefront __ballot of lines_emu.
#pragma once
#include <barrier>
#include <cstdint>
#include <cstring>
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
static inline uint32_t emu_alignbyte(uint32_t hi, uint32_t lo, uint32_t b) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (b & 3))); }
#define __builtin_amdgcn_alignbyte emu_alignbyte
#define __builtin_amdgcn_readfirstlane(x) (x)
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
static inline uint4 load_u4_unaligned(const uint8_t* p) { uint4 v; memcpy(&v, p, 16); return v; }
static inline uint32_t load_u32_unaligned(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
