// sync.hip — replication of a store onto an older copy (hmse_amd/sync.py): the byte proof behind a digest join.
//
// Equal SHA-256 digests say that two records decode to the same chunk, not that their STORED bytes are equal: the same chunk is FULL
// in one store and DELTA in the other, or DELTA against another dictionary.  A patch that copies on digest equality alone builds a blob
// that is not the wanted one.  hmse_sync_match compares the stored stream of every record of the wanted store (a) with the stream of
// its candidate in the store the replica holds (b) and answers one byte per record.
//
// One wavefront per record (streams are at most about 32 KiB; gc_gather_kernel is the model).  head: the bytes up to a's next 16-byte
// boundary, one per lane; tail: the last < 16 bytes, one per lane; body: 16 bytes per lane and side, 1 KiB per trip, loaded from
// wherever each side starts (lba_unit may be 1: the two sides are misaligned independently).  The trip loop is wave-uniform — its
// counter is a scalar and its exit a ballot all 64 lanes take — and is left at the first trip that differs.
#include "common.h"

constexpr int SYNC_NT = 256;                 // four wavefronts = four records per workgroup
constexpr uint32_t SYNC_TRIP = 64 * 16;      // bytes of each side one trip compares

__global__ __launch_bounds__(SYNC_NT) void sync_match_kernel(const uint8_t* __restrict__ a, uint64_t a_bytes, const uint64_t* __restrict__ a_off,
                                                            const uint32_t* __restrict__ a_len, uint64_t n, const uint8_t* __restrict__ b,
                                                            uint64_t b_bytes, const uint64_t* __restrict__ b_off, const uint32_t* __restrict__ b_len,
                                                            uint64_t n_b, const int64_t* __restrict__ cand, uint8_t* __restrict__ same,
                                                            uint32_t* status) {
  const uint64_t k = (uint64_t)blockIdx.x * (SYNC_NT / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (k >= n) return;
  const uint32_t lane = lane_id();
  const int64_t c = cand[k];
  bool bad = false;
  uint64_t any = 1;                                    // lanes that saw a difference; stays non-zero unless the streams were compared
  if (c >= 0) {
    if ((uint64_t)c >= n_b) bad = true;
    else {
      const uint64_t ao = a_off[k], bo = b_off[c];
      const uint32_t len = a_len[k], lb = b_len[c];
      if (ao > a_bytes || len > a_bytes - ao || bo > b_bytes || lb > b_bytes - bo) bad = true;
      else if (len == lb) {
        const uint8_t* pa = a + ao;
        const uint8_t* pb = b + bo;
        uint32_t head = (16u - (uint32_t)((uintptr_t)pa & 15u)) & 15u;
        if (head > len) head = len;
        const uint32_t body = (len - head) & ~15u, t0 = head + body;
        bool d = false;
        if (lane < head) d = pa[lane] != pb[lane];
        if (t0 + lane < len) d = d || pa[t0 + lane] != pb[t0 + lane];
        any = __ballot(d);
        const uint8_t* qa = pa + head;
        const uint8_t* qb = pb + head;
        for (uint32_t o = 0; any == 0 && o < body; o += SYNC_TRIP) {
          const uint32_t p = o + lane * 16u;
          bool e = false;
          if (p < body) {
            const uint4 x = load_u4_unaligned(qa + p), y = load_u4_unaligned(qb + p);
            e = ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0u;
          }
          any = __ballot(e);
        }
      }
    }
  }
  if (lane == 0) {
    same[k] = (uint8_t)(any == 0);
    if (bad) atomicOr(status, 1u);
  }
}

// ---- entry point ------------------------------------------------------------------------------------------------------------
extern "C" int hmse_sync_match(const uint8_t* a, uint64_t a_bytes, const uint64_t* a_off, const uint32_t* a_len, uint64_t n, const uint8_t* b,
                               uint64_t b_bytes, const uint64_t* b_off, const uint32_t* b_len, uint64_t n_b, const int64_t* cand,
                               uint8_t* same, uint32_t* status, void* stream_) {
  if (!status) return HMSE_EINVAL;
  if (n && (!a_off || !a_len || !cand || !same || (!a && a_bytes) || (!b && b_bytes) || (n_b && (!b_off || !b_len)))) return HMSE_EINVAL;
  if (n >= (1ull << 33)) return HMSE_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n == 0) return HMSE_OK;
  const uint64_t blocks = (n + SYNC_NT / 64 - 1) / (SYNC_NT / 64);
  PROF_BEGIN(HMSE_STAGE_SYNC_MATCH, stream);
  sync_match_kernel<<<dim3((uint32_t)blocks), dim3(SYNC_NT), 0, stream>>>(a, a_bytes, a_off, a_len, n, b, b_bytes, b_off, b_len, n_b, cand, same,
                                                                         status);
  PROF_END(HMSE_STAGE_SYNC_MATCH, stream);
  HMSE_LAUNCH_CHECK();
  return HMSE_OK;
}
