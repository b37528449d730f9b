// l4_query.hip — near-duplicate search over the stored chunks' MinHash signatures (hmse_l4_query, include/hmse.h).
//
// The index (bandtable.hip, hmse_l4_index_build) holds, per band, the stored ids sorted by their 32-bit band key.  A query batch
// runs in three steps:
//   probe  one lane per (query, band) binary-searches the query's key in that band's sorted keys: the run [lo, hi) of ids with an
//          equal key.  The query's work bound is w_i = sum over bands of (hi - lo).
//   score  a persistent grid of one-wavefront workgroups takes queries from an atomic hand-out counter (no spin-waits).  The
//          wavefront compares one candidate c at a time: lane l loads S_c[2l..2l+1] (8 bytes a lane: the 512-byte row, coalesced)
//          and compares it with the query's words, which it holds in registers.  Two ballots give the 128-bit equality mask; the
//          score is its popcount, band b' is equal iff its `rows` bits are all set.  c counts in the run of band b only if band b is
//          equal and no band b' < b is: a candidate found in several runs counts once, an equal key with different rows never, and
//          n_candidates is exact.  Hits go to an LDS buffer as packed (score << 32 | ~id) keys, so that a larger key is a better
//          hit (score descending, id ascending); when the buffer fills, and at the end, a rank pass reduces it to the top_k best and
//          raises the admission threshold to the k-th best.
// Queries are handed out in id order.  Handing them out heaviest first (sorted by w_i with the index's radix sort) was measured and
// not kept: the 10 GB self-join took 18.0 ms that way against 14.9 ms in id order (profiles/r5/).
// Every loop bound of the score kernel is wave-uniform and scalar (readfirstlane of uniform loads, ballot results), so no cross-lane
// instruction sits in a divergent loop (tools/isa_audit.py).
#include "common.h"

constexpr int QY_NT = 64;             // one wavefront per workgroup: one query at a time
constexpr uint32_t QY_CAP = 256;      // LDS hit buffer before a reduction to top_k (> 64 >= top_k)
constexpr uint32_t QY_GRID = 8192;    // persistent workgroups (256 CUs x 32 wavefronts)
constexpr int QY_U = 4;               // candidate rows in flight per wavefront

size_t hmse_l4_query_workspace_bytes_impl(uint64_t n_q, const hmse_cfg* cfg) {
  // runs (lo, hi per query and band), hand-out counter
  return hmse_align_up(8 * n_q * cfg->bands, 256) + 256;
}

__device__ __forceinline__ uint32_t qy_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// one lane per (query, band): [first key >= k, first key > k) in the band's sorted keys
__global__ __launch_bounds__(256) void qy_probe_kernel(const uint32_t* __restrict__ keys_q, uint64_t n_q, uint32_t bands,
                                                      const uint32_t* __restrict__ sorted_keys, uint64_t n_s, uint32_t* __restrict__ runs) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_q * bands) return;
  const uint32_t b = (uint32_t)(g % bands);
  const uint32_t key = keys_q[g];
  const uint32_t* a = sorted_keys + (uint64_t)b * n_s;
  uint32_t lo = 0, hi = (uint32_t)n_s;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  uint32_t lo2 = lo, hi2 = (uint32_t)n_s;
  while (lo2 < hi2) {
    const uint32_t mid = lo2 + ((hi2 - lo2) >> 1);
    if (a[mid] <= key) lo2 = mid + 1; else hi2 = mid;
  }
  runs[2 * g] = lo;
  runs[2 * g + 1] = lo2;
}

// the next query of the hand-out, in every lane (SGPR)
__device__ __forceinline__ uint32_t qy_next(uint32_t* ctr, uint32_t* slot) {
  if (threadIdx.x == 0) *slot = atomicAdd(ctr, 1u);
  __syncthreads();
  const uint32_t t = qy_uni(*slot);
  __syncthreads();
  return t;
}

// rank pass over the `cnt` (distinct) keys of buf: the best min(cnt, k) of them, descending, in buf[0..); k <= 64
__device__ __forceinline__ uint32_t qy_reduce(uint64_t* buf, uint64_t* top, uint32_t cnt, uint32_t k) {
  __syncthreads();
  for (uint32_t e0 = 0; e0 < cnt; e0 += QY_NT) {
    const uint32_t e = e0 + threadIdx.x;
    const uint64_t v = e < cnt ? buf[e] : 0ull;
    uint32_t r = 0;
    for (uint32_t t = 0; t < cnt; t++) r += buf[t] > v ? 1u : 0u;
    if (e < cnt && r < k) top[r] = v;
  }
  __syncthreads();
  const uint32_t kept = cnt < k ? cnt : k;
  if (threadIdx.x < kept) buf[threadIdx.x] = top[threadIdx.x];
  __syncthreads();
  return kept;
}

__global__ __launch_bounds__(QY_NT) void qy_score_kernel(const uint32_t* __restrict__ sig_q, uint32_t n_q, const uint32_t* __restrict__ sig_s,
                                                        uint32_t n_s, const uint32_t* __restrict__ sorted_ids, const uint32_t* __restrict__ runs,
                                                        uint32_t bands, uint32_t rows, uint32_t top_k, uint32_t min_score, uint32_t flags,
                                                        uint32_t* ctr, int64_t* __restrict__ out_ids, int32_t* __restrict__ out_scores,
                                                        uint32_t* __restrict__ n_hits, uint64_t* __restrict__ n_cand, uint32_t* status) {
  __shared__ uint64_t buf[QY_CAP];
  __shared__ uint64_t top[QY_NT];
  __shared__ uint32_t next;
  const uint32_t lane = threadIdx.x;
  const uint32_t half = rows >> 1;                                  // mask bits per band: lane l holds hashes 2l and 2l + 1
  const uint64_t bmask = half >= 64 ? ~0ull : (1ull << half) - 1;
  const bool excl = (flags & HMSE_QUERY_EXCLUDE_SELF) != 0;
  // one exit, no `continue`: the hand-out loop stays a scalar loop (an extra exit made the structuriser mask it with EXEC)
  for (uint32_t i = qy_next(ctr, &next); i < n_q; i = qy_next(ctr, &next)) {
    const uint2 qv = reinterpret_cast<const uint2*>(sig_q + (uint64_t)i * 128)[lane];
    uint32_t cnt = 0, bad = 0;
    uint64_t thr = 0, ncand = 0;
    for (uint32_t b = 0; b < bands; b++) {
      const uint64_t r = 2 * ((uint64_t)i * bands + b);
      const uint32_t lo = qy_uni(runs[r]), hi = qy_uni(runs[r + 1]);
      const uint32_t* ids_b = sorted_ids + (uint64_t)b * n_s;
      for (uint32_t j = lo; j < hi; j += QY_U) {
        uint32_t c[QY_U];
        uint2 sv[QY_U];
#pragma unroll
        for (int u = 0; u < QY_U; u++) {
          c[u] = j + u < hi ? qy_uni(ids_b[j + u]) : 0xFFFFFFFFu;
          sv[u] = c[u] < n_s ? reinterpret_cast<const uint2*>(sig_s + (uint64_t)c[u] * 128)[lane] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < QY_U; u++) {
          if (j + u >= hi) break;
          if (c[u] >= n_s) { bad = 1; continue; }
          if (excl && c[u] == i) continue;
          const uint64_t m0 = __ballot(sv[u].x == qv.x), m1 = __ballot(sv[u].y == qv.y);
          const uint64_t m = m0 & m1;
          uint32_t first = bands;
          for (uint32_t bb = 0; bb <= b; bb++) {
            if (((m >> (bb * half)) & bmask) == bmask) { first = bb; break; }
          }
          if (first != b) continue;                                 // a collision, or counted in an earlier band's run
          ncand++;
          const uint32_t score = (uint32_t)__builtin_popcountll(m0) + (uint32_t)__builtin_popcountll(m1);
          if (score < min_score) continue;
          const uint64_t key = ((uint64_t)score << 32) | (uint64_t)(~c[u]);
          if (key <= thr) continue;
          if (lane == 0) buf[cnt] = key;
          cnt++;
          if (cnt == QY_CAP) {
            cnt = qy_reduce(buf, top, cnt, top_k);
            const uint64_t kth = buf[top_k - 1];
            thr = ((uint64_t)qy_uni((uint32_t)(kth >> 32)) << 32) | qy_uni((uint32_t)kth);
          }
        }
      }
    }
    if (cnt) cnt = qy_reduce(buf, top, cnt, top_k);
    if (lane < top_k) {
      const bool h = lane < cnt;
      const uint64_t v = h ? buf[lane] : 0ull;
      out_ids[(uint64_t)i * top_k + lane] = h ? (int64_t)(uint32_t)~(uint32_t)v : (int64_t)-1;
      out_scores[(uint64_t)i * top_k + lane] = h ? (int32_t)(v >> 32) : 0;
    }
    if (lane == 0) {
      n_hits[i] = cnt;
      n_cand[i] = ncand;
      if (bad) atomicOr(status, 1u);
    }
  }
}

extern "C" int hmse_l4_query(const uint32_t* sig_q, const uint32_t* keys_q, uint64_t n_q, const uint32_t* sig_s, uint64_t n_s,
                             const uint32_t* sorted_keys, const uint32_t* sorted_ids, const hmse_cfg* cfg, uint32_t top_k, uint32_t min_score,
                             uint32_t flags, int64_t* out_ids, int32_t* out_scores, uint32_t* n_hits, uint64_t* n_candidates, uint32_t* status,
                             void* ws, size_t ws_bytes, void* stream_) {
  HMSE_WS_ALIGNED(ws);
  if (hmse_cfg_validate_impl(cfg) != 0) return HMSE_EINVAL;
  if (top_k < 1 || top_k > 64 || min_score > 128 || (flags & ~(uint32_t)HMSE_QUERY_EXCLUDE_SELF)) return HMSE_EINVAL;
  if (n_q >= (1ull << 32) || n_s >= (1ull << 32) || !status) return HMSE_EINVAL;
  if (n_q && (!sig_q || !keys_q || !out_ids || !out_scores || !n_hits || !n_candidates)) return HMSE_EINVAL;
  if (n_s && (!sig_s || !sorted_keys || !sorted_ids)) return HMSE_EINVAL;
  const uint32_t bands = cfg->bands;
  uint32_t *runs = nullptr, *ctr = nullptr;
  if (n_q) {
    WsCarver c(ws, ws_bytes);
    runs = c.take<uint32_t>(2 * n_q * bands);
    ctr = c.take<uint32_t>(64);
    if (!c.ok()) return HMSE_ENOSPC;
  }
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  HMSE_FILL(status, 0, 4, stream);
  if (n_q == 0) return HMSE_OK;
  HMSE_FILL(ctr, 0, 4, stream);
  const uint64_t nb = n_q * bands;
  qy_probe_kernel<<<dim3((uint32_t)((nb + 255) / 256)), dim3(256), 0, stream>>>(keys_q, n_q, bands, sorted_keys, n_s, runs);
  HMSE_LAUNCH_CHECK();
  const uint32_t grid = n_q < QY_GRID ? (uint32_t)n_q : QY_GRID;
  PROF_BEGIN(HMSE_STAGE_L4_QUERY, stream);
  qy_score_kernel<<<dim3(grid), dim3(QY_NT), 0, stream>>>(sig_q, (uint32_t)n_q, sig_s, (uint32_t)n_s, sorted_ids, runs, bands, cfg->rows,
                                                         top_k, min_score, flags, ctr, out_ids, out_scores, n_hits, n_candidates, status);
  HMSE_LAUNCH_CHECK();
  PROF_END(HMSE_STAGE_L4_QUERY, stream);
  return HMSE_OK;
}
