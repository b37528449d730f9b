/* hmse_tally.h — the C ABI of the TALLY of search results: which texts did the ranges of a search cover, and how often each
 * (hmse_amd/csrc/tally.hip, built into hmse_amd/csrc/libhmse_tally.so; bound by hmse_amd/_lib.py::TALLY_SIGNATURES; the grouping itself is
 * hmse_amd/find.py StoreFinder.tally).  An addition to include/hmse.h, which it includes: same conventions (status codes, stream-ordered
 * calls), same ABI version, the tables of hmse_lines_gather. */
#ifndef HMSE_TALLY_H
#define HMSE_TALLY_H
#include "hmse.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * Definitions (tests/tally_ref.py restates them in plain Python).  C is the N bytes read.read_store(store) returns.  There are n ranges
 * (start[i], end[i]) with start[i] <= end[i] <= N; each has a group g[i] in [0, G) (the pattern index).  The TEXT of i is
 * C[start[i] : end[i]).  With HMSE_FIND_IGNORE_CASE every byte first goes through fold_byte: A..Z become a..z, every other value (bytes
 * >= 0x80 included) stays as it is.  Empty ranges are legal and all equal each other.
 *
 * TALLY.  Per group, the distinct texts among the group's ranges; for each distinct text its `count` (the ranges that have it) and its
 * REPRESENTATIVE: the member with the smallest start, ties broken by the smallest index i.  Order within a group: count descending, then
 * the representative's start ascending, then the representative's index.  With top = k only the first k values per group are kept;
 * distinct[g] still reports all of them.
 *
 * KEY.  f(b) is the byte after folding (or the byte itself), L the length, t the index of a byte in its text.
 *   a1 = sum_t (f(b_t) + 1) * M1^t  mod 2^32,  M1 = 0x9E3779B1          a2 = the same sum with M2 = 0x85EBCA6B
 *   x  = (a1 | a2 << 32) ^ (L * 0x9E3779B97F4A7C15) ^ (seed * 0xD6E8FEB86659FD93)  mod 2^64
 *   the murmur3 64-bit finaliser: x ^= x >> 33; x *= 0xFF51AFD7ED558CCD; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53; x ^= x >> 33
 *   key = x & (2^key_bits - 1),  1 <= key_bits <= 64
 * The key only BUCKETS ranges; it never decides equality (hmse_tally_same does, byte by byte).  key_bits exists so that tests can force
 * collisions at small sizes.
 *
 * hmse_tally_keys: key[i] = the key of range i, for every i.
 * hmse_tally_same: same[i] = 1 iff the ranges i and rep[i] have the same length and the same (folded) bytes, else 0; rep[i] == i and a
 * length mismatch are answered without reading a byte.
 * The tables raw / raw_off / cuts / slot are those of hmse_lines_gather: corpus byte q of chunk k is raw[raw_off[slot[k]] + q - cuts[k]];
 * a range may cross any number of chunks, chunks may be 0, 1 or 2 bytes long.
 *
 * status (u32, cleared by the call): bit 1 = tables that break a rule of the chunk map (cuts[0] != 0 included), a range with
 * start > end or end > N, or a rep[i] >= n.  With bit 1 nothing is read through the tables and every output element is 0.  Bit 0 is
 * never set.  The outputs are written for every i: the caller clears nothing.
 * HMSE_EINVAL before anything is cleared or launched: a NULL status, a NULL pointer to a non-empty array, n >= 2^33, flag bits other
 * than HMSE_FIND_IGNORE_CASE, key_bits outside 1..64.
 * No workspace, no LDS; stream-ordered, allocate nothing, never sync.  Both main kernels report in profile slot 31
 * (HMSE_STAGE_FIND_PLACE), shared with the other search kernels: reset it first.
 * Out of scope: texts compared under anything but byte or ASCII-folded equality, weighting occurrences, lexicographic ordering of values,
 * tallying across several stores, several short ranges packed into one wavefront, approximate (k-error) grouping of values.
 */
#define HMSE_TALLY_M1    0x9E3779B1u
#define HMSE_TALLY_M2    0x85EBCA6Bu
#define HMSE_TALLY_LEN   0x9E3779B97F4A7C15ull
#define HMSE_TALLY_SEED  0xD6E8FEB86659FD93ull
#define HMSE_TALLY_MIX1  0xFF51AFD7ED558CCDull
#define HMSE_TALLY_MIX2  0xC4CEB9FE1A85EC53ull

int hmse_tally_keys(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                    const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, uint64_t n, uint32_t flags,
                    uint64_t seed, uint32_t key_bits, uint64_t* key, uint32_t* status, void* stream);
int hmse_tally_same(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                    const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* rep, uint64_t n,
                    uint32_t flags, uint8_t* same, uint32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HMSE_TALLY_H */
