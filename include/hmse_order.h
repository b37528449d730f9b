/* hmse_order.h — the C ABI of the ORDER of search results: the ranges of a search sorted by the texts they cover, as Python orders bytes
 * (hmse_amd/csrc/order.hip, built into hmse_amd/csrc/libhmse_order.so; bound by hmse_amd/_lib.py::ORDER_SIGNATURES; the rounds themselves
 * are hmse_amd/find.py order_ranges / StoreFinder.sort).  An addition to include/hmse.h, which it includes: same conventions (status codes,
 * stream-ordered calls), same ABI version, the tables of hmse_lines_gather. */
#ifndef HMSE_ORDER_H
#define HMSE_ORDER_H
#include "hmse.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * Definitions (tests/order_ref.py restates them in plain Python).  C is the N bytes read.read_store(store) returns.  There are n ranges
 * (start[i], end[i]) with start[i] <= end[i] <= N; each has a group g[i] in [0, G).  The TEXT of i is C[start[i] : end[i]), L_i its
 * length.  With HMSE_FIND_IGNORE_CASE every byte first goes through fold_byte: exactly A..Z become a..z, every other value (bytes >= 0x80
 * included) stays as it is.
 *
 * ORDER.  Within a group the texts are ordered as Python orders bytes: unsigned, byte by byte, a proper prefix first, the empty text
 * first of all.  Ranges with equal (folded) texts are ordered by (start, index): the order is total and deterministic,
 *   sorted(range(n), key=lambda i: (g[i], fold(text(i)), start[i], i)).
 *
 * KEY.  Seven bytes of the text and the state of its end at depth d, 0 <= d <= L; b_t is the folded byte t, 0 beyond the end:
 *   r   = min(L - d, 8)
 *   key = ((sum over j = 0..6 of b_{d+j} << 8 * (6 - j)) << 4) | r                  (below 2^60: it sorts as a signed int64 as well)
 * For two texts that agree in their first d bytes, key_a < key_b implies text_a < text_b; equal keys with r <= 7 mean the texts are equal;
 * equal keys with r = 8 mean they agree through d + 7, and the comparison continues there.  r tells a padding zero from a true zero byte:
 * the shorter text is the prefix and has the smaller r.
 *
 * LCP.  Range i has a partner rep[i] and a from[i] <= min(L_i, L_rep[i]); the caller promises that the first from[i] bytes of the two
 * texts agree, and they are not read.  lcp[i] = from[i] + the number of (folded) bytes that agree from text index from[i] on, at most
 * min(L_i, L_rep[i]).  rep[i] == i answers L_i without reading a byte.
 *
 * hmse_order_keys: key[i] = the key of range i at depth[i], for every i.
 * hmse_order_lcp:  lcp[i] as above, for every i.
 * The tables raw / raw_off / cuts / slot are those of hmse_lines_gather: corpus byte q of chunk k is raw[raw_off[slot[k]] + q - cuts[k]];
 * a range may cross any number of chunks, chunks may be 0, 1 or 2 bytes long, a deduplicated record lies at several places.
 *
 * status (u32, cleared by the call): bit 1 = tables that break a rule of the chunk map (cuts[0] != 0 included), a range with
 * start > end or end > N, a depth[i] > L_i, a rep[i] >= n, or a from[i] > min(L_i, L_rep[i]).  With bit 1 nothing is read through the
 * tables and every output element is 0.  Bit 0 is never set.  The outputs are written for every i: the caller clears nothing.
 * HMSE_EINVAL before anything is cleared or launched: a NULL status, a NULL pointer to a non-empty array, n >= 2^31, flag bits other
 * than HMSE_FIND_IGNORE_CASE.
 * No workspace, no LDS; stream-ordered, allocate nothing, never sync.  Both main kernels report in profile slot 31
 * (HMSE_STAGE_FIND_PLACE), shared with the other search kernels: reset it first.
 * Out of scope: descending order (flip a group on the caller's side), numeric, version, locale or key-field (-k) comparison, merging
 * several sorted results or several stores, sorting the store's records themselves, several short ranges packed into one wavefront.
 */
#define HMSE_ORDER_KEY_BYTES 7u   /* text bytes in a key */
#define HMSE_ORDER_R_MORE    8u   /* r of a text that goes on behind the key's bytes */

int hmse_order_keys(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                    const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* depth, uint64_t n,
                    uint32_t flags, uint64_t* key, uint32_t* status, void* stream);
int hmse_order_lcp(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                   const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* rep,
                   const uint64_t* from, uint64_t n, uint32_t flags, uint64_t* lcp, uint32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HMSE_ORDER_H */
