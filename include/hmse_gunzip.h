/* hmse_gunzip.h — the C ABI of the gzip import (hmse_amd/csrc/gunzip.hip; bound by hmse_amd/_lib.py::GUNZIP_SIGNATURES).  An addition to
 * include/hmse.h, which it includes: same library, same conventions (status codes, stream-ordered calls, 256-byte aligned workspaces),
 * same ABI version. */
#ifndef HMSE_GUNZIP_H
#define HMSE_GUNZIP_H
#include "hmse.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * Import of multi-member gzip / BGZF (hmse_amd/gunzip.py): where the members are.  Decoding is hmse_l1_inflate's (kind FULL, no base),
 * the CRC-32 hmse_crc32's.  A gzip member does not say how long it is; its end is known once its DEFLATE stream has been walked.  Both
 * calls are parallel over positions / candidates; the caller follows end[] from offset 0 to pick the members among the candidates.
 *
 * hmse_gzip_candidates: cand_off (DEVICE u64[cap]) receives, ascending, every position p with p + 20 <= n (10 header bytes, the 2-byte
 *   empty fixed block, 8 trailer bytes), data[p .. p + 3) == 1f 8b 08 and (data[p + 3] & 0xE0) == 0 (the reserved FLG bits).  count
 *   (DEVICE u64[1]) = their number, also when it is above cap: then status (DEVICE u32[1]) bit0 is set, the first cap are written and
 *   nothing behind cand_off[cap).  Entries behind the count are left as they were.  Reads data[0, n) only.
 * hmse_gzip_measure: for every candidate k (cand_off DEVICE u64[n_cand], any order, any values), one wavefront:
 *   stream_off[k] = the first byte behind the header (RFC 1952: FEXTRA, FNAME, FCOMMENT, FHCRC; MTIME, XFL, OS, FTEXT ignored),
 *   end[k] = one past the 8-byte trailer, raw_len[k] = the decoded length, crc[k] = the trailer's CRC-32 (all DEVICE, [n_cand]; u64, u64,
 *   u64, u32), flags[k] (DEVICE u32) = HMSE_GZIP_VALID | HMSE_GZIP_FAST, or for an invalid candidate reason << HMSE_GZIP_WHY_SHIFT with
 *   end[k] = cand_off[k], raw_len[k] = crc[k] = 0.  Reasons: HEADER = no magic / a reserved FLG bit / the FHCRC is not the low 16 bits of
 *   the CRC-32 of the header in front of it; BOUNDS = the header, the stream or the trailer runs past n; STREAM = the DEFLATE stream breaks
 *   a rule that hmse_l1_inflate (and zlib) refuse: reserved block type, over-subscribed or incomplete code set, no end-of-block code,
 *   length / distance symbol out of range, distance beyond the start, stored LEN / NLEN; LENGTH = the walked length is not ISIZE, or the
 *   raw or the compressed length is 2^32 or more.
 *   HMSE_GZIP_FAST (BGZF): FEXTRA holds a subfield 'B' 'C' of SLEN 2 whose BSIZE + 1 >= header + 2 + 8, the block lies inside data and its
 *   ISIZE <= 65536: end = p + BSIZE + 1, raw_len = ISIZE, crc from the block's trailer, NOTHING IS DECODED — a BSIZE that disagrees with
 *   the stream shows when the member is decoded.  A BC subfield that fails these conditions is ignored (the ordinary path).
 *   The ordinary path walks the stream for its length only (no stores, no window).  Every loop is bounded by 8 * (n - stream_off) + 64
 *   steps: a wavefront reaches its exit whatever the bytes are.  status is cleared; no bit is defined.
 * Workspace (256-byte aligned, contents don't matter): hmse_gzip_workspace_bytes(n) serves both calls (the per-tile counts of the
 *   candidate passes; the pull counter of the persistent wavefronts).  HMSE_ENOSPC if it is smaller.
 * HMSE_EINVAL before anything is cleared or launched: status / count NULL, a NULL pointer to a non-empty array, n above 2^40, n_cand
 * above 2^31 - 1.  Stream-ordered, allocate nothing, never sync.
 * Out of scope: one member split over several wavefronts, zlib / raw / zip containers, members of 4 GiB or more, a .gzi index.
 */
#define HMSE_GZIP_VALID 1u
#define HMSE_GZIP_FAST 2u
#define HMSE_GZIP_WHY_SHIFT 2
#define HMSE_GZIP_WHY_HEADER 1u
#define HMSE_GZIP_WHY_STREAM 2u
#define HMSE_GZIP_WHY_LENGTH 3u
#define HMSE_GZIP_WHY_BOUNDS 4u

size_t hmse_gzip_workspace_bytes(uint64_t n);
int hmse_gzip_candidates(const uint8_t* data, uint64_t n, uint64_t* cand_off, uint64_t cap, uint64_t* count, uint32_t* status, void* ws,
                         size_t ws_bytes, void* stream);
int hmse_gzip_measure(const uint8_t* data, uint64_t n, const uint64_t* cand_off, uint64_t n_cand, uint64_t* stream_off, uint64_t* end,
                      uint64_t* raw_len, uint32_t* crc, uint32_t* flags, uint32_t* status, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HMSE_GUNZIP_H */
