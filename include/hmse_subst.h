/* hmse_subst.h — the C ABI of SUBSTITUTE: the corpus with a list of ranges replaced, written on the device
 * (hmse_amd/csrc/subst.hip, built into hmse_amd/csrc/libhmse_subst.so; bound by hmse_amd/_lib.py::SUBST_SIGNATURES; the merging of the
 * ranges is hmse_amd/find.py StoreFinder.substitute / redact).  An addition to include/hmse.h, which it includes: same conventions (status
 * codes, stream-ordered calls), same ABI version, the tables of hmse_lines_gather. */
#ifndef HMSE_SUBST_H
#define HMSE_SUBST_H
#include "hmse.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * Definitions (tests/subst_ref.py restates them in plain Python).  C is the N = cuts[n_chunks] bytes read.read_store(store) returns.
 *
 * EDITS.  n edits (start[i], end[i], sel[i]), given in order: end[i-1] <= start[i] <= end[i] <= N, with end[-1] = 0.  Ranges do not
 * overlap; they may touch; they may be empty (an insertion); several insertions at one position keep the order they are given in.
 *
 * REPLACEMENTS.  Packed: replacement r is rep[rep_off[r] : rep_off[r+1]), r < n_rep, rep_off[0] = 0, rep_off[n_rep] <= rep_bytes, and
 * sel[i] < n_rep.
 *   HMSE_SUBST_LITERAL (flags = 0): R_i is replacement sel[i]; it may be empty (a deletion).
 *   HMSE_SUBST_FILL    (flags = 1): R_i is the ONE byte of replacement sel[i] repeated end[i] - start[i] times; every replacement then
 *                                   has length exactly 1, and lengths and offsets are preserved (|O| = N).
 *
 * OUTPUT.  O = C[0:start[0]) R_0 C[end[0]:start[1]) R_1 ... R_{n-1} C[end[n-1]:N).
 *   out_off[i] = start[i] + sum_{j<i} (|R_j| - (end[j] - start[j]))      where R_i begins in O
 *   out_off[n] = |O|
 * The caller supplies out_off, u64[n + 1] (with n = 0: the one entry N); the call proves it before anything is written.
 *
 * PER POSITION (what the kernel computes).  For an output position p let i be the LAST edit with out_off[i] <= p.  If i exists and
 * p < out_off[i] + |R_i| the byte is R_i[p - out_off[i]].  Otherwise it is C[p - D] with D = out_off[i+1] - start[i+1], or
 * out_off[n] - N behind the last edit, or 0 when no edit exists.  out_off never descends; among equal values the last is the right one
 * (the earlier ones wrote nothing).
 *
 * The tables raw / raw_off / cuts / slot are those of hmse_lines_gather: corpus byte q of chunk k is raw[raw_off[slot[k]] + q - cuts[k]];
 * chunks may be 0, 1 or 2 bytes long.
 *
 * status (u32, cleared by the call):
 *   bit 1 = tables that break a rule of the chunk map (cuts[0] != 0 included); an edit that breaks the edit rule; a sel[i] >= n_rep; a
 *           rep_off that descends, does not start at 0 or ends past rep_bytes; in fill mode a replacement whose length is not 1; an
 *           out_off[i] that is not the definition's.
 *   bit 0 = out_off[n] > out_cap.
 * With any bit set NOT ONE BYTE of out is written.  Without, exactly out[0 : out_off[n]) is written, every byte once.
 * HMSE_EINVAL before anything is cleared or launched: a NULL status, a NULL pointer to a non-empty array (out_off always has an entry),
 * n >= 2^33, flag bits other than HMSE_SUBST_FILL, n_rep == 0 with n > 0, and sizes whose grids would pass 2^31 - 1 workgroups.
 * No workspace; stream-ordered, allocates nothing, never syncs.  The writing kernel reports in profile slot 31 (HMSE_STAGE_FIND_PLACE),
 * shared with the other search kernels: reset it first.
 * Out of scope: captures and back-references, `&` (the whole match inside a replacement), case-preserving replacement, editing the
 * store's records in place without re-ingest, several stores, fill patterns longer than one byte.
 */
#define HMSE_SUBST_LITERAL 0u
#define HMSE_SUBST_FILL    1u

int hmse_subst_apply(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                     const uint64_t* slot, uint64_t n_chunks, const uint64_t* start, const uint64_t* end, const uint64_t* sel, uint64_t n,
                     const uint8_t* rep, uint64_t rep_bytes, const uint64_t* rep_off, uint64_t n_rep, uint32_t flags,
                     const uint64_t* out_off, uint8_t* out, uint64_t out_cap, uint32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HMSE_SUBST_H */
