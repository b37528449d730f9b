/* hmse_regexa.h — the C ABI of the regex search WITH ASSERTIONS: line anchors and word boundaries ^ $ \A \Z \b \B
 * (hmse_amd/csrc/regexa.hip, built into hmse_amd/csrc/libhmse_regexa.so; bound by hmse_amd/_lib.py::REGEXA_SIGNATURES).  An addition to
 * include/hmse.h, which it includes: same conventions (status codes, stream-ordered calls), same ABI version, the hit word, the tables
 * and the caps of hmse_regex_scan / hmse_regex_seams. */
#ifndef HMSE_REGEXA_H
#define HMSE_REGEXA_H
#include "hmse.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * Definitions.  C is the N bytes of the corpus.  Every byte has a KIND: NL = 1 (0x0A), WORD = 2 ([0-9A-Za-z_]), OTHER = 3 (the rest);
 * EDGE = 0 stands for "no byte": in front of C[0] and behind C[N - 1].  Between the previous byte a and the next byte b
 *   ^ holds iff kind(a) is EDGE or NL      $ holds iff kind(b) is EDGE or NL      \A iff kind(a) is EDGE      \Z iff kind(b) is EDGE
 *   \b holds iff exactly one of a, b is a WORD byte (the edge is none)            \B iff \b does not hold
 * (re.MULTILINE on bytes).  Start o is an OCCURRENCE iff some l with 1 <= l <= min(reach, N - o) has C[o .. o + l) matching the regex
 * with every assertion evaluated against the real bytes C[o - 1] and C[o + l] (or the edge); its LENGTH is the largest such l.  Empty
 * matches are never reported, every start counts, a match is at most HMSE_REGEX_MAX_LEN bytes.
 *
 * The compiled form (`hmse_regexa`, deterministic for a given pattern and flags; hmse_amd/regex.py Regex(assertions=True)):
 *   n_classes includes one class no byte maps to, EDGE = n_classes - 1: the look-ahead beyond N
 *   classmap = u8[256]: the class of every byte value, < n_classes - 1; a class holds bytes of ONE kind
 *   start[4] = the start state by the kind of the byte in front of the start (start[0]: o == 0), each in 1 .. n_states - 1
 *   table    = u16[n_states * n_classes]: table[s * n_classes + c] = the next state, OR-ed with HMSE_REGEX_ACCEPT iff A MATCH MAY END
 *              JUST BEFORE THIS BYTE: state s accepts when the next byte has the kind of class c.  Row 0 (the dead state) is all zero,
 *              flags included; the next state in the EDGE column is always 0
 *   reach    = 1..256: no match is longer
 *   n_states * n_classes <= HMSE_REGEX_MAX_TABLE, n_states <= 32767
 * The walk from start o: s = start[kind(C[o - 1])]; for i = 0, 1, ...: e = table[s * n_classes + class of C[o + i] (EDGE at N)]; if e has
 * the flag and i >= 1 then best = i; stop after the read at i = reach (look-ahead only) or when the next state e & 0x7FFF is 0.
 * The header is a HOST struct, read during the call only.  HMSE_EINVAL before anything is cleared or launched: what hmse_regex_scan
 * refuses (struct_size, n_states outside 2..32767, n_classes above 256, a table above HMSE_REGEX_MAX_TABLE, reach outside 1..256, NULL
 * arrays, NULL n_hits / count / status, a NULL pointer to a non-empty array, raw_bytes >= 2^56, n_chunks > 2^40) and n_classes < 2 or a
 * start[i] outside 1 .. n_states - 1.
 *
 * Partition by START.  Start p of record r is a SCAN start iff p > raw_off[r] and raw_off[r+1] - p > reach: the byte in front, the walk
 * and its look-ahead byte lie in the record, so the answer holds for every chunk that maps to r (hmse_regexa_scan, laid out by
 * hmse_find_place).  Start o of a non-empty chunk k is a SEAM start iff o == cuts[k] or cuts[k+1] - o <= reach: walked through the chunk
 * map over any number of tiny or empty chunks, C[o - 1] being the last byte of the nearest non-empty chunk in front (hmse_regexa_seams).
 * Scan starts placed plus seam starts of all chunks are every occurrence exactly once.
 *
 * Both calls take the argument lists of hmse_regex_scan / hmse_regex_seams and report the same way: hits[i] = position << 8 |
 * (length - 1) in any order, n_hits, count (scan: the sum of mult[record], NULL: 1 each; seams: n_hits), status bit0 = the list ran out
 * (n_hits and count are complete, the first hits_cap words are written), bit1 = tables that break a rule of the chunk map, bit2 = a
 * bad automaton: a table entry whose low 15 bits are >= n_states, a non-zero dead row, a byte mapped to a class >= n_classes - 1, a class
 * that mixes kinds, a non-zero next state in the EDGE column.  With bit1 or bit2 nothing is read through the tables or the automaton
 * and nothing is reported.  hits NULL or hits_cap 0: count only.  No workspace; stream-ordered, allocate nothing, never sync.
 * Profile slots: hmse_regexa_scan reports in 30, hmse_regexa_seams in 31, as hmse_regex_* do.
 * Out of scope: captures, lazy forms, look-around, Unicode word classes, multi-byte line terminators and CR handling, matches over 256
 * bytes, several regexes in one automaton.
 */
#define HMSE_REGEXA_EDGE  0u
#define HMSE_REGEXA_NL    1u
#define HMSE_REGEXA_WORD  2u
#define HMSE_REGEXA_OTHER 3u

typedef struct hmse_regexa {
  uint32_t struct_size;      /* sizeof(hmse_regexa) */
  uint32_t n_states;
  uint32_t n_classes;        /* EDGE included */
  uint32_t reach;
  uint32_t start[4];         /* by the kind of the byte in front */
  const uint16_t* table;     /* DEVICE u16[n_states * n_classes] */
  const uint8_t* classmap;   /* DEVICE u8[256] */
} hmse_regexa;

int hmse_regexa_scan(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint32_t* mult,
                     const hmse_regexa* rx, uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits, uint64_t* count, uint32_t* status,
                     void* stream);
int hmse_regexa_seams(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                      const uint64_t* slot, uint64_t n_chunks, const hmse_regexa* rx, uint64_t* hits, uint64_t hits_cap,
                      uint64_t* n_hits, uint64_t* count, uint32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HMSE_REGEXA_H */
