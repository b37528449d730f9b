// regexa.hip — regular-expression search WITH ASSERTIONS (^ $ \A \Z \b \B) over the decoded records of a store (hmse_amd/regex.py
// Regex(assertions=True) compiles the automaton; hmse_amd/find.py StoreFinder picks these entry points by Regex.asserting;
// include/hmse_regexa.h hmse_regexa_*; a library of its own, libhmse_regexa.so, beside libhmse_hip.so).  The ASSERTING form of
// regex_core.h, which holds the kernels (regexa_validate_kernel, regexa_scan_kernel, regexa_seams_kernel) and the bodies of the entry
// points, and says where this form leaves regex.hip's.
#include "common.h"
#include "../../include/hmse_regexa.h"
#include "chunkmap.h"

constexpr bool RX_A = true;
using RxX = struct RxaDev;
using RxHeader = hmse_regexa;
#define RX_KERNEL(name) regexa_##name
#include "regex_core.h"

// tests/test_gpu_regexa.py places its tile, strip and grid edges by the scan's geometry and reads it from THIS file, as regex_core.h defines it:
//   constexpr int RX_NT = 256;   constexpr int RX_STRIP = 32;   constexpr uint32_t RX_MAX_BLOCKS = 512;
static_assert(RX_NT == 256 && RX_STRIP == 32 && RX_MAX_BLOCKS == 512, "the line above no longer says what regex_core.h defines");

extern "C" int hmse_regexa_scan(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint32_t* mult,
                                const hmse_regexa* rx, uint64_t* hits, uint64_t hits_cap, uint64_t* n_hits, uint64_t* count,
                                uint32_t* status, void* stream_) {
  return rx_scan(raw, raw_bytes, raw_off, n_rec, mult, rx, hits, hits_cap, n_hits, count, status, stream_);
}

extern "C" int hmse_regexa_seams(const uint8_t* raw, uint64_t raw_bytes, const uint64_t* raw_off, uint64_t n_rec, const uint64_t* cuts,
                                 const uint64_t* slot, uint64_t n_chunks, const hmse_regexa* rx, uint64_t* hits, uint64_t hits_cap,
                                 uint64_t* n_hits, uint64_t* count, uint32_t* status, void* stream_) {
  return rx_seams(raw, raw_bytes, raw_off, n_rec, cuts, slot, n_chunks, rx, hits, hits_cap, n_hits, count, status, stream_);
}
