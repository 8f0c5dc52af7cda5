// The forms an engine keeps its tips in, and the one rule that derives them.  Plain C++ (the
// __host__ __device__ marks appear under hipcc only): tips_prepare_kernel and engine creation's
// host path (mi_phylo_engine.cpp) both read this, and tests/cpp/tip_forms_check.cpp checks it
// without a device.
//
// A compact state c is 0..states-1, or `states` for a gap (any caller value outside the range).
// What a 4-state engine derives from it (SitePattern::GetPartials, site_pattern.cpp:117-131):
//   mask     bit s = compatible with state s: 1 << c, 0xF for a gap (the matrix-core kernels)
//   code     byte offset of the state's entry in the look-up walk's tip tables: 16 c, 64 for a gap
//   partial  row of four doubles: 1 where the mask has its bit, else 0
// Caller-supplied partials go the other way: a row whose entries are all exactly 0 or 1 has a
// mask, a mask that is one of the five above has a code.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MI_TIP_HD __host__ __device__
#else
#define MI_TIP_HD
#endif

namespace miphylo {

constexpr int kTipDna = 4;         // states of the forms below (kStates)
constexpr uint8_t kTipNoForm = 0xFF;  // "this row has no mask" / "this mask has no code"

MI_TIP_HD inline int8_t tip_state(int32_t v, int states) { return (int8_t)((v >= 0 && v < states) ? v : states); }
MI_TIP_HD inline uint8_t tip_mask(int c) { return c >= kTipDna ? 0xF : (uint8_t)(1u << c); }
MI_TIP_HD inline uint8_t tip_code(int c) { return c >= kTipDna ? 64 : (uint8_t)(16 * c); }
MI_TIP_HD inline double tip_partial(int c, int k) { return (tip_mask(c) >> k) & 1 ? 1.0 : 0.0; }

// the mask of a caller's 4-state partial row, kTipNoForm unless every entry is exactly 0 or 1
inline uint8_t tip_mask_of_partials(const double* row) {
  uint8_t m = 0;
  for (int x = 0; x < kTipDna; x++) {
    if (row[x] == 1.0) m |= (uint8_t)(1u << x);
    else if (row[x] != 0.0) return kTipNoForm;
  }
  return m;
}
// the code of a mask, kTipNoForm unless it is the mask of a compact state
inline uint8_t tip_code_of_mask(uint8_t m) {
  for (int c = 0; c <= kTipDna; c++)
    if (m == tip_mask(c)) return tip_code(c);
  return kTipNoForm;
}
// the compact state of a caller's partial row of `states` entries: the state of a one-hot row,
// `states` for all ones, -1 for anything else (the 20-state kernels read compact states only)
inline int tip_state_of_partials(const double* row, int states) {
  int ones = 0, last = 0;
  for (int x = 0; x < states; x++) {
    if (row[x] == 1.0) { ones++; last = x; }
    else if (row[x] != 0.0) return -1;
  }
  return ones == 1 ? last : ones == states ? states : -1;
}

}  // namespace miphylo
