// scn_emitters.h -- the trace emitters' arithmetic (scanner_hip.h, "Trace emitters"), stated once for the kernels that segment a line
// of a plan's trace (scn_emitters.hip), for the host form (scn_trace_emitters: scn_host.hip) and for tests/cpp/test_emitters.cpp,
// which a plain C++ compiler builds without a HIP header in sight: the value of a line, what is on, where an emitter starts, the
// peak's key and the hertz fields.  Integers and compares only, but for the one float32 subtraction of the spread.
#pragma once
#include <stdint.h>

#include "scn_trace.h"

constexpr uint32_t kEmitLineMax = 0, kEmitLineMin = 1, kEmitLineSpread = 2;  // SCN_TRACE_LINE_*

SCN_HOST_DEVICE float scn_emit_float(uint32_t bits) {
  float f;
  __builtin_memcpy(&f, &bits, sizeof(f));
  return f;
}
SCN_HOST_DEVICE uint32_t scn_emit_bits(float f) {
  uint32_t bits;
  __builtin_memcpy(&bits, &f, sizeof(bits));
  return bits;
}

// v of a cell, as bits: max_db, min_db, or max_db - min_db in ONE float32 subtraction, round to nearest, a denormal result kept
// (inf - inf: a NaN of either sign, which is never on)
SCN_HOST_DEVICE uint32_t scn_emit_value(uint32_t line, uint32_t max_bits, uint32_t min_bits) {
  if (line == kEmitLineMax) return max_bits;
  if (line == kEmitLineMin) return min_bits;
  return scn_emit_bits(scn_emit_float(max_bits) - scn_emit_float(min_bits));
}
// peak_other_db: the cell's other extreme
SCN_HOST_DEVICE uint32_t scn_emit_other(uint32_t line, uint32_t max_bits, uint32_t min_bits) { return line == kEmitLineMax ? min_bits : max_bits; }

// v > threshold as float32 compares them -- neither a NaN, -0.0 equal to +0.0 --, decided on the ordered keys: no float mode has a say
SCN_HOST_DEVICE uint32_t scn_emit_compare_key(uint32_t bits) { return scn_trace_key((bits & 0x7fffffffu) == 0u ? 0u : bits); }
SCN_HOST_DEVICE bool scn_emit_on(uint64_t count, uint32_t v_bits, uint32_t threshold_bits) {
  return count != 0u && !scn_trace_is_nan(v_bits) && scn_emit_compare_key(v_bits) > scn_emit_compare_key(threshold_bits);
}

// An on cell c starts an emitter when the window has no on cell before it, or the last one (prev < c) lies more than max_gap + 1 back
SCN_HOST_DEVICE bool scn_emit_starts(bool has_prev, uint32_t prev, uint32_t c, uint32_t max_gap) { return !has_prev || c - prev - 1u > max_gap; }

// The peak's key: unsigned maximum = the largest v in the trace's key order (-0.0 below +0.0), equal v: the LOWEST cell.  Never 0
// for a value that is not a NaN (the lowest value key is -inf's, 0x007fffff), so 0 is the key of "no cell yet".
SCN_HOST_DEVICE uint64_t scn_emit_peak_key(uint32_t v_bits, uint32_t cell) { return ((uint64_t)scn_trace_key(v_bits) << 32) | (uint64_t)(~cell); }
SCN_HOST_DEVICE uint32_t scn_emit_peak_cell(uint64_t key) { return ~(uint32_t)key; }
SCN_HOST_DEVICE uint32_t scn_emit_peak_bits(uint64_t key) { return scn_trace_unkey((uint32_t)(key >> 32)); }

// f0_hz + cell * cell_hz in uint64 arithmetic (cell: up to `cells`, for the exclusive upper edge)
SCN_HOST_DEVICE uint64_t scn_emit_hz(uint64_t f0_hz, uint32_t cell_hz, uint64_t cell) { return f0_hz + cell * (uint64_t)cell_hz; }
