// scn_trace.h -- the sweep trace's arithmetic (scanner_hip.h, "Sweep trace"), stated once for the kernel that folds a collected
// spectrum into a plan's trace (scn_trace.hip) and for the host forms (scn_trace_fold_spectrum, scn_trace_merge: scn_host.hip), which
// a plain C++ compiler builds without a HIP header in sight: the frequency of a bin, its cell, the ordered key and what is a NaN.
// Integers and compares only, but for the one double addition and cast that every hit record's freq_hz is made with.
#pragma once
#include <stdint.h>

#include "scn_mask.h"

// a bin that folds into no cell: masked, NaN, below f0_hz or at or beyond the last cell (cells <= SCN_TRACE_CELLS_MAX < this)
constexpr uint32_t kTraceNoCell = 0xffffffffu;

// The ordered key of a float's bits and its inverse (the floor detector's: unsigned order = float order, -inf lowest, -0.0 below
// +0.0), and the bits that are a NaN, either sign
SCN_HOST_DEVICE uint32_t scn_trace_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
SCN_HOST_DEVICE uint32_t scn_trace_unkey(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }
SCN_HOST_DEVICE bool scn_trace_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
// an empty cell: max_db = -inf, min_db = +inf, as keys (every value that is not a NaN lies between them, ends included)
constexpr uint32_t kTraceEmptyMaxKey = 0x007fffffu;  // scn_trace_key(0xff800000)
constexpr uint32_t kTraceEmptyMinKey = 0xff800000u;  // scn_trace_key(0x7f800000)

// freq_hz of the record of (unit, i), as scn_hitlist.h completes it: start_frequency = fc - double(sample_rate / 2) (process.cpp:38,
// uint32 division), frequency = start_frequency + double(uint32(i * bin_step)) (process.cpp:55, the product wraps in uint32),
// bin_step = sample_rate / n truncated (process.cpp:39), and uint64_t(double) the way the reference's x86-64 build casts (a
// negative double becomes the two's complement of its magnitude, not 0).  |frequency| < 2^63, as for the records.
SCN_HOST_DEVICE double scn_trace_start(double fc, uint32_t sample_rate) { return fc - (double)(sample_rate / 2u); }
SCN_HOST_DEVICE uint64_t scn_trace_freq(double start_frequency, uint32_t i, uint32_t bin_step) {
  const double f = start_frequency + (double)(uint32_t)(i * bin_step);
  return f < 0.0 ? (uint64_t)(int64_t)f : (uint64_t)f;
}

// The cell of a frequency on the grid (f0_hz, cell_hz >= 1, cells): (f - f0_hz) / cell_hz in uint64 integer arithmetic, or
// kTraceNoCell below the grid or at or beyond its end.  (A distance under 2^32 -- any grid a sweep of one band draws -- divides in 32 bits.)
SCN_HOST_DEVICE uint32_t scn_trace_cell(uint64_t f, uint64_t f0_hz, uint32_t cell_hz, uint32_t cells) {
  if (f < f0_hz) return kTraceNoCell;
  const uint64_t d = f - f0_hz;
  const uint64_t c = d <= 0xffffffffull ? (uint64_t)((uint32_t)d / cell_hz) : d / cell_hz;
  return c < cells ? (uint32_t)c : kTraceNoCell;
}

// The same cells for a whole unit without a double per bin, where that is the same arithmetic.  A start frequency that is a
// non-negative integer below 2^52 makes start_frequency + double(k), k < 2^32, exact: f = base + k with base = uint64(start_frequency).
// If the unit also begins on the grid (base >= f0_hz), then with base - f0_hz = q0 * cell_hz + r0 the cell of a bin is
// q0 + (r0 + k) / cell_hz -- the division above, of a number that almost always fits 32 bits.  `exact` says whether that holds;
// where it does not (a centre with a fraction, a negative start, a unit that begins below the grid) the bins go through
// scn_trace_freq and scn_trace_cell.  tests/cpp/test_trace.cpp holds the two ways to each other.
struct ScnTraceUnit {
  uint64_t q0;
  uint32_t r0;
  bool exact;
};
SCN_HOST_DEVICE ScnTraceUnit scn_trace_unit(double start_frequency, uint64_t f0_hz, uint32_t cell_hz) {
  ScnTraceUnit u = {0, 0, false};
  if (!(start_frequency >= 0.0 && start_frequency < 4503599627370496.0)) return u;  // (2^52; a NaN fails both)
  const uint64_t base = (uint64_t)start_frequency;
  if ((double)base != start_frequency || base < f0_hz) return u;
  u.q0 = (base - f0_hz) / cell_hz;
  u.r0 = (uint32_t)((base - f0_hz) % cell_hz);
  u.exact = true;
  return u;
}
// k = uint32(i * bin_step), as scn_trace_freq forms it
SCN_HOST_DEVICE uint32_t scn_trace_cell_in_unit(const ScnTraceUnit &u, uint32_t k, uint32_t cell_hz, uint32_t cells) {
  const uint64_t s = (uint64_t)u.r0 + k;
  const uint64_t c = u.q0 + (s <= 0xffffffffull ? (uint64_t)((uint32_t)s / cell_hz) : s / cell_hz);
  return c < cells ? (uint32_t)c : kTraceNoCell;
}
