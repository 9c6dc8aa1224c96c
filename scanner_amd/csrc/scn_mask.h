// scn_mask.h -- the kernel-side arithmetic the host restates, K5's mask, the baseline row of a unit and the detectors' grid: shared by the kernels (through
// scn_kernels.h) and by the plan arithmetic of scn_host.hip, which a plain C++ compiler builds without a HIP header in sight.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__  // (spelled out: what __forceinline__ stands for, since a unit without the HIP runtime header includes this too)
#define SCN_HOST_DEVICE __host__ __device__ inline __attribute__((always_inline))
#else
#define SCN_HOST_DEVICE inline
#endif

// K5's mask (process.cpp:46-52, uint32 arithmetic): is bin j of an n-point spectrum, fftshift index i = (j + n/2) % n, held
// against the threshold?  `a` carries dc_ignore, i_lo and i_hi (the argument structs of every path; the host sizes hit_region by it)
template <class A>
SCN_HOST_DEVICE bool scn_bin_evaluated(uint32_t j, uint32_t i, uint32_t n, const A &a) {
  return !(j < a.dc_ignore || (n - j) < a.dc_ignore) && !(i < a.i_lo || i > a.i_hi);
}

// The baseline row that unit u of a submit reads, and an update writes (scanner_hip.h, "Baseline detector"): (first + u) % rows.
// The caller keeps first < rows and first + u below 2^32; a row per unit, the usual table, takes no division.
SCN_HOST_DEVICE uint32_t scn_baseline_row(uint32_t first, uint32_t u, uint32_t rows) {
  const uint32_t s = first + u;
  return s < rows ? s : s % rows;
}

// The hit history (scanner_hip.h, "Hit history"), one 32-bit word per bin: bit 0 the row's most recent visit, bit k the visit k
// visits before it.  A fold shifts the visit in at the bottom (the oldest falls off the top); a record is confirmed when at least m
// of the `window` most recent visits were hits, 1 <= m <= window <= 32 (the caller's check: check_history_window, scn_host.h).
SCN_HOST_DEVICE uint32_t scn_history_fold(uint32_t word, uint32_t hit) { return (word << 1) | (hit & 1u); }
SCN_HOST_DEVICE uint32_t scn_history_mask(uint32_t window) { return window >= 32u ? 0xffffffffu : (1u << window) - 1u; }
SCN_HOST_DEVICE bool scn_history_confirms(uint32_t word, uint32_t mask, uint32_t m) { return (uint32_t)__builtin_popcount(word & mask) >= m; }

// The grid of a launch of persistent teams (scn_detect.h): ceil(n_units / teams) workgroups of `teams` teams each, capped at what is
// resident at once, per_cu workgroups on each of num_cus CUs (256 CUs where the count is unknown).
SCN_HOST_DEVICE uint32_t scn_team_grid(uint32_t n_units, uint32_t teams, int num_cus, int per_cu) {
  const uint32_t resident = (uint32_t)(num_cus > 0 ? num_cus : 256) * (uint32_t)per_cu;
  const uint32_t blocks = n_units / teams + (n_units % teams != 0u ? 1u : 0u);  // (n_units + teams - 1 wraps from 2^32 - teams + 1 units up)
  return blocks < resident ? blocks : resident;
}
