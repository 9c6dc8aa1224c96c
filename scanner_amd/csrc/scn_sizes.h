// scn_sizes.h -- which sizes each kernel family takes, the shape of the fused kernels' per-thread twiddle table, and the path a
// plan of a size runs on.  Plain C++, no HIP header: the launchers (through scn_kernels.h) and the host arithmetic (scn_host.hip,
// built by g++ in tests/cpp/test_plan_resolve.cpp) read the same rules.
#pragma once
#include <stdint.h>

#include "../../include/scanner_hip.h"
#include "scn_mixed_plans.h"

inline bool scn_fft_size_supported(uint32_t n) { return n >= 16 && n <= 16384 && (n & (n - 1u)) == 0u; }  // scn_kernels.hip
inline bool scn_big_size_supported(uint32_t n) { return n == 65536u || n == 32768u; }                     // scn_big.hip
inline bool scn_bluestein_size_supported(uint32_t n) { return n >= 16u && n < 65536u && (n & (n - 1u)) != 0u; }  // scn_generic.hip: transform length <= 131072
inline bool scn_avg_size_supported(uint32_t n) { return n == 1024 || n == 2048 || n == 4096 || n == 8192; }      // scn_average.hip
// layout of ScnFftArgs::tw1_table for size n: `rows` rows of `threads` entries, row p-1 = W_n^(t p): 15 rows of n/16 for the
// 16 x 16 x M kernels, 31 rows of 512 for the 32 x 16 x 32 form of 16384 points
inline void scn_tw1_layout(uint32_t n, uint32_t *rows, uint32_t *threads) {
  *rows = n == 16384 ? 31u : 15u;
  *threads = n == 16384 ? 512u : n / 16u;
}
// the plan of a mixed size n (scn_mixed.hip), or false: its smallest radix R1 (the tw1 table has R1 - 1 rows) and the pass-1 thread count T1 (its row length)
#define SCN_MIXED_LOOKUP(N, R1, R2, R3, PAD1, PAD2, UNIT) \
  if (n == N) {                                            \
    if (rows) *rows = R1 - 1;                              \
    if (threads) *threads = R2 * R3;                       \
    return true;                                           \
  }
#define SCN_MIXED_BIG_LOOKUP(N, R1, R2, R3, PAD1, UNIT) SCN_MIXED_LOOKUP(N, R1, R2, R3, PAD1, 0, UNIT)
inline bool scn_mixed_layout(uint32_t n, uint32_t *rows, uint32_t *threads) {
  SCN_MIXED_PLANS(SCN_MIXED_LOOKUP)
  SCN_MIXED_BIG_PLANS(SCN_MIXED_BIG_LOOKUP)
  return false;
}
#undef SCN_MIXED_LOOKUP
#undef SCN_MIXED_BIG_LOOKUP
inline bool scn_mixed_size_supported(uint32_t n) { return scn_mixed_layout(n, nullptr, nullptr); }

// How a plan computes its spectrum: decided once, by path_of, and read by everything that depends on it
enum class Path { TimeDomain, FusedPow2, FusedMixed, FourStep, Bluestein, Unsupported };
inline Path path_of(uint32_t mode, uint32_t n) {
  if (mode == SCN_MODE_TIME_DOMAIN) return Path::TimeDomain;
  if (scn_fft_size_supported(n)) return Path::FusedPow2;        // the powers of two 16 ... 16384
  if (scn_mixed_size_supported(n)) return Path::FusedMixed;     // the sizes 2^a 3^b 5^c of scn_mixed_plans.h
  if (scn_big_size_supported(n)) return Path::FourStep;         // 32768, 65536
  if (scn_bluestein_size_supported(n)) return Path::Bluestein;  // every other size from 16 to 65535
  return Path::Unsupported;
}
