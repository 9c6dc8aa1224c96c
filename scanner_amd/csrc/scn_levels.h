// scn_levels.h -- the level histogram's arithmetic (scanner_hip.h, "Level histogram"), stated once for the kernels that fold a
// collected spectrum into a plan's histogram and summarise it (scn_levels.hip) and for the host forms (scn_levels_fold_spectrum,
// scn_levels_merge, scn_levels_summary: scn_host.hip), which a plain C++ compiler builds without a HIP header in sight: the level of
// a value on a table of edges, and the rank a permille asks for.  The cell of a bin is scn_trace.h's, unchanged.  Integers and
// compares only.
#pragma once
#include <stdint.h>

#include "scn_trace.h"

// The edges as a search reads them: kLevelsKeys ordered keys (scn_trace_key of the edges' bits), the n_edges <= SCN_LEVELS_EDGES_MAX
// of the table first, in increasing order, and kLevelsPadKey behind them -- above the key of every value that is not a NaN (+inf is
// 0xff800000), so a pad is never counted.
constexpr uint32_t kLevelsKeys = 256u;
constexpr uint32_t kLevelsPadKey = 0xffffffffu;

// The first step of the search: the largest power of two <= n_edges (n_edges >= 1).  The steps top, top / 2, ... 1 sum to
// 2 top - 1 >= n_edges, and reach index 2 top - 2 <= kLevelsKeys - 2 at the most: at most 8 steps.
SCN_HOST_DEVICE uint32_t scn_levels_top(uint32_t n_edges) { return 1u << (31 - __builtin_clz(n_edges)); }

// level(v): the number of edges e with key(e) <= key(v), 0 ... n_edges -- level l holds edges[l - 1] <= v < edges[l], a value equal
// to an edge belongs to the level above it.  `keys`: the kLevelsKeys padded keys, `top`: scn_levels_top(n_edges), `key`: the key of
// a value that is not a NaN.  After the steps down to s, pos is the largest multiple of s with keys[pos - 1] <= key.
SCN_HOST_DEVICE uint32_t scn_levels_level(const uint32_t *keys, uint32_t top, uint32_t key) {
  uint32_t pos = 0;
  for (uint32_t step = top; step != 0u; step >>= 1)
    if (keys[pos + step - 1u] <= key) pos += step;
  return pos;
}

// The rank a summary reads of a cell of total >= 1 counts: r = floor(permille * (total - 1) / 1000), permille 0 ... 1000, formed
// without an overflow -- total - 1 = 1000 a + b, 0 <= b < 1000, r = permille a + (permille b) / 1000 (permille a <= total - 1).
// rank_level is the smallest level whose cumulative count exceeds r.
SCN_HOST_DEVICE uint64_t scn_levels_rank(uint64_t total, uint32_t permille) {
  const uint64_t a = (total - 1u) / 1000u, b = (total - 1u) % 1000u;
  return (uint64_t)permille * a + ((uint64_t)permille * b) / 1000u;
}
// an empty cell's rank_level
constexpr uint32_t kLevelsNoRank = 0xffffffffu;
