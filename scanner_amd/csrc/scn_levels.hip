// scn_levels.hip -- the level histogram (definition: scanner_hip.h, "Level histogram"): the kernel that folds the spectrum of a
// collected submit into the plan's histogram (scn_plan_update_levels) -- per cell of a frequency grid and per level of a table of
// edges, how many dB values fell into it -- and the kernel that reduces cells of it to total, above and rank_level
// (scn_plan_levels_summary).  Integers and compares only (a float is read as its bits, ordered by the floor detector's key; the
// cell of a bin is the trace's, scn_trace.h; the level and the rank are scn_levels.h's), and an integer sum commutes: the histogram
// is the same bits whatever the order the units, waves and atomics arrive in.
//
// Fold.  The rows are streamed as scn_trace.hip streams them: one TEAM per unit and trip (the team model of scn_detect.h: a wave for
// n <= 512, a workgroup of 256 up to 4096 points, of 1024 above; persistent, walking units with the grid's stride), through a
// descriptor of exactly the unit's row, 16 bytes per lane where n % 4 == 0 and the row starts 16-byte aligned, 4 bytes otherwise, U
// loads of a lane in flight (U = 1, 2, 4), and the cell from integers alone where scn_trace_unit says that is the same arithmetic.
// What the trace does with a run of equal cells does not carry over: the bins of one run scatter over the levels.  Instead:
//   edges  the workgroup stages the table's keys into LDS once (kLevelsKeys words, padded); a bin's level is a binary search of at
//          most 8 steps there (scn_levels_level), made by every lane whether its bin folds or not: the reads stay converged.
//   tile   each team owns TILE 32-bit counters in LDS (the workgroup's tile, divided among its teams): `span` consecutive cells of
//          n_levels counters each, from c0, the cell of the unit's first evaluated bin (fftshift index i_lo; cell 0 where that bin
//          has none), as far as the cell of its last (i_hi), the grid's end or as the tile reaches, TILE / n_levels cells; no
//          cell at all where neither end of the unit has one (a unit off the grid: its flush scans nothing).
//   bin    a bin whose cell lies in [c0, c0 + span) does one no-return LDS atomicAdd; any other -- cells narrower than the tile
//          covers, a negative start frequency that wraps in the middle of the unit, a unit that is not monotonic -- one no-return
//          64-bit global atomicAdd.  Nothing rests on c0 or span being right: they decide the route of an addition, not its place.
//   flush  after the unit team_sync; the team scans span * n_levels words, issues one no-return 64-bit global atomicAdd per word
//          that is not 0 and zeroes it; team_sync again before the team's next unit adds to it.
// A unit has at most 65536 bins: a 32-bit tile counter cannot wrap.  A tile word of a cell at or beyond `cells` is never added to
// (scn_trace_cell's promise), stays 0 and is never flushed: no global address outside the histogram is formed for an atomic.
//
// LDS: the tile (kLevelsTileWords256 / kLevelsTileWords1024 words) and the keys, 17 KiB per workgroup of 256 -- 136 KiB for the 8
// workgroups the grid puts on a CU, of 160 KiB -- and 33 KiB per workgroup of 1024, of which a CU gets 2.  Grid:
// kLevelsBlocksPerCu workgroups per CU, stated -- not an occupancy query --, so that a test can size the batch that takes every
// team through its loop twice (tests/levels_caps.py); no more workgroups than units need (scn_team_grid).
//
// Summary.  A wave per cell; lane k of round r holds level 64 r + k of the cell's contiguous row, at most 4 rounds.  An inclusive
// scan by shuffles with the rounds' carry gives every lane its cumulative count; the last is `total`, a ballot finds the first
// level whose cumulative count exceeds r (scn_levels_rank), and `above` is total minus the exclusive count at `level`.  64-bit
// integers only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scn_detect.h"
#include "scn_hitlist.h"  // scn_unit_centre
#include "scn_levels.h"

namespace {

typedef float v4f_t __attribute__((ext_vector_type(4)));

// the tile of a workgroup in 32-bit words, by workgroup size, and the workgroups per CU of the fold's grid: stated, so that
// tests/levels_caps.py can restate them
constexpr int kLevelsTileWords256 = 4096, kLevelsTileWords1024 = 8192;
constexpr int kLevelsBlocksPerCu256 = 8, kLevelsBlocksPerCu1024 = 2;
static_assert((kLevelsTileWords256 + (int)kLevelsKeys) * 4 * kLevelsBlocksPerCu256 <= 160 * 1024, "the stated workgroups of 256 fit a CU's LDS");
static_assert((kLevelsTileWords1024 + (int)kLevelsKeys) * 4 * kLevelsBlocksPerCu1024 <= 160 * 1024, "the stated workgroups of 1024 fit a CU's LDS");
static_assert(kLevelsTileWords256 / 4 >= (int)SCN_LEVELS_EDGES_MAX + 1, "a wave-team's tile holds at least one cell of the largest table");

// W consecutive floats at byte offset `off` of the row behind r, as their bits (outside the row: zeros)
template <bool VEC>
__device__ __forceinline__ void load_bits(__amdgpu_buffer_rsrc_t r, uint32_t off, uint32_t (&v)[VEC ? 4 : 1]) {
  if constexpr (VEC) {
    const v4f_t x = __builtin_bit_cast(v4f_t, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
    v[0] = __float_as_uint(x.x);
    v[1] = __float_as_uint(x.y);
    v[2] = __float_as_uint(x.z);
    v[3] = __float_as_uint(x.w);
  } else {
    v[0] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
  }
}

// what a team knows of the unit it is in: the cells of its tile
struct Tile {
  uint32_t *words;  // LDS: [span][n_levels]
  uint32_t c0, span;
};

// The lane's W bins of one load: bins j0 ... j0 + W - 1, their bits in v
template <int W>
__device__ __forceinline__ void fold_load(const ScnLevelsArgs &a, const uint32_t (&v)[W], uint32_t j0, uint32_t to_i, uint32_t bin_step, double start_frequency,
                                          const ScnTraceUnit &unit, const uint32_t *keys, uint32_t top, uint32_t n_levels, const Tile &tile) {
  const uint32_t n = a.n;
#pragma unroll
  for (int x = 0; x < W; x++) {
    const uint32_t j = j0 + (uint32_t)x, i = shift_of_bin(j, to_i, n);
    const bool folds = j < n && scn_bin_evaluated(j, i, n, a) && !scn_trace_is_nan(v[x]);
    const uint32_t level = scn_levels_level(keys, top, scn_trace_key(v[x]));  // (of a NaN or a masked bin too: not used)
    uint32_t c = kTraceNoCell;
    if (folds)  // (unit.exact is the same in every lane of a wave)
      c = unit.exact ? scn_trace_cell_in_unit(unit, i * bin_step, a.cell_hz, a.cells)
                     : scn_trace_cell(scn_trace_freq(start_frequency, i, bin_step), a.f0_hz, a.cell_hz, a.cells);
    if (c == kTraceNoCell) continue;
    const uint32_t rel = c - tile.c0;  // (a cell below c0 wraps to a number no span reaches)
    if (rel < tile.span)
      atomicAdd(tile.words + rel * n_levels + level, 1u);
    else
      atomicAdd(a.hist + ((size_t)c * n_levels + level), 1ull);
  }
}

template <int T, bool VEC, int U>
__global__ __launch_bounds__(T == 64 ? 256 : T) void scn_levels_fold_kernel(ScnLevelsArgs a) {
  typedef Team<T> G;
  constexpr int W = VEC ? 4 : 1;
  constexpr uint32_t BLOCK_TILE = T == 1024 ? (uint32_t)kLevelsTileWords1024 : (uint32_t)kLevelsTileWords256, TILE = BLOCK_TILE / G::TEAMS;
  __shared__ uint32_t s_keys[kLevelsKeys];
  __shared__ uint32_t s_tile[BLOCK_TILE];
  const uint32_t t = G::t(), team = G::team();
  const uint32_t n = a.n, to_i = n - n / 2u;
  const uint32_t bin_step = a.sample_rate / n;  // process.cpp:39 (truncating)
  const uint32_t trips = (n + (uint32_t)(W * T) - 1u) / (uint32_t)(W * T);
  const uint32_t n_levels = a.n_edges + 1u, top = scn_levels_top(a.n_edges), tile_cells = TILE / n_levels;
  for (uint32_t e = threadIdx.x; e < kLevelsKeys; e += G::BLOCK) s_keys[e] = a.edge_keys[e];
  for (uint32_t w = threadIdx.x; w < BLOCK_TILE; w += G::BLOCK) s_tile[w] = 0u;
  __syncthreads();
  Tile tile;
  tile.words = s_tile + team * TILE;
  for (uint32_t u0 = blockIdx.x * G::TEAMS + team; u0 < a.n_units; u0 += gridDim.x * G::TEAMS) {
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)u0);  // (the same in every lane of a wave)
    const __amdgpu_buffer_rsrc_t rin = spectrum_rsrc(a, u);
    const double start_frequency = scn_trace_start(scn_unit_centre(a, u), a.sample_rate);
    const ScnTraceUnit unit = scn_trace_unit(start_frequency, a.f0_hz, a.cell_hz);  // (one 64-bit division per unit instead of one per bin)
    // the tile's cells: from the first evaluated bin's as far as the last one's, or as the tile reaches (a guess that costs speed
    // where it is wrong, never a count)
    const uint32_t c_lo = scn_trace_cell(scn_trace_freq(start_frequency, a.i_lo, bin_step), a.f0_hz, a.cell_hz, a.cells);
    const uint32_t c_hi = scn_trace_cell(scn_trace_freq(start_frequency, a.i_hi, bin_step), a.f0_hz, a.cell_hz, a.cells);
    tile.c0 = c_lo == kTraceNoCell ? 0u : c_lo;
    tile.span = a.cells - tile.c0 < tile_cells ? a.cells - tile.c0 : tile_cells;  // (the grid ends inside the tile)
    if (c_hi != kTraceNoCell && c_hi >= tile.c0 && c_hi - tile.c0 < tile.span) tile.span = c_hi - tile.c0 + 1u;
    if (c_lo == kTraceNoCell && c_hi == kTraceNoCell) tile.span = 0u;  // (a unit off the grid at both ends: nothing to scan)
    for (uint32_t k0 = 0; k0 < trips; k0 += (uint32_t)U) {
      uint32_t v[U][W];
#pragma unroll
      for (int x = 0; x < U; x++)  // (a trip past the last: outside the descriptor, zeros, j >= n)
        load_bits<VEC>(rin, (t + (k0 + (uint32_t)x) * (uint32_t)T) * (uint32_t)(4 * W), v[x]);
#pragma unroll
      for (int x = 0; x < U; x++)
        if (k0 + (uint32_t)x < trips)  // (wave-uniform)
          fold_load<W>(a, v[x], (t + (k0 + (uint32_t)x) * (uint32_t)T) * (uint32_t)W, to_i, bin_step, start_frequency, unit, s_keys, top, n_levels, tile);
    }
    team_sync<T>();
    unsigned long long *const out = a.hist + (size_t)tile.c0 * n_levels;
    for (uint32_t w = t; w < tile.span * n_levels; w += (uint32_t)T) {
      const uint32_t count = tile.words[w];
      if (count != 0u) {  // (a word of a cell at or beyond a.cells is 0: out + w stays inside the histogram)
        atomicAdd(out + w, (unsigned long long)count);
        tile.words[w] = 0u;
      }
    }
    team_sync<T>();
  }
}

template <int T, bool VEC, int U>
hipError_t launch(const ScnLevelsArgs &a, int num_cus, hipStream_t stream) {
  typedef Team<T> G;
  const int per_cu = G::BLOCK == 256u ? kLevelsBlocksPerCu256 : kLevelsBlocksPerCu1024;
  hipLaunchKernelGGL((scn_levels_fold_kernel<T, VEC, U>), dim3(scn_team_grid(a.n_units, G::TEAMS, num_cus, per_cu)), dim3(G::BLOCK), 0, stream, a);
  return hipGetLastError();
}

// U: loads of a lane in flight, the smallest of 1, 2, 4 that covers the row in one trip, or 4
template <int T, bool VEC>
hipError_t launch_team(const ScnLevelsArgs &a, int num_cus, hipStream_t stream) {
  const uint32_t per_trip = (uint32_t)T * (VEC ? 4u : 1u), trips = (a.n + per_trip - 1u) / per_trip;
  if (trips <= 1u) return launch<T, VEC, 1>(a, num_cus, stream);
  if (trips <= 2u) return launch<T, VEC, 2>(a, num_cus, stream);
  return launch<T, VEC, 4>(a, num_cus, stream);
}

template <bool VEC>
hipError_t launch_size(const ScnLevelsArgs &a, int num_cus, hipStream_t stream) {
  if (a.n <= 512u) return launch_team<64, VEC>(a, num_cus, stream);
  if (a.n <= 4096u) return launch_team<256, VEC>(a, num_cus, stream);
  return launch_team<1024, VEC>(a, num_cus, stream);
}

// the inclusive scan of x over the wave's lanes
__device__ __forceinline__ unsigned long long wave_scan(unsigned long long x, uint32_t lane) {
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const unsigned long long below = __shfl_up(x, off, 64);
    if (lane >= off) x += below;
  }
  return x;
}

constexpr uint32_t kSummaryWaves = 4;  // cells per workgroup of 256
constexpr int kSummaryRounds = ((int)SCN_LEVELS_EDGES_MAX + 1 + 63) / 64;

__global__ __launch_bounds__(256) void scn_levels_summary_kernel(ScnLevelsSummaryArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = blockIdx.x * kSummaryWaves + threadIdx.x / 64u;  // the cell of the window (wave-uniform)
  if (w >= a.cells) return;
  const unsigned long long *const row = a.hist + (size_t)(a.first_cell + w) * a.n_levels;
  unsigned long long x[kSummaryRounds], cum[kSummaryRounds], carry = 0;
#pragma unroll
  for (int r = 0; r < kSummaryRounds; r++) {
    const uint32_t l = (uint32_t)r * 64u + lane;
    x[r] = 0;
    cum[r] = carry;
    if ((uint32_t)r * 64u < a.n_levels) {  // (wave-uniform)
      x[r] = l < a.n_levels ? row[l] : 0ull;
      cum[r] = carry + wave_scan(x[r], lane);
      carry = __shfl(cum[r], 63, 64);
    }
  }
  const unsigned long long total = carry;
  uint32_t rank = kLevelsNoRank;
  unsigned long long below_level = 0;  // the counts of the levels under a.level
  const unsigned long long wanted = total != 0ull ? scn_levels_rank(total, a.permille) : 0ull;
#pragma unroll
  for (int r = kSummaryRounds - 1; r >= 0; r--) {  // (downwards: the lowest round that has one wins)
    const uint32_t l = (uint32_t)r * 64u + lane;
    const unsigned long long m = __ballot(l < a.n_levels && cum[r] > wanted);
    if (m != 0ull) rank = (uint32_t)r * 64u + (uint32_t)__builtin_ctzll(m);
    const unsigned long long e = __shfl(cum[r] - x[r], (int)(a.level & 63u), 64);
    if ((a.level >> 6) == (uint32_t)r) below_level = e;
  }
  if (lane == 0u) {
    a.rank_level[w] = total != 0ull ? rank : kLevelsNoRank;
    a.above[w] = total - below_level;
    a.total[w] = total;
  }
}

}  // namespace

hipError_t scn_launch_levels_fold(const ScnLevelsArgs &a, int num_cus, hipStream_t stream) {
  if (a.n_units == 0) return hipSuccess;
  if (a.n == 0 || a.n > 65536u || a.sample_rate == 0 || a.cell_hz == 0 || a.cells == 0 || a.cells > SCN_TRACE_CELLS_MAX || a.n_edges == 0 ||
      a.n_edges > SCN_LEVELS_EDGES_MAX || (uint64_t)a.cells * (a.n_edges + 1u) > SCN_LEVELS_WORDS_MAX || !a.power_db || !a.center_freq || !a.edge_keys || !a.hist)
    return hipErrorInvalidValue;
  const bool vec = a.n % 4u == 0 && ((uintptr_t)a.power_db & 15u) == 0;
  return vec ? launch_size<true>(a, num_cus, stream) : launch_size<false>(a, num_cus, stream);
}

hipError_t scn_launch_levels_summary(const ScnLevelsSummaryArgs &a, hipStream_t stream) {
  if (a.cells == 0) return hipSuccess;
  if (!a.hist || !a.rank_level || !a.above || !a.total || a.n_levels < 2u || a.n_levels > SCN_LEVELS_EDGES_MAX + 1u || a.permille > 1000u ||
      a.level >= a.n_levels)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(scn_levels_summary_kernel, dim3((a.cells + kSummaryWaves - 1u) / kSummaryWaves), dim3(256), 0, stream, a);
  return hipGetLastError();
}
