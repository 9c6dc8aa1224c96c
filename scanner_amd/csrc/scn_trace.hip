// scn_trace.hip -- the sweep trace (definition: scanner_hip.h, "Sweep trace"): the kernel that folds the spectrum of a collected
// submit into the plan's power-versus-frequency trace (scn_plan_update_trace) -- per cell of a frequency grid the largest and the
// smallest dB value that fell into it and their number.  Integers and compares only (a float is read as its bits, ordered by the
// floor detector's key; the one double addition and cast are those every record's freq_hz is made with: scn_trace.h), and maximum,
// minimum and an integer sum commute: the trace is the same bits whatever the order the units, waves and atomics arrive in.
//
// One TEAM per unit and trip (the team model of scn_detect.h: a wave for n <= 512, a workgroup of 256 up to 4096 points, of 1024
// above; persistent, walking units with the grid's stride).  The team streams the unit's row through a descriptor of exactly that
// row, 16 bytes per lane where n % 4 == 0 and the row starts 16-byte aligned (four consecutive natural bins j), 4 bytes otherwise;
// a lane keeps U loads in flight before it looks at the first (U = 1, 2, 4 as in scn_baseline.hip).  Natural order is fftshift
// order rotated by n / 2: i grows with j but for one wrap, so the cell c of consecutive bins almost never decreases and mostly stays.
// A unit whose start frequency is a whole number of hertz on the grid takes its cells from integers alone (scn_trace_unit: the same
// arithmetic, one 64-bit division per unit and a 32-bit one per bin); any other unit makes the double addition and the cast per bin.
//
// The point is to keep atomics rare.  A RUN is a stretch of neighbouring bins with the same c -- nothing more: correctness does not
// rest on c being monotonic (a negative start frequency wraps to a huge f in the middle of a unit; the fftshift wrap, a masked
// bin, a NaN all merely end a run).  Per load:
//   lane   the lane's W bins are merged while c stays; a lane whose bins are not all of one c (a cell boundary, a mask edge)
//          keeps its first and its last run for the wave and issues the ones in between itself,
//   wave   the lanes' runs are reduced over runs of equal c in neighbouring lanes -- key maximum, key minimum, count; six steps
//          of cross-lane moves, bounded by the run's first lane (a ballot) -- and the LAST lane of a run issues
//   ONE no-return atomic triple: atomicMax and atomicMin on the uint32 keys, a 64-bit atomicAdd on the count.
// A whole wave in one cell, the common case of a wide cell, is one triple by one lane per load; a wave without an evaluated bin
// (the band edges: a quarter of the row at the default bandwidth) issues nothing and skips the reduction.  Runs are not carried
// from one load to the next, nor across a team's waves: at 4096 points and 256 bins per wave and load that is 16 triples per unit
// where a carried run would issue one per cell.  cell_hz = bin_step is the worst case: a triple per evaluated bin.
// The atomics execute at the memory side (vector global atomics, device scope); nothing else is written, no LDS, no barrier.
//
// Grid: kTraceBlocksPerCu workgroups per CU, stated -- not an occupancy query --, so that a test can size the batch that takes
// every team through its loop twice; no more workgroups than units need (scn_team_grid).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scn_detect.h"
#include "scn_hitlist.h"  // scn_unit_centre
#include "scn_trace.h"

namespace {

typedef float v4f_t __attribute__((ext_vector_type(4)));

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

// one run's triple (count != 0, c < cells: scn_trace_cell's promise); the results are not used: no-return atomics
__device__ __forceinline__ void issue_run(const ScnTraceArgs &a, uint32_t c, uint32_t kmax, uint32_t kmin, uint32_t count) {
  atomicMax(a.max_key + c, kmax);
  atomicMin(a.min_key + c, kmin);
  atomicAdd(a.count + c, (unsigned long long)count);
}

// The wave's W * 64 bins of one load: bins j0 ... j0 + W - 1 in this lane, their bits in v
template <int W>
__device__ __forceinline__ void fold_load(const ScnTraceArgs &a, const uint32_t (&v)[W], uint32_t j0, uint32_t to_i, uint32_t bin_step, double start_frequency,
                                          const ScnTraceUnit &unit, uint32_t lane) {
  const uint32_t n = a.n;
  // the lane's bins merged while the cell stays: (rc, rmax, rmin, rcount) is the run the lane is in, in the end its LAST; a lane
  // whose bins are not all of one cell keeps its FIRST run in (fc, ...) and issues the ones in between as they end
  uint32_t rc = kTraceNoCell, rmax = 0, rmin = 0, rcount = 0;
  uint32_t fc = kTraceNoCell, fmax = 0, fmin = 0, fcount = 0;
  bool one_cell = true;  // every bin of the lane has the same c (kTraceNoCell included)
#pragma unroll
  for (int x = 0; x < W; x++) {
    const uint32_t j = j0 + (uint32_t)x, i = shift_of_bin(j, to_i, n);
    const bool folds = j < n && scn_bin_evaluated(j, i, n, a) && !scn_trace_is_nan(v[x]);
    uint32_t c = kTraceNoCell;
    if (folds)  // (unit.exact is the same in every lane of a wave)
      c = unit.exact ? scn_trace_cell_in_unit(unit, i * bin_step, a.cell_hz, a.cells)
                     : scn_trace_cell(scn_trace_freq(start_frequency, i, bin_step), a.f0_hz, a.cell_hz, a.cells);
    const uint32_t key = scn_trace_key(v[x]);
    if (x == 0 || c != rc) {
      if (x != 0) {
        if (one_cell) {
          fc = rc, fmax = rmax, fmin = rmin, fcount = rcount;
          one_cell = false;
        } else if (rc != kTraceNoCell) {
          issue_run(a, rc, rmax, rmin, rcount);
        }
      }
      rc = c;
      rmax = rmin = key;
      rcount = 1u;
    } else {
      rmax = key > rmax ? key : rmax;
      rmin = key < rmin ? key : rmin;
      rcount++;
    }
  }
  const uint32_t hc = one_cell ? rc : fc;  // the cell the lane begins in
  if (__ballot(rc != kTraceNoCell || hc != kTraceNoCell) == 0ull) return;  // (wave-uniform) nothing evaluated here
  // Runs over neighbouring lanes.  A lane JOINS when its first run continues the run the lane before ends in.  The lanes' last runs
  // are scanned: a lane of one cell that joins extends the scan's run, every other lane begins one.  first[l] = the lane that does.
  const uint32_t before = (uint32_t)__shfl_up((int)rc, 1, 64);
  const bool joins = lane != 0u && hc != kTraceNoCell && hc == before;
  const unsigned long long heads = __ballot(!(one_cell && joins));
  const uint32_t first = 63u - (uint32_t)__builtin_clzll(heads & (~0ull >> (63u - lane)));  // (bit 0 is set: never clz(0))
  const uint32_t reach = lane - first;  // lanes of the run below this one
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {  // inclusive scan inside the run: after step `off` a lane holds min(2 off, reach + 1) lanes
    const uint32_t pmax = (uint32_t)__shfl_up((int)rmax, off, 64), pmin = (uint32_t)__shfl_up((int)rmin, off, 64);
    const uint32_t pcount = (uint32_t)__shfl_up((int)rcount, off, 64);
    if (reach >= off) {
      rmax = pmax > rmax ? pmax : rmax;
      rmin = pmin < rmin ? pmin : rmin;
      rcount += pcount;
    }
  }
  // a lane of several cells: its first run takes what the lanes before it gathered, if it joins them, and is issued here
  const uint32_t gmax = (uint32_t)__shfl_up((int)rmax, 1, 64), gmin = (uint32_t)__shfl_up((int)rmin, 1, 64);
  const uint32_t gcount = (uint32_t)__shfl_up((int)rcount, 1, 64);
  if (!one_cell && fc != kTraceNoCell) {
    if (joins) {
      fmax = gmax > fmax ? gmax : fmax;
      fmin = gmin < fmin ? gmin : fmin;
      fcount += gcount;
    }
    issue_run(a, fc, fmax, fmin, fcount);
  }
  // the last lane of a scanned run holds all of it -- unless the lane behind it joins: then that lane carries it on
  const bool joined = __shfl_down((int)joins, 1, 64) != 0;
  if ((lane == 63u || !joined) && rc != kTraceNoCell) issue_run(a, rc, rmax, rmin, rcount);
}

template <int T, bool VEC, int U>
__global__ __launch_bounds__(T == 64 ? 256 : T) void scn_trace_fold_kernel(ScnTraceArgs a) {
  typedef Team<T> G;
  constexpr int W = VEC ? 4 : 1;
  const uint32_t t = G::t(), team = G::team(), lane = G::lane();
  const uint32_t n = a.n, to_i = n - n / 2u;
  const uint32_t bin_step = a.sample_rate / n;  // process.cpp:39 (truncating)
  const uint32_t trips = (n + (uint32_t)(W * T) - 1u) / (uint32_t)(W * T);
  for (uint32_t u0 = blockIdx.x * G::TEAMS + team; u0 < a.n_units; u0 += gridDim.x * G::TEAMS) {
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)u0);  // (the same in every lane of a wave)
    const __amdgpu_buffer_rsrc_t rin = spectrum_rsrc(a, u);
    const double start_frequency = scn_trace_start(scn_unit_centre(a, u), a.sample_rate);
    const ScnTraceUnit unit = scn_trace_unit(start_frequency, a.f0_hz, a.cell_hz);  // (one 64-bit division per unit instead of one per bin)
    for (uint32_t k0 = 0; k0 < trips; k0 += (uint32_t)U) {
      uint32_t v[U][W];
#pragma unroll
      for (int x = 0; x < U; x++)  // (a trip past the last: outside the descriptor, zeros, j >= n)
        load_bits<VEC>(rin, (t + (k0 + (uint32_t)x) * (uint32_t)T) * (uint32_t)(4 * W), v[x]);
#pragma unroll
      for (int x = 0; x < U; x++)
        if (k0 + (uint32_t)x < trips)  // (wave-uniform)
          fold_load<W>(a, v[x], (t + (k0 + (uint32_t)x) * (uint32_t)T) * (uint32_t)W, to_i, bin_step, start_frequency, unit, lane);
    }
  }
}

// workgroups per CU of the fold's grid, by workgroup size: stated, so that tests/trace_caps.py can restate it
constexpr int kTraceBlocksPerCu256 = 8, kTraceBlocksPerCu1024 = 2;

template <int T, bool VEC, int U>
hipError_t launch(const ScnTraceArgs &a, int num_cus, hipStream_t stream) {
  typedef Team<T> G;
  const int per_cu = G::BLOCK == 256u ? kTraceBlocksPerCu256 : kTraceBlocksPerCu1024;
  hipLaunchKernelGGL((scn_trace_fold_kernel<T, VEC, U>), dim3(scn_team_grid(a.n_units, G::TEAMS, num_cus, per_cu)), dim3(G::BLOCK), 0, stream, a);
  return hipGetLastError();
}

// U: loads of a lane in flight, the smallest of 1, 2, 4 that covers the row in one trip, or 4
template <int T, bool VEC>
hipError_t launch_team(const ScnTraceArgs &a, int num_cus, hipStream_t stream) {
  const uint32_t per_trip = (uint32_t)T * (VEC ? 4u : 1u), trips = (a.n + per_trip - 1u) / per_trip;
  if (trips <= 1u) return launch<T, VEC, 1>(a, num_cus, stream);
  if (trips <= 2u) return launch<T, VEC, 2>(a, num_cus, stream);
  return launch<T, VEC, 4>(a, num_cus, stream);
}

template <bool VEC>
hipError_t launch_size(const ScnTraceArgs &a, int num_cus, hipStream_t stream) {
  if (a.n <= 512u) return launch_team<64, VEC>(a, num_cus, stream);
  if (a.n <= 4096u) return launch_team<256, VEC>(a, num_cus, stream);
  return launch_team<1024, VEC>(a, num_cus, stream);
}

}  // namespace

hipError_t scn_launch_trace_fold(const ScnTraceArgs &a, int num_cus, hipStream_t stream) {
  if (a.n_units == 0) return hipSuccess;
  if (a.n == 0 || a.n > 65536u || a.sample_rate == 0 || a.cell_hz == 0 || a.cells == 0 || a.cells > SCN_TRACE_CELLS_MAX || !a.power_db || !a.center_freq ||
      !a.max_key || !a.min_key || !a.count)
    return hipErrorInvalidValue;
  const bool vec = a.n % 4u == 0 && ((uintptr_t)a.power_db & 15u) == 0;
  return vec ? launch_size<true>(a, num_cus, stream) : launch_size<false>(a, num_cus, stream);
}
