// scn_emitters.hip -- the trace emitters (definition: scanner_hip.h, "Trace emitters"; arithmetic: scn_emitters.h): the kernels that
// segment a window of a plan's trace into runs of on cells and leave one record per run (scn_plan_trace_emitters), and the kernel
// that takes a host trace into the plan's (scn_plan_merge_trace).  Integers and compares only -- a cell's value is read as its bits,
// the spread's one float32 subtraction is scn_emitters.h's --, and an emitter that spans lanes, waves and workgroups is joined by
// integer atomics alone: maximum and an integer sum commute, so the list is the same bits on every run.
//
// No thread and no wave walks a run: every emitter shape -- the whole window one emitter, every other cell one, a run across every
// workgroup -- costs the same passes over the window.
//
// A TILE is kEmitTile consecutive cells of the window, worked by ONE wave in kEmitTile / 64 trips of 64 cells, a cell per lane: what
// is on is a ballot, so the last on cell before a lane is a count of leading zeros and an emitter's index a population count.
// Four tiles (waves) per workgroup; no LDS, no barrier, and no grid loop -- a window has at most kEmitTilesMax tiles.
//   count   per tile: its last and its first on cell, and its starts BY THE GAP RULE WITH NOTHING BEFORE THE TILE (so that its
//           first on cell counts as a start).
//   scan    one workgroup, kEmitScanPerThread consecutive tiles per thread: the last on cell before each tile (a maximum scan) --
//           which tells whether the tile's first on cell does start an emitter or carries one on --, then the starts before each
//           tile (a sum scan) and the window's total.
//   build   per tile, with its two carries: each lane's emitter index e, and per trip a segmented scan over the lanes of equal e
//           (six steps of cross-lane moves, bounded by the segment's first lane) of the peak key (maximum), the on cells and
//           their counts (sums) and the last on cell (maximum).  A segment's last lane holds the segment and issues ONE set of
//           no-return atomics on acc[e]; the segment a trip ends in is carried in registers into the next trip instead, so an
//           emitter costs one set per tile it touches, not one per trip.  An emitter's first cell stores acc[e].first_cell.
//   finish  a thread per record of the page: acc[e] and the peak cell's other extreme become the scn_emitter.
// The launches of one call follow each other on one stream: a kernel boundary is what makes one pass's stores visible to the next.
//
// The spread on the device: hipcc compiles this file with f32 denormals on (the code object's float_denorm_mode_32 is 3, preserve
// source and destination), and v_sub_f32 is IEEE round-to-nearest: max_db - min_db is the host's subtraction bit for bit, a
// denormal difference included (tests/test_emitters_gpu.py pins 1.5 * 2^-126 - 2^-126).  What is on is decided on keys, not by a
// float compare, so no float mode has a say in it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/scanner_hip.h"
#include "scn_emitters.h"
#include "scn_kernels.h"

namespace {

constexpr uint32_t kEmitTrips = kEmitTile / 64u;      // trips of a tile
constexpr uint32_t kEmitBlock = 256;                  // threads of a count / build workgroup: a tile per wave
constexpr uint32_t kEmitTilesPerBlock = kEmitBlock / 64u;
constexpr uint32_t kEmitInFlight = 4;                 // trips whose loads a lane issues before it looks at the first
constexpr uint32_t kEmitScanBlock = 1024, kEmitScanPerThread = 4;  // the scan's one workgroup
static_assert(kEmitTilesMax * kEmitTile == SCN_TRACE_CELLS_MAX && kEmitTile % (64u * kEmitInFlight) == 0, "whole tiles, whole groups of trips");
static_assert(kEmitScanBlock * kEmitScanPerThread == kEmitTilesMax, "the scan's one workgroup takes every tile of the largest window");
static_assert(sizeof(scn_emitter) == 56 && sizeof(ScnEmitterAcc) == 32, "the records' sizes");

// one cell as a lane sees it: on, and then its value's bits and its count
struct EmitCell {
  uint32_t v;
  unsigned long long count;
  bool on;
};

// cell `w` of the window (off beyond its end); LINE picks the arrays that are read
template <uint32_t LINE>
__device__ __forceinline__ EmitCell load_cell(const ScnEmittersArgs &a, uint32_t w) {
  EmitCell x = {0u, 0ull, false};
  if (w >= a.cells) return x;
  const uint32_t c = a.first_cell + w;
  const uint32_t mx = LINE != kEmitLineMin ? scn_trace_unkey(a.max_key[c]) : 0u;
  const uint32_t mn = LINE != kEmitLineMax ? scn_trace_unkey(a.min_key[c]) : 0u;
  x.count = a.count[c];
  x.v = scn_emit_value(LINE, mx, mn);
  x.on = scn_emit_on(x.count, x.v, a.threshold_bits);
  return x;
}

// One trip's on cells `mask` (wave-uniform, not 0), lane 0 at absolute cell c0; prev1: the last on cell before the trip + 1, 0 for
// none.  Returns the lanes that start an emitter, and moves prev1 behind the trip.
__device__ __forceinline__ unsigned long long trip_starts(unsigned long long mask, uint32_t c0, uint32_t lane, uint32_t max_gap, uint32_t &prev1) {
  const unsigned long long below = mask & ((1ull << lane) - 1ull);
  const uint32_t p1 = below ? c0 + (63u - (uint32_t)__builtin_clzll(below)) + 1u : prev1;
  const bool on = (mask >> lane) & 1ull;
  const unsigned long long starts = __ballot(on && scn_emit_starts(p1 != 0u, p1 - 1u, c0 + lane, max_gap));
  prev1 = c0 + (63u - (uint32_t)__builtin_clzll(mask)) + 1u;
  return starts;
}

template <uint32_t LINE>
__global__ __launch_bounds__(kEmitBlock) void scn_emitters_count_kernel(ScnEmittersArgs a) {
  const uint32_t lane = threadIdx.x & 63u, tile = blockIdx.x * kEmitTilesPerBlock + (threadIdx.x >> 6);
  const uint32_t w0 = tile * kEmitTile;
  if (w0 >= a.cells) return;  // (wave-uniform)
  uint32_t prev1 = 0, first = 0, starts = 0;
  for (uint32_t k0 = 0; k0 < kEmitTrips; k0 += kEmitInFlight) {
    EmitCell x[kEmitInFlight];
#pragma unroll
    for (uint32_t k = 0; k < kEmitInFlight; k++) x[k] = load_cell<LINE>(a, w0 + (k0 + k) * 64u + lane);
#pragma unroll
    for (uint32_t k = 0; k < kEmitInFlight; k++) {
      const unsigned long long mask = __ballot(x[k].on);
      if (mask == 0ull) continue;
      const uint32_t c0 = a.first_cell + w0 + (k0 + k) * 64u;
      if (prev1 == 0u) first = c0 + (uint32_t)__builtin_ctzll(mask);
      starts += (uint32_t)__builtin_popcountll(trip_starts(mask, c0, lane, a.max_gap, prev1));
    }
  }
  if (lane == 0u) {
    a.tile_last[tile] = prev1;
    a.tile_first[tile] = first;
    a.tile_starts[tile] = starts;
  }
}

// exclusive scan of one uint32 per thread over the scan's workgroup, identity 0 (a maximum of cells + 1, or a sum); *all: everything
template <bool MAX>
__device__ __forceinline__ uint32_t scan_block(uint32_t v, uint32_t *shared, uint32_t *all) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const uint32_t p = (uint32_t)__shfl_up((int)inc, off, 64);
    if (lane >= off) inc = MAX ? (p > inc ? p : inc) : inc + p;
  }
  uint32_t exc = (uint32_t)__shfl_up((int)inc, 1, 64);
  if (lane == 0u) exc = 0u;
  __syncthreads();  // (the array's readers of the scan before this one are done)
  if (lane == 63u) shared[wave] = inc;
  __syncthreads();
  uint32_t before = 0, whole = 0;
  for (uint32_t k = 0; k < kEmitScanBlock / 64u; k++) {
    const uint32_t s = shared[k];
    if (k < wave) before = MAX ? (s > before ? s : before) : before + s;
    whole = MAX ? (s > whole ? s : whole) : whole + s;
  }
  *all = whole;
  return MAX ? (before > exc ? before : exc) : before + exc;
}

__global__ __launch_bounds__(kEmitScanBlock) void scn_emitters_scan_kernel(ScnEmittersArgs a, uint32_t tiles) {
  __shared__ uint32_t shared[kEmitScanBlock / 64u];
  const uint32_t t0 = threadIdx.x * kEmitScanPerThread;
  uint32_t last[kEmitScanPerThread], mine = 0, all;
#pragma unroll
  for (uint32_t k = 0; k < kEmitScanPerThread; k++) {
    last[k] = t0 + k < tiles ? a.tile_last[t0 + k] : 0u;
    mine = last[k] > mine ? last[k] : mine;  // (tiles lie in increasing cells: the maximum is the latest)
  }
  uint32_t prev1 = scan_block<true>(mine, shared, &all);
  uint32_t starts[kEmitScanPerThread], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kEmitScanPerThread; k++) {
    starts[k] = 0;
    if (t0 + k >= tiles) continue;
    a.carry_last[t0 + k] = prev1;
    starts[k] = a.tile_starts[t0 + k];
    // the tile's first on cell was counted as a start: it is none where an on cell before the tile lies within the gap
    if (last[k] != 0u && !scn_emit_starts(prev1 != 0u, prev1 - 1u, a.tile_first[t0 + k], a.max_gap)) starts[k]--;
    sum += starts[k];
    prev1 = last[k] > prev1 ? last[k] : prev1;
  }
  uint32_t before = scan_block<false>(sum, shared, &all);
#pragma unroll
  for (uint32_t k = 0; k < kEmitScanPerThread; k++) {
    if (t0 + k >= tiles) continue;
    a.carry_starts[t0 + k] = before;
    before += starts[k];
  }
  if (threadIdx.x == 0u) *a.total = all;
}

// what a lane, a segment or the carried segment holds of an emitter
struct EmitPart {
  unsigned long long key, count;
  uint32_t n, last;
};
__device__ __forceinline__ void join(EmitPart &p, const EmitPart &q) {
  p.key = q.key > p.key ? q.key : p.key;
  p.count += q.count;
  p.n += q.n;
  p.last = q.last > p.last ? q.last : p.last;
}
__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, uint32_t off) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), off, 64);
  return ((unsigned long long)hi << 32) | lo;
}
// one emitter's set of atomics (p.n != 0; e < acc_cap: the host sized acc by the scan's total); no result is used: no-return atomics
__device__ __forceinline__ void issue(const ScnEmittersArgs &a, uint32_t e, const EmitPart &p) {
  if (e >= a.acc_cap) return;
  ScnEmitterAcc *const r = a.acc + e;
  atomicMax(&r->key, p.key);
  atomicAdd(&r->count, p.count);
  atomicAdd(&r->n_cells, p.n);
  atomicMax(&r->last_cell, p.last);
}

template <uint32_t LINE>
__global__ __launch_bounds__(kEmitBlock) void scn_emitters_build_kernel(ScnEmittersArgs a) {
  const uint32_t lane = threadIdx.x & 63u, tile = blockIdx.x * kEmitTilesPerBlock + (threadIdx.x >> 6);
  const uint32_t w0 = tile * kEmitTile;
  if (w0 >= a.cells) return;  // (wave-uniform)
  uint32_t prev1 = a.carry_last[tile];
  uint32_t next_e = a.carry_starts[tile];  // the index the next start takes; next_e - 1: the emitter that is open
  EmitPart held = {0ull, 0ull, 0u, 0u};    // the segment the last trip ended in (emitter next_e - 1), the same in every lane; n 0: none
  for (uint32_t k0 = 0; k0 < kEmitTrips; k0 += kEmitInFlight) {
    EmitCell x[kEmitInFlight];
#pragma unroll
    for (uint32_t k = 0; k < kEmitInFlight; k++) x[k] = load_cell<LINE>(a, w0 + (k0 + k) * 64u + lane);
#pragma unroll
    for (uint32_t k = 0; k < kEmitInFlight; k++) {
      const unsigned long long mask = __ballot(x[k].on);
      if (mask == 0ull) continue;  // (wave-uniform; what is held stays held)
      const uint32_t c0 = a.first_cell + w0 + (k0 + k) * 64u, c = c0 + lane;
      const unsigned long long starts = trip_starts(mask, c0, lane, a.max_gap, prev1);
      // a lane's emitter: the starts up to and including it.  (Lanes before the window's first start hold next_e - 1 = 0xffffffff: they
      // are off -- an on cell with nothing before it starts -- and their segment holds nothing.)
      const uint32_t e = next_e + (uint32_t)__builtin_popcountll(starts & (~0ull >> (63u - lane))) - 1u;
      const bool start = (starts >> lane) & 1ull;
      if (start && e < a.acc_cap) a.acc[e].first_cell = c;
      EmitPart p = {x[k].on ? scn_emit_peak_key(x[k].v, c) : 0ull, x[k].on ? x[k].count : 0ull, x[k].on ? 1u : 0u, x[k].on ? c : 0u};
      if (held.n != 0u && lane == 0u) {  // the held segment: carried on by lane 0, or over where lane 0 starts the next emitter
        if (start) issue(a, next_e - 1u, held);
        else join(p, held);
      }
      // segments: lane 0 and every start begin one; an inclusive scan inside each
      const unsigned long long heads = starts | 1ull;
      const uint32_t head = 63u - (uint32_t)__builtin_clzll(heads & (~0ull >> (63u - lane)));
      const uint32_t reach = lane - head;
#pragma unroll
      for (uint32_t off = 1; off < 64u; off <<= 1) {
        EmitPart q;
        q.key = shfl_up64(p.key, off);
        q.count = shfl_up64(p.count, off);
        q.n = (uint32_t)__shfl_up((int)p.n, off, 64);
        q.last = (uint32_t)__shfl_up((int)p.last, off, 64);
        if (reach >= off) join(p, q);
      }
      // a segment's last lane holds it; the trip's last segment is held for the next trip
      if (lane != 63u && ((starts >> (lane + 1u)) & 1ull) && p.n != 0u) issue(a, e, p);
      held.key = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(p.key >> 32), 63, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)p.key, 63, 64);
      held.count = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(p.count >> 32), 63, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)p.count, 63, 64);
      held.n = (uint32_t)__shfl((int)p.n, 63, 64);
      held.last = (uint32_t)__shfl((int)p.last, 63, 64);
      next_e += (uint32_t)__builtin_popcountll(starts);
    }
  }
  if (held.n != 0u && lane == 0u) issue(a, next_e - 1u, held);
}

__global__ __launch_bounds__(256) void scn_emitters_finish_kernel(ScnEmittersArgs a) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= a.out_cap) return;
  const ScnEmitterAcc acc = a.acc[a.first + k];
  const uint32_t pc = scn_emit_peak_cell(acc.key);
  scn_emitter r;
  r.start_hz = scn_emit_hz(a.f0_hz, a.cell_hz, acc.first_cell);
  r.stop_hz = scn_emit_hz(a.f0_hz, a.cell_hz, (uint64_t)acc.last_cell + 1u);
  r.peak_hz = scn_emit_hz(a.f0_hz, a.cell_hz, pc);
  r.count = acc.count;
  r.first_cell = acc.first_cell;
  r.last_cell = acc.last_cell;
  r.peak_cell = pc;
  r.n_cells = acc.n_cells;
  r.peak_db = scn_emit_float(scn_emit_peak_bits(acc.key));
  // (pc lies in the window: it is an on cell's.  An acc that was never gathered would read cell 0xffffffff: bounded here.)
  const bool inside = pc - a.first_cell < a.cells;
  r.peak_other_db = scn_emit_float(inside ? scn_emit_other(a.line, scn_trace_unkey(a.max_key[pc]), scn_trace_unkey(a.min_key[pc])) : 0u);
  ((scn_emitter *)a.out)[k] = r;
}

__global__ __launch_bounds__(256) void scn_trace_merge_kernel(ScnTraceMergeArgs a) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= a.cells) return;
  const uint32_t c = a.first_cell + w;
  const uint32_t hi = scn_trace_key(a.src_max[w]), lo = scn_trace_key(a.src_min[w]);
  if (hi > a.max_key[c]) a.max_key[c] = hi;
  if (lo < a.min_key[c]) a.min_key[c] = lo;
  a.count[c] += a.src_count[w];
}

uint32_t tiles_of(uint32_t cells) { return cells / kEmitTile + (cells % kEmitTile != 0u ? 1u : 0u); }
bool window_ok(const ScnEmittersArgs &a) {
  return a.cells != 0 && a.cells <= SCN_TRACE_CELLS_MAX && a.first_cell <= SCN_TRACE_CELLS_MAX - a.cells && a.line <= kEmitLineSpread && a.max_key && a.min_key &&
         a.count && a.tile_last && a.tile_first && a.tile_starts && a.carry_last && a.carry_starts && a.total;
}

}  // namespace

hipError_t scn_launch_emitters_count(const ScnEmittersArgs &a, hipStream_t stream) {
  if (!window_ok(a)) return hipErrorInvalidValue;
  const uint32_t tiles = tiles_of(a.cells);
  const dim3 grid((tiles + kEmitTilesPerBlock - 1u) / kEmitTilesPerBlock), block(kEmitBlock);
  if (a.line == kEmitLineMax) hipLaunchKernelGGL(scn_emitters_count_kernel<kEmitLineMax>, grid, block, 0, stream, a);
  else if (a.line == kEmitLineMin) hipLaunchKernelGGL(scn_emitters_count_kernel<kEmitLineMin>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(scn_emitters_count_kernel<kEmitLineSpread>, grid, block, 0, stream, a);
  if (const hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(scn_emitters_scan_kernel, dim3(1), dim3(kEmitScanBlock), 0, stream, a, tiles);
  return hipGetLastError();
}

hipError_t scn_launch_emitters_build(const ScnEmittersArgs &a, hipStream_t stream) {
  if (!window_ok(a) || !a.acc) return hipErrorInvalidValue;
  const uint32_t tiles = tiles_of(a.cells);
  const dim3 grid((tiles + kEmitTilesPerBlock - 1u) / kEmitTilesPerBlock), block(kEmitBlock);
  if (a.line == kEmitLineMax) hipLaunchKernelGGL(scn_emitters_build_kernel<kEmitLineMax>, grid, block, 0, stream, a);
  else if (a.line == kEmitLineMin) hipLaunchKernelGGL(scn_emitters_build_kernel<kEmitLineMin>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(scn_emitters_build_kernel<kEmitLineSpread>, grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t scn_launch_emitters_finish(const ScnEmittersArgs &a, hipStream_t stream) {
  if (a.out_cap == 0) return hipSuccess;
  if (!window_ok(a) || !a.acc || !a.out || a.first > a.acc_cap || a.out_cap > a.acc_cap - a.first) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scn_emitters_finish_kernel, dim3((a.out_cap + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t scn_launch_trace_merge(const ScnTraceMergeArgs &a, hipStream_t stream) {
  if (a.cells == 0) return hipSuccess;
  if (a.cells > SCN_TRACE_CELLS_MAX || a.first_cell > SCN_TRACE_CELLS_MAX - a.cells || !a.max_key || !a.min_key || !a.count || !a.src_max || !a.src_min ||
      !a.src_count)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(scn_trace_merge_kernel, dim3((a.cells + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}
