// scn_baseline.hip -- the baseline detector (scn_plan_desc.detect = SCN_DETECT_BASELINE; definition: scanner_hip.h, "Baseline
// detector") and the kernel that folds a collected spectrum into the baseline (scn_plan_update_baseline).
//
// Detect: one kernel behind the transform, on the dB spectrum the spectrum-only specialisations store (the team model and the hit
// pass are scn_detect.h's).  Unit u (a buffer, or a group of an averaged plan) is held against row (first + u) % rows of the plan's baseline: an
// evaluated bin j is a hit iff power_db[u][j] > baseline_db[row][j] + threshold -- ONE float addition, a strict compare -- and is
// recorded as the FFT kernels' own hit paths record it: {i, power_db} in the unit's region, in any order, and the unit's count.
// Scan, compaction, signals and gather read them unchanged.  The kernel only READS the baseline.  There is nothing to select, so it
// is a single streaming pass over the two rows: no float arithmetic beyond that addition, no global atomics, nothing zeroed
// beforehand (every unit's count is written).
//
// Sizes: n <= 512: T = 64, n <= 4096: T = 256, above: T = 1024.
// Loads (VEC): rows that start 16-byte aligned -- n % 4 == 0 and both base pointers 16-byte aligned -- are read 16 bytes per lane,
// four consecutive bins j = 4 q ... 4 q + 3; every other size (odd n: row u starts 4-byte aligned only; n = 18: 8-byte) takes the
// 4-byte form, a bin per lane and load.  A lane keeps U loads of each row in flight before it looks at the first: U = 1, 2 or 4,
// the smallest that covers trips = ceil(n / (T * bins per load)) or 4.  So
//   16 ... 256 (n % 4 == 0)  <64, VEC, 1>      512 <64, VEC, 2>      1000, 1024 <256, VEC, 1>     2048 <256, VEC, 2>
//   4096 <256, VEC, 4>       8192 <1024, VEC, 2>      16384 ... 65536 <1024, VEC, 4>
//   18, 1001 and every n % 4 != 0: <64 | 256 | 1024, scalar, U by the same rule> (n <= 64: U = 1, n <= 128: 2, ...)
// The baseline row is read through a descriptor of exactly that row, as the spectrum's is: a load past either reads 0 and its bins
// are not evaluated (j >= n).
// Cache policy: default on both streams.  The baseline rows are re-read every sweep and must stay cacheable.  The spectrum was
// written by the transform immediately before, on the same stream, and is read again by scn_collect's copy (spectrum + hits plans)
// or by scn_plan_update_baseline: a non-temporal read would not save a fetch that reaches memory, and was not measured.
// One slot grab per wave and load: a wave without a hit in it touches neither LDS nor memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/scanner_hip.h"  // SCN_BASELINE_*
#include "scn_detect.h"

namespace {

typedef float v4f_t __attribute__((ext_vector_type(4)));

// W consecutive floats at byte offset `off` of the row behind r (outside the row: zeros)
template <bool VEC>
__device__ __forceinline__ void load_bins(__amdgpu_buffer_rsrc_t r, uint32_t off, float (&v)[VEC ? 4 : 1]) {
  if constexpr (VEC) {
    const v4f_t x = __builtin_bit_cast(v4f_t, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
    v[0] = x.x;
    v[1] = x.y;
    v[2] = x.z;
    v[3] = x.w;
  } else {
    v[0] = __uint_as_float((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
  }
}

template <int T, bool VEC, int U>
__global__ __launch_bounds__(T == 64 ? 256 : T) void scn_baseline_kernel(ScnBaselineArgs a) {
  typedef Team<T> G;
  constexpr uint32_t TEAMS = G::TEAMS;
  constexpr int W = VEC ? 4 : 1;
  __shared__ uint32_t s_count[TEAMS];
  const uint32_t t = G::t(), team = G::team(), lane = G::lane();
  const uint32_t n = a.n, to_i = n - n / 2u;
  const uint32_t trips = (n + (uint32_t)(W * T) - 1u) / (uint32_t)(W * T);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t u0 = blockIdx.x * TEAMS + team; u0 < a.n_units; u0 += gridDim.x * TEAMS) {
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)u0);  // (the same in every lane of a wave)
    const uint32_t row = scn_baseline_row(a.first, u, a.rows);
    const __amdgpu_buffer_rsrc_t rin = spectrum_rsrc(a, u);
    const __amdgpu_buffer_rsrc_t rbase = make_rsrc(a.baseline_db + (size_t)row * n, n * 4u);
    const __amdgpu_buffer_rsrc_t rhit = region_rsrc(a, u);
    if (t == 0) s_count[team] = 0u;
    team_sync<T>();
    for (uint32_t k0 = 0; k0 < trips; k0 += (uint32_t)U) {
      float p[U][W], b[U][W];
#pragma unroll
      for (int x = 0; x < U; x++) {  // (a trip past the last: outside both descriptors, zeros, j >= n)
        const uint32_t off = (t + (k0 + (uint32_t)x) * (uint32_t)T) * (uint32_t)(4 * W);
        load_bins<VEC>(rin, off, p[x]);
        load_bins<VEC>(rbase, off, b[x]);
      }
#pragma unroll
      for (int x = 0; x < U; x++) {
        const uint32_t j0 = (t + (k0 + (uint32_t)x) * (uint32_t)T) * (uint32_t)W;
        unsigned long long m[W];
        uint32_t total = 0;
#pragma unroll
        for (int c = 0; c < W; c++) {
          const uint32_t j = j0 + (uint32_t)c;
          const uint32_t i = shift_of_bin(j, to_i, n);
          const bool hit = (j < n) & scn_bin_evaluated(j, i, n, a) & (p[x][c] > b[x][c] + a.threshold);  // (no branches)
          m[c] = __ballot(hit);
          total += (uint32_t)__popcll(m[c]);
        }
        if (total) {  // one slot grab for the wave, then the records at ballot-prefix positions
          uint32_t base = grab_slots(&s_count[team], total, lane);
#pragma unroll
          for (int c = 0; c < W; c++) {
            const uint32_t i = shift_of_bin(j0 + (uint32_t)c, to_i, n);
            store_record(rhit, base, m[c], (m[c] >> lane) & 1ull, below, i, __float_as_uint(p[x][c]));
          }
        }
      }
    }
    team_sync<T>();  // every wave's grabs are in s_count
    if (t == 0) a.counts[u] = s_count[team];  // (the same thread zeroes it for the team's next unit: no barrier in between)
  }
}

template <int T, bool VEC, int U>
hipError_t launch(const ScnBaselineArgs &a, int num_cus, hipStream_t stream) {
  typedef Team<T> G;  // (the fallback: 8 workgroups of 256 threads or 2 of 1024 per CU)
  return launch_teams<scn_baseline_kernel<T, VEC, U>, G::BLOCK, G::TEAMS>(0, G::BLOCK == 256u ? 8 : 2, a, num_cus, stream);
}

template <int T, bool VEC>
hipError_t launch_team(const ScnBaselineArgs &a, int num_cus, hipStream_t stream) {
  const uint32_t per_trip = (uint32_t)T * (VEC ? 4u : 1u), trips = (a.n + per_trip - 1u) / per_trip;
  if (trips <= 1u) return launch<T, VEC, 1>(a, num_cus, stream);
  if (trips <= 2u) return launch<T, VEC, 2>(a, num_cus, stream);
  return launch<T, VEC, 4>(a, num_cus, stream);
}

template <bool VEC>
hipError_t launch_size(const ScnBaselineArgs &a, int num_cus, hipStream_t stream) {
  if (a.n <= 512u) return launch_team<64, VEC>(a, num_cus, stream);
  if (a.n <= 4096u) return launch_team<256, VEC>(a, num_cus, stream);
  return launch_team<1024, VEC>(a, num_cus, stream);
}

// Element-wise over units x n: a workgroup per unit (walking units with the grid's stride), its threads over the row's bins.
// units <= rows (the caller's check), so no row is named by two units of one launch: no two threads write the same word.
__global__ __launch_bounds__(256) void scn_baseline_update_kernel(ScnBaselineArgs a) {
  const uint32_t n = a.n;
  for (uint32_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.power_db) + (size_t)u * n;
    uint32_t *dst = reinterpret_cast<uint32_t *>(a.baseline_db) + (size_t)scn_baseline_row(a.first, u, a.rows) * n;
    for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
      const uint32_t v = src[j];
      if (a.op == SCN_BASELINE_SET || floor_key(v) > floor_key(dst[j])) dst[j] = v;  // (the bits as they are: no float is computed)
    }
  }
}

bool args_ok(const ScnBaselineArgs &a) {
  return a.n != 0 && a.n <= 65536u && a.rows != 0 && a.first < a.rows && (uint64_t)a.first + a.n_units <= 0xffffffffull && a.power_db && a.baseline_db;
}

}  // namespace

hipError_t scn_launch_baseline_detect(const ScnBaselineArgs &a, int num_cus, hipStream_t stream) {
  if (a.n_units == 0) return hipSuccess;
  if (!args_ok(a) || a.hit_region == 0 || !a.hits || !a.counts) return hipErrorInvalidValue;
  const bool vec = a.n % 4u == 0 && (((uintptr_t)a.power_db | (uintptr_t)a.baseline_db) & 15u) == 0;
  return vec ? launch_size<true>(a, num_cus, stream) : launch_size<false>(a, num_cus, stream);
}

hipError_t scn_launch_baseline_update(const ScnBaselineArgs &a, hipStream_t stream) {
  if (a.n_units == 0) return hipSuccess;
  if (!args_ok(a) || a.n_units > a.rows || (a.op != SCN_BASELINE_SET && a.op != SCN_BASELINE_MAX)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scn_baseline_update_kernel, dim3(a.n_units < 65536u ? a.n_units : 65536u), dim3(256), 0, stream, a);
  return hipGetLastError();
}
