// scn_history.hip -- the hit history (definition: scanner_hip.h, "Hit history"): the kernel that folds a collected submit's hits
// into the per-entry history words (scn_plan_update_history) and the two kernels that make the confirmed list -- the records whose
// bin was a hit in at least m of the last `window` visits of its table entry (scn_collect_confirmed).  Integers and compares only:
// no float is read as a float anywhere in this file, so the history and the confirmed list are the same bits on every route.
//
// Fold: one TEAM per unit (the team model of scn_detect.h: a wave for n <= 512, a workgroup of 256 up to 4096 points, of 1024
// above).  The team rebuilds the unit's hit bitmap in LDS from its UNORDERED region, as the compaction kernel does (LDS atomicOr,
// n / 32 words: 8 KiB at 65536 points), and then streams the unit's row: word = (word << 1) | bit for EVERY bin, hit or not --
// a bin that was no hit, or that the mask removes, shifts in a 0.  n % 4 == 0: 16 bytes per lane and access (rows start at
// multiples of n words of a hipMalloc'd array: 16-byte aligned), U accesses of a lane in flight before the first store; every
// other n: 4 bytes.  One lane adds one to the row's visits (saturating).  units <= rows (the launcher's check), so no row is
// named by two units of one launch: no global atomics, no order between teams.  Traffic: 8 bytes per bin (the word read and
// written) plus 8 per stored record; the rows are read once and written once per fold, default cache policy (the next sweep's
// fold and every confirm read them again).
//
// Confirm: a count kernel and a build kernel around scn_launch_hit_scan, as the signals (scn_hits.hip).  One WAVE per unit with
// hits: the unit's hit bitmap as above, ANDed with its CONFIRMED bitmap -- bit i = scn_history_confirms(history[row][i]) -- which
// the wave makes 64 bins at a time: a coalesced 256-byte read of the row, one ballot, two bitmap words; runs of 64 bins without
// a hit are not read at all.  The count kernel stores the number of bits left; the build kernel ranks the region's records whose
// bit is left and writes them completed -- ranking and record are scn_hitlist.h's, the compaction kernel's own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scn_detect.h"
#include "scn_hitlist.h"

namespace {

typedef uint32_t v4u_t __attribute__((ext_vector_type(4)));

// bitmap words a team of T threads holds: the largest n its launcher gives it, / 32
template <int T>
constexpr uint32_t kFoldWords = T == 64 ? 512u / 32u : T == 256 ? 4096u / 32u : 65536u / 32u;

template <int T, bool VEC, int U>
__global__ __launch_bounds__(T == 64 ? 256 : T) void scn_history_fold_kernel(ScnHistoryArgs a) {
  typedef Team<T> G;
  constexpr uint32_t W = VEC ? 4u : 1u;
  __shared__ uint32_t s_bits[G::TEAMS * kFoldWords<T>];
  const uint32_t t = G::t(), team = G::team();
  uint32_t *const bits = s_bits + team * kFoldWords<T>;
  const uint32_t n = a.n, words = (n + 31u) / 32u;  // (words <= kFoldWords<T>: launch_size)
  const uint32_t accesses = n / W;                  // (VEC: n % 4 == 0)
  for (uint32_t u0 = blockIdx.x * G::TEAMS + team; u0 < a.n_units; u0 += gridDim.x * G::TEAMS) {
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)u0);  // (the same in every lane of a wave)
    const uint32_t row = scn_baseline_row(a.first, u, a.rows);
    const ScnDevHit *const region = a.regions + (size_t)u * a.hit_region;
    const uint32_t c = a.counts[u], stored = c < a.hit_region ? c : a.hit_region;
    for (uint32_t w = t; w < words; w += (uint32_t)T) bits[w] = 0u;
    team_sync<T>();
    for (uint32_t k = t; k < stored; k += (uint32_t)T) {
      const uint32_t i = region[k].i;
      if (i < n) atomicOr(&bits[i >> 5], 1u << (i & 31u));
    }
    team_sync<T>();
    uint32_t *const hrow = a.history + (size_t)row * n;
    for (uint32_t q0 = t; q0 < accesses; q0 += (uint32_t)(U * T)) {
      if constexpr (VEC) {
        v4u_t h[U];
#pragma unroll
        for (int x = 0; x < U; x++) {
          const uint32_t q = q0 + (uint32_t)(x * T);
          if (q < accesses) h[x] = reinterpret_cast<const v4u_t *>(hrow)[q];
        }
#pragma unroll
        for (int x = 0; x < U; x++) {
          const uint32_t q = q0 + (uint32_t)(x * T);
          if (q < accesses) {
            const uint32_t b4 = bits[q >> 3] >> ((q & 7u) * 4u);  // bins 4 q ... 4 q + 3
            v4u_t r;
            r.x = scn_history_fold(h[x].x, b4);
            r.y = scn_history_fold(h[x].y, b4 >> 1);
            r.z = scn_history_fold(h[x].z, b4 >> 2);
            r.w = scn_history_fold(h[x].w, b4 >> 3);
            reinterpret_cast<v4u_t *>(hrow)[q] = r;
          }
        }
      } else {
        uint32_t h[U];
#pragma unroll
        for (int x = 0; x < U; x++) {
          const uint32_t q = q0 + (uint32_t)(x * T);
          if (q < accesses) h[x] = hrow[q];
        }
#pragma unroll
        for (int x = 0; x < U; x++) {
          const uint32_t q = q0 + (uint32_t)(x * T);
          if (q < accesses) hrow[q] = scn_history_fold(h[x], bits[q >> 5] >> (q & 31u));
        }
      }
    }
    if (t == 0) {
      const uint32_t v = a.visits[row];
      if (v != 0xffffffffu) a.visits[row] = v + 1u;
    }
    team_sync<T>();  // the bitmap is reused by the team's next unit
  }
}

template <int T, bool VEC, int U>
hipError_t launch_fold(const ScnHistoryArgs &a, int num_cus, hipStream_t stream) {
  typedef Team<T> G;  // (the fallback: 8 workgroups of 256 threads or 2 of 1024 per CU)
  return launch_teams<scn_history_fold_kernel<T, VEC, U>, G::BLOCK, G::TEAMS>(0, G::BLOCK == 256u ? 8 : 2, a, num_cus, stream);
}

// U: accesses of a lane in flight, the smallest of 1, 2, 4 that covers the row in one trip, or 4
template <int T, bool VEC>
hipError_t launch_fold_team(const ScnHistoryArgs &a, int num_cus, hipStream_t stream) {
  const uint32_t per_trip = (uint32_t)T * (VEC ? 4u : 1u), trips = (a.n + per_trip - 1u) / per_trip;
  if (trips <= 1u) return launch_fold<T, VEC, 1>(a, num_cus, stream);
  if (trips <= 2u) return launch_fold<T, VEC, 2>(a, num_cus, stream);
  return launch_fold<T, VEC, 4>(a, num_cus, stream);
}

template <bool VEC>
hipError_t launch_fold_size(const ScnHistoryArgs &a, int num_cus, hipStream_t stream) {
  if (a.n <= 512u) return launch_fold_team<64, VEC>(a, num_cus, stream);
  if (a.n <= 4096u) return launch_fold_team<256, VEC>(a, num_cus, stream);
  return launch_fold_team<1024, VEC>(a, num_cus, stream);
}

// One wave: bits[0, words) = the unit's hit bitmap AND its confirmed bitmap, 64 bins (two words) a step; a step without a hit
// reads nothing of the row.  Returns the number of bits left, in every lane.
__device__ __forceinline__ uint32_t confirmed_bitmap(const ScnConfirmArgs &a, uint32_t b, const ScnDevHit *region, const ScnDevHit &first64,
                                                     uint32_t stored, uint32_t words, uint32_t lane, uint32_t *bits) {
  scn_wave_hit_bitmap(region, first64, stored, words, lane, bits);
  const uint32_t *const hrow = a.history + (size_t)scn_baseline_row(a.hist_first, b, a.rows) * a.n;
  uint32_t left = 0;
  for (uint32_t w = 0; w < words; w += 2u) {  // (wave-uniform: every lane reads the same two LDS words)
    const uint32_t lo = bits[w], hi = w + 1u < words ? bits[w + 1u] : 0u;
    if ((lo | hi) == 0u) continue;
    const uint32_t i = w * 32u + lane;
    const bool hit = (((lane < 32u ? lo : hi) >> (lane & 31u)) & 1u) != 0u;
    const unsigned long long conf = __ballot(hit && i < a.n && scn_history_confirms(hrow[i], a.mask, a.m));
    if (lane == 0) {
      bits[w] = (uint32_t)conf;
      if (w + 1u < words) bits[w + 1u] = (uint32_t)(conf >> 32);
    }
    left += (uint32_t)__popcll(conf);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return left;
}

// (workgroups of 256 threads = four waves, no s_setprio: as the list kernels, these run beside other slots' FFT launches)
__global__ __launch_bounds__(256) void scn_confirm_count_kernel(ScnConfirmArgs a) {
  extern __shared__ uint32_t smem[];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t words = (a.n + 31u) / 32u;
  uint32_t *const bits = smem + (size_t)wave * 2u * words;
  for (uint32_t b = blockIdx.x * 4u + wave; b < a.n_buffers; b += gridDim.x * 4u) {
    const ScnDevHit *const region = a.regions + (size_t)b * a.hit_region;
    const uint32_t c = a.offsets[b + 1u] - a.offsets[b];
    uint32_t left = 0;
    if (c) {
      const ScnDevHit first64 = region[lane < a.hit_region ? lane : 0u];
      left = confirmed_bitmap(a, b, region, first64, c < a.hit_region ? c : a.hit_region, words, lane, bits);
      __builtin_amdgcn_wave_barrier();  // the bitmap is reused by this wave's next unit
    }
    if (lane == 0) a.conf_counts[b] = left;
  }
}

__global__ __launch_bounds__(256) void scn_confirm_build_kernel(ScnConfirmArgs a) {
  extern __shared__ uint32_t smem[];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t words = (a.n + 31u) / 32u;
  uint32_t *const bits = smem + (size_t)wave * 2u * words;
  uint32_t *const below = bits + words;
  const uint32_t bin_step = a.sample_rate / a.n;  // process.cpp:39 (truncating)
  const uint32_t last = a.first + a.out_cap;      // exclusive (no wrap: checked by the caller)
  scn_hit *const out = static_cast<scn_hit *>(a.out);
  for (uint32_t b = blockIdx.x * 4u + wave; b < a.n_buffers; b += gridDim.x * 4u) {
    const uint32_t c0 = a.conf_offsets[b], c1 = a.conf_offsets[b + 1u];
    if (c1 == c0 || c0 >= last || c1 <= a.first) continue;  // nothing confirmed, or none of this unit's inside the window
    const ScnDevHit *const region = a.regions + (size_t)b * a.hit_region;
    const ScnDevHit first64 = region[lane < a.hit_region ? lane : 0u];
    const uint32_t c = a.offsets[b + 1u] - a.offsets[b], stored = c < a.hit_region ? c : a.hit_region;
    const double fc = scn_unit_centre(a, b);
    const uint64_t seq = scn_unit_seq(a, b);
    confirmed_bitmap(a, b, region, first64, stored, words, lane, bits);
    scn_wave_rank_prefix(bits, below, words, lane);
    scn_wave_write_ranked<true>(region, first64, stored, bits, below, c0, a.first, last, seq, fc, a.sample_rate, bin_step, out, lane);
    __builtin_amdgcn_wave_barrier();  // the bitmap is reused by this wave's next unit
  }
}

bool confirm_args_ok(const ScnConfirmArgs &a) {
  return a.n != 0 && a.n <= 65536u && a.rows != 0 && a.hist_first < a.rows && (uint64_t)a.hist_first + a.n_buffers <= 0xffffffffull && a.history &&
         a.regions && a.offsets && a.m >= 1u && a.m <= 32u;
}

template <class K>
hipError_t launch_confirm(K kernel, const ScnConfirmArgs &a, hipStream_t stream) {
  const uint32_t words = (a.n + 31u) / 32u;
  const size_t lds = (size_t)4u * 2u * words * sizeof(uint32_t);  // 4 waves x (bitmap + prefix), the compaction kernel's
  uint32_t blocks = (a.n_buffers + 3u) / 4u;
  if (blocks > 8192u) blocks = 8192u;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t scn_launch_history_fold(const ScnHistoryArgs &a, int num_cus, hipStream_t stream) {
  if (a.n_units == 0) return hipSuccess;
  if (a.n == 0 || a.n > 65536u || a.rows == 0 || a.first >= a.rows || a.n_units > a.rows || !a.history || !a.visits || !a.regions || !a.counts)
    return hipErrorInvalidValue;
  const bool vec = a.n % 4u == 0 && ((uintptr_t)a.history & 15u) == 0;
  return vec ? launch_fold_size<true>(a, num_cus, stream) : launch_fold_size<false>(a, num_cus, stream);
}

hipError_t scn_launch_confirm_count(const ScnConfirmArgs &a, hipStream_t stream) {
  if (a.n_buffers == 0) return hipSuccess;
  if (!confirm_args_ok(a) || !a.conf_counts) return hipErrorInvalidValue;
  return launch_confirm(scn_confirm_count_kernel, a, stream);
}

hipError_t scn_launch_confirm_build(const ScnConfirmArgs &a, hipStream_t stream) {
  if (a.n_buffers == 0 || a.out_cap == 0) return hipSuccess;
  if (!confirm_args_ok(a) || !a.conf_offsets || !a.out) return hipErrorInvalidValue;
  return launch_confirm(scn_confirm_build_kernel, a, stream);
}
