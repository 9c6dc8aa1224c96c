// scn_floor_local.hip -- the floor detector with a floor window (scn_plan_set_floor_window; definition: scanner_hip.h, "Floor window").
//
// One kernel behind the transform, on the dB spectrum the spectrum-only specialisations store; its output: {i, power_db} records in
// the unit's region, in any order, and the unit's count.  Every bin has a floor of its own: the value of rank r_i among its reference
// cells, the evaluated bins guard < |i' - i| <= guard + train away in fftshift order.  The team model and the hit pass are scn_detect.h's.
//
// No selection is needed.  With the cells' values in key order v_(0) <= v_(1) <= ... and w_(k) = fl(v_(k) + threshold),
//     power_db[j] > fl(v_(r_i) + threshold)   <=>   #{cells c : fl(c + threshold) < power_db[j]} >= r_i + 1,
// because v -> fl(v + threshold) is non-decreasing along the key order (-0.0 and +0.0 differ in key but compare equal, which
// changes no comparison): if x > w_(r) then w_(0) ... w_(r) are all below x, r + 1 of them; and if r + 1 cells lie below x, one of
// them has a rank k >= r, so w_(r) <= w_(k) < x.  Integer counts and float compares only: no atomics on floats, no float sums --
// the hit set is the same whatever order the waves run in.
// The argument holds for cells that are not NaN.  A NaN cell counts as below nothing here, whatever its sign -- fl(NaN + threshold)
// is below no x --, while the key puts a NaN with its sign bit set under every value: for a window that mixed such cells with finite
// ones the count and a rank taken in key order would differ, and the count is the definition (scanner_hip.h, "Floor window";
// tests/local_floor_ref.py, hit_bins_by_count).  No transform here stores such a mix: a NaN sample makes its whole unit NaN
// (tests/test_plan_sequences_gpu.py asserts it of every NaN unit it submits), and a unit that is all NaN has no hits either way.
// r_i + 1 depends on (n, mask, train, guard, permille) alone: the host makes the table need[i] once per window (floor_window_ranks,
// scn_host.hip: M_i from the mask, never from the values), 0 for a bin the mask removes, and the kernel reads 2 bytes per bin of it.
//
// Sizes: n <= 512: T = 64, n <= 4096: T = 256, above: T = 1024.
// Per unit and TILE of CAP = 4 T RUNS consecutive fftshift indices (one tile up to 16384 points, four at 65536), the team stages
//   w[i] = evaluated ? fl(power_db + threshold) : +inf      (+inf is below nothing: a bin that is not a cell counts for nothing)
// into LDS in fftshift order, with a halo of 192 = SCN_FLOOR_TRAIN_MAX + SCN_FLOOR_GUARD_MAX slots on either side -- the
// neighbouring tiles' bins, re-read from L2, or +inf beyond the band's edges: there is no wrap.  A thread owns RUNS runs of 4
// consecutive bins, run r at 4 (r T + t): it keeps their raw values in registers from the staging loads (for the compare and the
// record), its LDS stores and loads are 16 bytes at 16-byte lane stride (full rate, no bank conflict), and the windows of the four
// bins of a run share their reads: a 16-byte chunk of cells is read once and held against all four.  Whether cell e of chunk q
// belongs to bin k's window depends on 4 q + e - k, guard and train only -- the same in every lane, so the membership tests are
// scalar, and a chunk that lies inside all four windows (most of them once train >= 8) takes 16 compare-and-count pairs straight.
// One slot grab per wave and tile; the table is read through a descriptor of exactly its length, as the spectrum is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/scanner_hip.h"
#include "scn_detect.h"

namespace {

constexpr uint32_t kHalo = SCN_FLOOR_TRAIN_MAX + SCN_FLOOR_GUARD_MAX;  // slots on either side of a tile (a multiple of 4)
typedef float f4 __attribute__((ext_vector_type(4)));

template <int T, int RUNS>
struct LocalGeo : Team<T> {
  using Team<T>::TEAMS;
  static constexpr uint32_t CAP = 4u * (uint32_t)T * (uint32_t)RUNS;  // bins per tile
  static constexpr uint32_t SLOTS = CAP + 2u * kHalo;                 // floats of LDS per team
  static constexpr uint32_t LDS_BYTES = TEAMS * SLOTS * 4u + TEAMS * 4u;
};

template <int T, int RUNS>
__global__ __launch_bounds__(T == 64 ? 256 : T) void scn_floor_local_kernel(ScnFloorLocalArgs a) {
  typedef LocalGeo<T, RUNS> G;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const uint32_t t = G::t(), team = G::team(), lane = G::lane();
  float *const s_w = reinterpret_cast<float *>(smem_raw) + team * G::SLOTS + kHalo;  // s_w[il]: the tile's bin il, -kHalo <= il < CAP + kHalo
  uint32_t *const s_count = reinterpret_cast<uint32_t *>(smem_raw + G::TEAMS * G::SLOTS * 4u) + team;
  const uint32_t n = a.n, half = n / 2u;
  const int guard = (int)a.guard, train = (int)a.train, reach = guard + train;
  const float inf = __builtin_inff();
  const __amdgpu_buffer_rsrc_t rneed = make_rsrc(a.need, ((n + 3u) & ~3u) * 2u);
  for (uint32_t u0 = blockIdx.x * G::TEAMS + team; u0 < a.n_units; u0 += gridDim.x * G::TEAMS) {
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)u0);  // (the same in every lane of a wave)
    const __amdgpu_buffer_rsrc_t rin = spectrum_rsrc(a, u), rhit = region_rsrc(a, u);
    // the bin at fftshift index i (which may lie outside the band): its value's bits, and whether it is a cell
    auto cell = [&](int i, uint32_t &bits) -> bool {
      const bool inside = (uint32_t)i < n;
      const uint32_t j = bin_of_shift(inside ? (uint32_t)i : 0u, half, n);
      bits = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rin, j * 4u, 0, 0);
      return inside && scn_bin_evaluated(j, (uint32_t)i, n, a);
    };
    if (t == 0) *s_count = 0u;
    for (uint32_t tile0 = 0; tile0 < n; tile0 += G::CAP) {
      uint32_t x[RUNS][4];
#pragma unroll
      for (int r = 0; r < RUNS; r++) {
        const uint32_t il0 = 4u * ((uint32_t)r * T + t);
        f4 w;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const bool ok = cell((int)(tile0 + il0) + e, x[r][e]);
          w[e] = ok ? __uint_as_float(x[r][e]) + a.threshold : inf;
        }
        *reinterpret_cast<f4 *>(s_w + il0) = w;
      }
      for (uint32_t h = t; h < 2u * kHalo; h += T) {
        const int il = h < kHalo ? (int)h - (int)kHalo : (int)(G::CAP + h - kHalo);
        uint32_t bits;
        const bool ok = cell((int)tile0 + il, bits);
        s_w[il] = ok ? __uint_as_float(bits) + a.threshold : inf;
      }
      team_sync<T>();
      uint32_t hm = 0;  // bit 4 r + k: bin k of run r is a hit
#pragma unroll
      for (int r = 0; r < RUNS; r++) {
        const uint32_t il0 = 4u * ((uint32_t)r * T + t);
        typedef uint32_t u2 __attribute__((ext_vector_type(2)));
        // (beyond the table -- the band's end inside the last tile -- the descriptor returns 0: not evaluated)
        const u2 nd = __builtin_bit_cast(u2, __builtin_amdgcn_raw_buffer_load_b64(rneed, (tile0 + il0) * 2u, 0, 0));
        if (!__ballot((nd.x | nd.y) != 0u)) continue;  // a wave whose runs the mask removes altogether (outside the band)
        const uint32_t need[4] = {nd.x & 0xffffu, nd.x >> 16, nd.y & 0xffffu, nd.y >> 16};
        const float xf[4] = {__uint_as_float(x[r][0]), __uint_as_float(x[r][1]), __uint_as_float(x[r][2]), __uint_as_float(x[r][3])};
        uint32_t cnt[4] = {0u, 0u, 0u, 0u};
        const float *const base = s_w + il0;
        // chunk q: the four cells 4 q ... 4 q + 3 bins from the run's first bin; cell e lies d = 4 q + e - k from bin k
        auto chunk = [&](int q) {
          const f4 w = *reinterpret_cast<const f4 *>(base + 4 * q);
          const int lo = 4 * q - 3, hi = 4 * q + 3;
          if ((hi < -guard && lo >= -reach) || (lo > guard && hi <= reach)) {  // inside all four windows
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
              for (int k = 0; k < 4; k++) cnt[k] += w[e] < xf[k] ? 1u : 0u;
          } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
              for (int k = 0; k < 4; k++) {
                const int d = 4 * q + e - k, ad = d < 0 ? -d : d;
                const bool in = (uint32_t)(ad - guard - 1) < (uint32_t)train;  // guard < |d| <= guard + train
                cnt[k] += (in && w[e] < xf[k]) ? 1u : 0u;
              }
          }
        };
        // the windows below the run reach from -reach to 2 - guard, those above it from guard + 1 to 3 + reach
        const int l0 = (-reach) >> 2, l1 = (2 - guard) >> 2, r0 = (guard + 1) >> 2, r1 = (3 + reach) >> 2;
        for (int q = l0; q <= l1; q++) chunk(q);
        for (int q = r0 > l1 ? r0 : l1 + 1; q <= r1; q++) chunk(q);
#pragma unroll
        for (int k = 0; k < 4; k++) hm |= (need[k] != 0u && cnt[k] >= need[k]) ? 1u << (4 * r + k) : 0u;
      }
      // the hit pass: the wave's total first, one slot grab, then the records at ballot-prefix positions
      uint32_t total = 0;
#pragma unroll
      for (int b = 0; b < 4 * RUNS; b++) total += (uint32_t)__popcll(__ballot((hm >> b) & 1u));
      if (total) {
        uint32_t slot = grab_slots(s_count, total, lane);
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int b = 0; b < 4 * RUNS; b++) {
          const bool hit = (hm >> b) & 1u;
          const uint32_t i = tile0 + 4u * ((uint32_t)(b / 4) * T + t) + (uint32_t)(b % 4);
          store_record(rhit, slot, __ballot(hit), hit, below, i, x[b / 4][b % 4]);
        }
      }
      team_sync<T>();  // every wave is done with the tile's cells, and its grab is in s_count
    }
    if (t == 0) a.counts[u] = *s_count;
    team_sync<T>();  // (s_count is zeroed again for the team's next unit)
  }
}

template <int T, int RUNS>
hipError_t launch(const ScnFloorLocalArgs &a, int num_cus, hipStream_t stream) {
  typedef LocalGeo<T, RUNS> G;
  if (G::LDS_BYTES > 65536u) {  // the opt-in for more than 64 KiB of dynamic LDS: per function and per device, so set on every launch
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(scn_floor_local_kernel<T, RUNS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)G::LDS_BYTES);
    if (e != hipSuccess) return e;
  }
  // (the fallback: what the LDS alone allows, at most 8 workgroups of 256 threads or 2 of 1024 per CU)
  const int fallback = (int)std::min<uint32_t>(G::BLOCK == 256u ? 8u : 2u, std::max<uint32_t>(1u, 163840u / G::LDS_BYTES));
  return launch_teams<scn_floor_local_kernel<T, RUNS>, G::BLOCK, G::TEAMS>(G::LDS_BYTES, fallback, a, num_cus, stream);
}

}  // namespace

hipError_t scn_launch_floor_local(const ScnFloorLocalArgs &a, int num_cus, hipStream_t stream) {
  if (a.n_units == 0) return hipSuccess;
  if (a.n == 0 || a.n > 65536u || a.hit_region == 0 || a.train == 0 || a.train > SCN_FLOOR_TRAIN_MAX || a.guard > SCN_FLOOR_GUARD_MAX ||
      !a.power_db || !a.hits || !a.counts || !a.need)
    return hipErrorInvalidValue;
  const uint32_t n = a.n;
  if (n <= 256u) return launch<64, 1>(a, num_cus, stream);
  if (n <= 512u) return launch<64, 2>(a, num_cus, stream);
  if (n <= 1024u) return launch<256, 1>(a, num_cus, stream);
  if (n <= 4096u) return launch<256, 4>(a, num_cus, stream);
  if (n <= 8192u) return launch<1024, 2>(a, num_cus, stream);
  return launch<1024, 4>(a, num_cus, stream);  // (one tile up to 16384 points, ceil(n / 16384) above)
}
