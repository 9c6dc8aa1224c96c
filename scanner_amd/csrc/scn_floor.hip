// scn_floor.hip -- the floor detector (scn_plan_desc.detect = SCN_DETECT_FLOOR; definition: scanner_hip.h, "Floor detector").
//
// One kernel behind the transform, on the dB spectrum the spectrum-only specialisations store: per unit (a buffer, or a group
// of an averaged plan) it selects the value of a given rank among the evaluated bins -- the unit's floor --, adds the plan's
// offset to it in one float addition and records every evaluated bin strictly above that cut, in the format the FFT kernels'
// own hit paths leave: {i, power_db} records in the unit's region, in any order, and the unit's count.  Scan, compaction,
// signals and gather read them unchanged.  The team model and the hit pass are scn_detect.h's.
//
// Selection: an MSB-first radix select on the ordered keys (floor_key, scn_detect.h: unsigned order = float order, -inf lowest,
// -0.0 below +0.0).  Per pass: a histogram of the digit over the keys that match the prefix found so far,
// built in LDS with integer atomics; every wave scans it (4 entries per lane, one 16-byte read, a shuffle scan) and picks the
// digit that holds the rank.  Integer counts only: no global atomics, no float atomics, no float sums -- the floor, the cut and
// the hit set are the same whatever order the waves run in.
// Digits are 8 bits, 4 passes (not 11/11/10 in 3): a 256-entry histogram is 1 KiB, so each of the four waves of a small-unit
// workgroup owns its set, the scan is one 16-byte read per lane of ONE wave with no second level, and while the keys sit in
// registers a pass is ~KPT VALU operations and LDS atomics -- the fourth pass costs less than the 8 KiB histograms and the
// two-level scan of 2048 entries would.  Only the re-read route pays a real price for it: one more read of the unit from L2.
// dB values of one spectrum share their sign and exponent bits, so in the first pass nearly every lane of a wave holds the same
// digit: the lanes with the leading lane's digit add their number with ONE atomic (up to three such rounds), the rest singly
// -- 64 same-address LDS atomics would serialise.
//
// Sizes: n <= 512: T = 64, n <= 4096: T = 256, n <= 16384: T = 1024, and in all of these the unit's values stay in registers
// (KPT = ceil(n / T) <= 16 per thread): the spectrum is read ONCE.  n > 16384: T = 1024, the unit re-read from memory in every pass
// and in the hit pass (5 reads of 128 / 256 KiB, which L2 holds): the evaluated keys alone exceed what a workgroup can keep on chip.
// The wave counts its hits over all its bins before its one slot grab.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scn_detect.h"

namespace {

// hist[digit] += 1 for the active lanes (called by whole waves)
__device__ __forceinline__ void hist_add(uint32_t *hist, bool active, uint32_t digit, uint32_t lane) {
#pragma unroll
  for (int round = 0; round < 3; round++) {
    const unsigned long long m = __ballot(active);
    if (!m) return;
    const uint32_t lead = (uint32_t)__builtin_ctzll(m);
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)digit, (int)lead);  // (lead is wave-uniform: no LDS round trip)
    const bool same = active && digit == d0;
    const unsigned long long sm = __ballot(same);
    if (lane == lead) atomicAdd(&hist[d0], (uint32_t)__popcll(sm));
    active = active && !same;
  }
  if (active) atomicAdd(&hist[digit], 1u);
}

// The digit whose keys hold rank r of the histogrammed keys (in every lane of the calling wave); r becomes the rank among them.
__device__ __forceinline__ uint32_t pick_digit(const uint32_t *hist, uint32_t &r, uint32_t lane) {
  const uint4 h = *reinterpret_cast<const uint4 *>(hist + 4u * lane);
  const uint32_t s = h.x + h.y + h.z + h.w;
  uint32_t incl = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
    if (lane >= (uint32_t)off) incl += v;
  }
  const unsigned long long m = __ballot(incl > r);
  const int l = m ? __builtin_ctzll(m) : 63;  // (m != 0: the rank is below the number of keys)
  uint32_t before = (uint32_t)__shfl((int)(incl - s), l, 64);
  const uint32_t hx = (uint32_t)__shfl((int)h.x, l, 64), hy = (uint32_t)__shfl((int)h.y, l, 64), hz = (uint32_t)__shfl((int)h.z, l, 64);
  uint32_t d = 4u * (uint32_t)l;
  if (r >= before + hx) {
    before += hx;
    d++;
    if (r >= before + hy) {
      before += hy;
      d++;
      if (r >= before + hz) {
        before += hz;
        d++;
      }
    }
  }
  r -= before;
  return d;
}

template <int T, int KPT, bool REREAD>
__global__ __launch_bounds__(T == 64 ? 256 : T) void scn_floor_kernel(ScnFloorArgs a) {
  typedef Team<T> G;
  constexpr uint32_t TEAMS = G::TEAMS;
  __shared__ __attribute__((aligned(16))) uint32_t s_hist[TEAMS][4][256];  // one histogram per pass: zeroed once per unit
  __shared__ uint32_t s_count[TEAMS];
  const uint32_t t = G::t(), team = G::team(), lane = G::lane();
  const uint32_t n = a.n, to_i = n - n / 2u;
  const uint32_t trips = REREAD ? (n + T - 1u) / T : (uint32_t)KPT;
  uint32_t(*const hist)[256] = s_hist[team];
  uint32_t *const hist_all = &s_hist[team][0][0];  // the team's four histograms, 4 x 256 words in a row
  for (uint32_t u0 = blockIdx.x * TEAMS + team; u0 < a.n_units; u0 += gridDim.x * TEAMS) {
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)u0);  // (the same in every lane of a wave)
    const __amdgpu_buffer_rsrc_t rin = spectrum_rsrc(a, u), rhit = region_rsrc(a, u);
    // bin j = t + k T of the unit: its value's bits, and whether the mask lets it through
    auto load = [&](uint32_t k, uint32_t &bits, uint32_t &i) -> bool {
      const uint32_t j = t + k * T;
      bits = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rin, j * 4u, 0, 0);  // (j >= n: outside the descriptor, reads 0)
      i = shift_of_bin(j, to_i, n);
      return j < n && scn_bin_evaluated(j, i, n, a);
    };
    uint32_t val[REREAD ? 1 : KPT];
    uint32_t valid = 0;
    (void)val;
    if constexpr (!REREAD) {
#pragma unroll
      for (int k = 0; k < KPT; k++) {
        uint32_t i;
        valid |= load((uint32_t)k, val[k], i) ? 1u << k : 0u;
      }
    }
    for (uint32_t w = t; w < 4u * 256u; w += T) hist_all[w] = 0u;
    if (t == 0) s_count[team] = 0u;
    team_sync<T>();
    uint32_t prefix = 0, mask = 0, r = a.rank;
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
      const uint32_t shift = 24u - 8u * (uint32_t)pass;
      if constexpr (REREAD) {
        for (uint32_t k = 0; k < trips; k++) {
          uint32_t bits, i;
          const bool ok = load(k, bits, i);
          const uint32_t key = floor_key(bits);
          hist_add(hist[pass], ok && (key & mask) == prefix, (key >> shift) & 255u, lane);
        }
      } else {
#pragma unroll
        for (int k = 0; k < KPT; k++) {
          const uint32_t key = floor_key(val[k]);
          hist_add(hist[pass], ((valid >> k) & 1u) && (key & mask) == prefix, (key >> shift) & 255u, lane);
        }
      }
      team_sync<T>();
      prefix |= pick_digit(hist[pass], r, lane) << shift;
      mask |= 255u << shift;
    }
    const float floor_db = __uint_as_float(floor_unkey(prefix));
    const float cut = floor_db + a.threshold;
    // the hit pass: the wave's total first, one slot grab, then the records at ballot-prefix positions
    uint32_t total = 0;
    if constexpr (REREAD) {
      for (uint32_t k = 0; k < trips; k++) {
        uint32_t bits, i;
        const bool ok = load(k, bits, i);
        total += (uint32_t)__popcll(__ballot(ok && __uint_as_float(bits) > cut));
      }
    } else {
#pragma unroll
      for (int k = 0; k < KPT; k++) total += (uint32_t)__popcll(__ballot(((valid >> k) & 1u) && __uint_as_float(val[k]) > cut));
    }
    if (total) {
      uint32_t base = grab_slots(&s_count[team], total, lane);
      const unsigned long long below = (1ull << lane) - 1ull;
      if constexpr (REREAD) {
        for (uint32_t k = 0; k < trips; k++) {
          uint32_t bits, i;
          const bool hit = load(k, bits, i) && __uint_as_float(bits) > cut;
          store_record(rhit, base, __ballot(hit), hit, below, i, bits);
        }
      } else {
#pragma unroll
        for (int k = 0; k < KPT; k++) {
          const bool hit = ((valid >> k) & 1u) && __uint_as_float(val[k]) > cut;
          store_record(rhit, base, __ballot(hit), hit, below, shift_of_bin(t + (uint32_t)k * T, to_i, n), val[k]);
        }
      }
    }
    team_sync<T>();  // every wave's grab is in s_count, every wave is done with the histograms
    if (t == 0) {
      a.counts[u] = s_count[team];
      a.floor_db[u] = floor_db;
    }
    team_sync<T>();  // (s_count is zeroed again for the team's next unit)
  }
}

template <int T, int KPT, bool REREAD>
hipError_t launch(const ScnFloorArgs &a, int num_cus, hipStream_t stream) {
  typedef Team<T> G;  // (the fallback: 8 workgroups of 256 threads or 2 of 1024 per CU)
  return launch_teams<scn_floor_kernel<T, KPT, REREAD>, G::BLOCK, G::TEAMS>(0, G::BLOCK == 256u ? 8 : 2, a, num_cus, stream);
}

}  // namespace

hipError_t scn_launch_floor(const ScnFloorArgs &a, int num_cus, hipStream_t stream) {
  if (a.n_units == 0) return hipSuccess;
  if (a.n == 0 || a.n > 65536u || a.hit_region == 0 || a.rank >= a.hit_region || !a.power_db || !a.hits || !a.counts || !a.floor_db)
    return hipErrorInvalidValue;
  const uint32_t n = a.n;
  if (n <= 128u) return launch<64, 2, false>(a, num_cus, stream);
  if (n <= 512u) return launch<64, 8, false>(a, num_cus, stream);
  if (n <= 1024u) return launch<256, 4, false>(a, num_cus, stream);
  if (n <= 4096u) return launch<256, 16, false>(a, num_cus, stream);
  if (n <= 8192u) return launch<1024, 8, false>(a, num_cus, stream);
  if (n <= 16384u) return launch<1024, 16, false>(a, num_cus, stream);
  return launch<1024, 1, true>(a, num_cus, stream);
}
