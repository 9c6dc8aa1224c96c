// scn_floor.hip -- the floor detector (scn_plan_desc.detect = SCN_DETECT_FLOOR; definition: scanner_hip.h, "Floor detector").
//
// One kernel behind the transform, on the dB spectrum the spectrum-only specialisations store: per unit (a buffer, or a group
// of an averaged plan) it selects the value of a given rank among the evaluated bins -- the unit's floor --, adds the plan's
// offset to it in one float addition and records every evaluated bin strictly above that cut, in the format the FFT kernels'
// own hit paths leave: {i, power_db} records in the unit's region, in any order, and the unit's count.  Scan, compaction,
// signals and gather read them unchanged.  No FFT kernel is touched (sharing code with them reschedules
// every instantiation).
//
// Selection: an MSB-first radix select on the keys `(bits & 0x80000000) ? ~bits : bits | 0x80000000` (unsigned order = float
// order, -inf lowest, -0.0 below +0.0).  Per pass: a histogram of the digit over the keys that match the prefix found so far,
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
// Geometry (a TEAM of T threads per unit, persistent: teams walk units with the grid's stride):
//   n <= 512          T = 64: a wave per unit, four units per 256-thread workgroup, wave barriers only
//   n <= 4096         T = 256, n <= 16384: T = 1024: a workgroup per unit
//   in all of these the unit's values stay in registers (KPT = ceil(n / T) <= 16 per thread): the spectrum is read ONCE.
//   n > 16384         T = 1024, the unit re-read from memory in every pass and in the hit pass (5 reads of 128 / 256 KiB,
//                     which L2 holds): the evaluated keys alone exceed what a workgroup can keep on chip.
// Hit pass: the hits-only kernels' slot grab -- a wave counts its hits over all its bins (ballots), takes that many slots of
// the unit's region with one LDS atomic, and its lanes store their records at ballot-prefix positions.  A region holds
// hit_region = M records, as many as there are evaluated bins: it cannot overflow, and the stores go through a buffer
// descriptor of exactly the region, as the loads go through one of exactly the unit's spectrum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scn_device.h"

namespace {

__device__ __forceinline__ uint32_t floor_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__device__ __forceinline__ uint32_t floor_unkey(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

template <int T>
__device__ __forceinline__ void team_sync() {
  if constexpr (T == 64) {  // a wave: its LDS operations complete in order
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

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
  constexpr int BLOCK = T == 64 ? 256 : T, TEAMS = BLOCK / T;
  __shared__ __attribute__((aligned(16))) uint32_t s_hist[TEAMS][4][256];  // one histogram per pass: zeroed once per unit
  __shared__ uint32_t s_count[TEAMS];
  const uint32_t t = threadIdx.x % T, team = threadIdx.x / T, lane = threadIdx.x & 63u;
  const uint32_t n = a.n, to_i = n - n / 2u;  // i = (j + n - n / 2) % n is the i with (i + n / 2) % n == j (process.cpp:47)
  const uint32_t trips = REREAD ? (n + T - 1u) / T : (uint32_t)KPT;
  uint32_t(*const hist)[256] = s_hist[team];
  uint32_t *const hist_all = &s_hist[team][0][0];  // the team's four histograms, 4 x 256 words in a row
  for (uint32_t u0 = blockIdx.x * TEAMS + team; u0 < a.n_units; u0 += gridDim.x * TEAMS) {
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)u0);  // (the same in every lane of a wave)
    const __amdgpu_buffer_rsrc_t rin = make_rsrc(a.power_db + (size_t)u * n, n * 4u);
    const __amdgpu_buffer_rsrc_t rhit = make_rsrc(a.hits + (size_t)u * a.hit_region, a.hit_region * (uint32_t)sizeof(ScnDevHit));
    // bin j = t + k T of the unit: its value's bits, and whether the mask lets it through
    auto load = [&](uint32_t k, uint32_t &bits, uint32_t &i) -> bool {
      const uint32_t j = t + k * T;
      bits = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rin, j * 4u, 0, 0);  // (j >= n: outside the descriptor, reads 0)
      i = j + to_i;
      i = i >= n ? i - n : i;
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
    uint32_t base = 0;
    if (total) {
      if (lane == 0) base = atomicAdd(&s_count[team], total);
      base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
      const unsigned long long below = (1ull << lane) - 1ull;
      auto record = [&](bool hit, uint32_t bits, uint32_t i) {
        const unsigned long long m = __ballot(hit);
        const uint32_t pos = base + (uint32_t)__popcll(m & below);
        typedef uint32_t u2 __attribute__((ext_vector_type(2)));
        // (a lane without a hit stores outside the descriptor: dropped)
        __builtin_amdgcn_raw_buffer_store_b64(u2{i, bits}, rhit, hit ? pos * (uint32_t)sizeof(ScnDevHit) : 0x80000000u, 0, 0);
        base += (uint32_t)__popcll(m);
      };
      if constexpr (REREAD) {
        for (uint32_t k = 0; k < trips; k++) {
          uint32_t bits, i;
          const bool ok = load(k, bits, i);
          record(ok && __uint_as_float(bits) > cut, bits, i);
        }
      } else {
#pragma unroll
        for (int k = 0; k < KPT; k++) {
          uint32_t i = t + (uint32_t)k * T + to_i;
          i = i >= n ? i - n : i;
          record(((valid >> k) & 1u) && __uint_as_float(val[k]) > cut, val[k], i);
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
  constexpr uint32_t block = T == 64 ? 256u : (uint32_t)T, teams = block / (uint32_t)T;
  // persistent teams: as many workgroups as the runtime says are resident at once for this instantiation's registers and LDS
  // (asked once per instantiation; at most 8 of 256 threads or 2 of 1024 per CU, the fallback should the query fail); no more
  // workgroups than there are units to walk.  The workgroups share nothing: the grid's size is a matter of speed only.
  static int per_cu = 0;  // (plans of several threads may race to the same answer)
  if (per_cu <= 0) {
    int q = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, scn_floor_kernel<T, KPT, REREAD>, (int)block, 0) != hipSuccess || q <= 0) {
      (void)hipGetLastError();
      q = block == 256u ? 8 : 2;
    }
    per_cu = q;
  }
  const uint32_t resident = (uint32_t)(num_cus > 0 ? num_cus : 256) * (uint32_t)per_cu;
  uint32_t blocks = (a.n_units + teams - 1u) / teams;
  if (blocks > resident) blocks = resident;
  hipLaunchKernelGGL((scn_floor_kernel<T, KPT, REREAD>), dim3(blocks), dim3(block), 0, stream, a);
  return hipGetLastError();
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
