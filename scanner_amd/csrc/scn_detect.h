// scn_detect.h -- what the detect kernels behind the transform share (scn_floor.hip, scn_floor_local.hip, scn_baseline.hip): the
// team model, the ordered key, the bin index maps, the per-unit descriptors, the hit pass and the launcher.  Internal; .hip files only.
//
// Team model: a TEAM of T threads works one unit (a buffer, or a group of an averaged plan) of the dB spectrum the spectrum-only
// transform stored:
//   T = 64            a wave per unit, four units per 256-thread workgroup, wave barriers only
//   T = 256, 1024     a workgroup per unit
// Teams are persistent: they walk units with the grid's stride, `for (u0 = blockIdx.x * TEAMS + team; u0 < n_units; u0 += gridDim.x *
// TEAMS)`, and the grid is capped at what is resident (launch_teams).  The workgroups share nothing.
// Hit pass: a wave counts its hits (ballots), takes that many slots of the unit's region with ONE LDS atomic on the team's counter
// (grab_slots) and its lanes store their {i, power_db} records at ballot-prefix positions (store_record) -- the format the FFT
// kernels' own hit paths leave, in any order; the team's counter ends as the unit's count.  A region holds hit_region = M records,
// as many as there are evaluated bins: it cannot overflow.  Loads and stores go through buffer descriptors of exactly the unit's
// spectrum and exactly its region: a load past the row reads 0, a store past the region is dropped.
// No FFT kernel includes this (sharing code with them reschedules every instantiation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "scn_device.h"

namespace {

// The team's geometry: t the thread's index in its team, team the team's in its workgroup, lane the thread's in its wave
template <int T>
struct Team {
  static_assert(T == 64 || T == 256 || T == 1024, "a wave, or a workgroup of 256 or 1024");
  static constexpr uint32_t BLOCK = T == 64 ? 256u : (uint32_t)T, TEAMS = BLOCK / (uint32_t)T;
  static __device__ __forceinline__ uint32_t t() { return threadIdx.x % T; }
  static __device__ __forceinline__ uint32_t team() { return threadIdx.x / T; }
  static __device__ __forceinline__ uint32_t lane() { return threadIdx.x & 63u; }
};

// The team's barrier
template <int T>
__device__ __forceinline__ void team_sync() {
  if constexpr (T == 64) {  // a wave: its LDS operations complete in order
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// The ordered key of a float's bits and its inverse: unsigned order = float order, -inf lowest, -0.0 below +0.0
__device__ __forceinline__ uint32_t floor_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__device__ __forceinline__ uint32_t floor_unkey(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

// Natural bin j < n -> fftshift index i, the i with (i + n / 2) % n == j (process.cpp:47): i = (j + to_i) % n, to_i = n - n / 2;
// and back, j = (i + half) % n, half = n / 2.  One conditional subtraction each.
__device__ __forceinline__ uint32_t shift_of_bin(uint32_t j, uint32_t to_i, uint32_t n) {
  const uint32_t i = j + to_i;
  return i >= n ? i - n : i;
}
__device__ __forceinline__ uint32_t bin_of_shift(uint32_t i, uint32_t half, uint32_t n) {
  const uint32_t j = i + half;
  return j >= n ? j - n : j;
}

// Unit u's descriptors: exactly its row of the spectrum, exactly its region of the records (`a`: any detector's argument struct)
template <class A>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t spectrum_rsrc(const A &a, uint32_t u) {
  return make_rsrc(a.power_db + (size_t)u * a.n, a.n * 4u);
}
template <class A>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t region_rsrc(const A &a, uint32_t u) {
  return make_rsrc(a.hits + (size_t)u * a.hit_region, a.hit_region * (uint32_t)sizeof(ScnDevHit));
}

// The wave's slot grab: `total` (wave-uniform, not 0) slots of the team's counter; the first of them, in every lane
__device__ __forceinline__ uint32_t grab_slots(uint32_t *count, uint32_t total, uint32_t lane) {
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(count, total);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
}

// One record per hit lane at the wave's next slots: m the ballot of `hit`, below = (1ull << lane) - 1 (the caller's, computed once
// outside its loops).  A lane without a hit stores at offset 0x80000000, outside the descriptor: dropped.  (The offset of a hit is
// formed for every lane and then selected: no branch.)
__device__ __forceinline__ void store_record(__amdgpu_buffer_rsrc_t rhit, uint32_t &base, unsigned long long m, bool hit, unsigned long long below,
                                             uint32_t i, uint32_t bits) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  const uint32_t rank = (uint32_t)__popcll(m & below);  // the hits in the lanes below this one
  const u2 record = {i, bits};
  const uint32_t offset = (base + rank) * (uint32_t)sizeof(ScnDevHit);
  __builtin_amdgcn_raw_buffer_store_b64(record, rhit, hit ? offset : 0x80000000u, 0, 0);
  base += (uint32_t)__popcll(m);
}

// The launch of persistent teams: as many workgroups as the runtime says are resident at once for this instantiation's registers
// and LDS (`fallback` per CU should the query fail), no more than there are units to walk (scn_team_grid, scn_mask.h).  The grid's
// size is a matter of speed only.  The runtime is asked once per instantiation: plans of several threads may race to the same
// answer, so the cache is a relaxed atomic -- both store the same value, neither reads a torn one.
template <auto KERNEL, uint32_t BLOCK, uint32_t TEAMS, class A>
hipError_t launch_teams(uint32_t lds_bytes, int fallback, const A &a, int num_cus, hipStream_t stream) {
  static std::atomic<int> cached;
  int per_cu = cached.load(std::memory_order_relaxed);
  if (per_cu <= 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERNEL, (int)BLOCK, lds_bytes) != hipSuccess || per_cu <= 0) {
      (void)hipGetLastError();
      per_cu = fallback;
    }
    cached.store(per_cu, std::memory_order_relaxed);
  }
  hipLaunchKernelGGL(KERNEL, dim3(scn_team_grid(a.n_units, TEAMS, num_cus, per_cu)), dim3(BLOCK), lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace
