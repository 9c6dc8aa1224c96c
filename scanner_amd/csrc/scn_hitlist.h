// scn_hitlist.h -- what the kernels that rank a unit's records by bin share: the compaction of the ordered hit list (scn_hits.hip)
// and the confirmed list of a plan with a hit history (scn_history.hip).  One WAVE per unit; the unit's hit bitmap and the set bits
// before each of its words lie in the wave's LDS; a record's place in the unit is the number of set bits below its bin.  The
// completed public record {seq_id, i, power_db, freq_hz} is written by ONE function, so that every list made from a unit's region
// carries the same bits.  Internal; .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/scanner_hip.h"
#include "scn_kernels.h"

namespace {

// uint64_t(double) the way the reference's x86-64 build does it (process.cpp:57 casts a double that is negative for the
// lowest bins of a sweep starting at 0 Hz: cvttsd2si gives the two's complement of the magnitude, not 0)
__device__ __forceinline__ uint64_t to_u64_like_x86(double f) {
  return f < 0.0 ? (uint64_t)(int64_t)f : (uint64_t)f;
}

// bits[0, words) = the unit's hit bitmap, from the first `stored` records of its region in whatever order they lie (bins are
// distinct within a unit).  first64: the lane's speculative load of record `lane` (the caller issued it with the unit's other loads)
__device__ __forceinline__ void scn_wave_hit_bitmap(const ScnDevHit *region, const ScnDevHit &first64, uint32_t stored, uint32_t words, uint32_t lane,
                                                    uint32_t *bits) {
  for (uint32_t w = lane; w < words; w += 64u) bits[w] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (uint32_t k = lane; k < stored; k += 64u) {
    const uint32_t i = k < 64u ? first64.i : region[k].i;
    atomicOr(&bits[i >> 5], 1u << (i & 31u));
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// below[w] = set bits in the words before word w: lane l sums its words [l*per_lane, (l+1)*per_lane), exclusive scan over the
// lanes, then fills in.  Returns the bitmap's number of set bits, in every lane.
__device__ __forceinline__ uint32_t scn_wave_rank_prefix(const uint32_t *bits, uint32_t *below, uint32_t words, uint32_t lane) {
  const uint32_t per_lane = (words + 63u) / 64u;  // contiguous words a lane sums
  uint32_t mine = 0;
  for (uint32_t k = 0; k < per_lane; k++) {
    const uint32_t w = lane * per_lane + k;
    if (w < words) mine += (uint32_t)__popc(bits[w]);
  }
  uint32_t incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = __shfl_up(incl, off, 64);
    if (lane >= (uint32_t)off) incl += v;
  }
  uint32_t run = incl - mine;
  for (uint32_t k = 0; k < per_lane; k++) {
    const uint32_t w = lane * per_lane + k;
    if (w < words) {
      below[w] = run;
      run += (uint32_t)__popc(bits[w]);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return (uint32_t)__shfl(incl, 63, 64);
}

// The unit's records ranked by the bitmap and written, completed, to the window [first, last) of a list in which the unit's
// first record has position o0.  SUBSET: the bitmap may have lost bits since it was made from the region (the confirmed list);
// a record whose bit is clear is not part of the list.  Without it every record's bit is set and nothing is tested.
template <bool SUBSET>
__device__ __forceinline__ void scn_wave_write_ranked(const ScnDevHit *region, const ScnDevHit &first64, uint32_t stored, const uint32_t *bits,
                                                      const uint32_t *below, uint32_t o0, uint32_t first, uint32_t last, uint64_t seq, double fc,
                                                      uint32_t sample_rate, uint32_t bin_step, scn_hit *out, uint32_t lane) {
  const double start_frequency = fc - (double)(sample_rate / 2u);  // process.cpp:38 (uint32 division)
  for (uint32_t k = lane; k < stored; k += 64u) {
    const ScnDevHit h = k < 64u ? first64 : region[k];
    const uint32_t w = h.i >> 5;
    if (SUBSET && !((bits[w] >> (h.i & 31u)) & 1u)) continue;
    const uint32_t pos = o0 + below[w] + (uint32_t)__popc(bits[w] & ((1u << (h.i & 31u)) - 1u));
    if (pos >= first && pos < last) {
      const double frequency = start_frequency + (double)(uint32_t)(h.i * bin_step);  // process.cpp:55
      scn_hit r;
      r.seq_id = seq;
      r.i = h.i;
      r.power_db = h.power_db;
      r.freq_hz = to_u64_like_x86(frequency);  // process.cpp:57
      out[pos - first] = r;
    }
  }
}

// The header fields of unit b's records, from where the submit left them (`a`: ScnCompactArgs, ScnSignalArgs, ScnConfirmArgs)
template <class A>
__device__ __forceinline__ double scn_unit_centre(const A &a, uint32_t b) {
  return a.center_freq[a.table_count ? (uint32_t)(((uint64_t)a.table_first + b) % a.table_count) : b];
}
template <class A>
__device__ __forceinline__ uint64_t scn_unit_seq(const A &a, uint32_t b) {
  return a.seq_id ? a.seq_id[b] : (uint64_t)b;  // (no ids given at submit: a buffer's id is its index, messageQueue.h:86 from zero)
}

}  // namespace
