// scn_plan.hip -- a plan's lifecycle: what it is made from (the path, the tables), what a slot allocates at its first use, its
// end (the members release themselves, scn_resource.h), and the getters.
#include <algorithm>
#include <cstring>
#include <new>

#include "scn_plan.h"

namespace {

Path path_of(uint32_t mode, uint32_t n) {
  if (mode == SCN_MODE_TIME_DOMAIN) return Path::TimeDomain;
  if (scn_fft_size_supported(n)) return Path::FusedPow2;    // scn_kernels.hip: the powers of two 16 ... 16384
  if (scn_mixed_size_supported(n)) return Path::FusedMixed;  // scn_mixed.hip: the sizes 2^a 3^b 5^c of scn_mixed_plans.h
  if (scn_big_size_supported(n)) return Path::FourStep;      // scn_big.hip: 32768, 65536
  if (scn_bluestein_size_supported(n)) return Path::Bluestein;  // scn_generic.hip: every other size from 16 to 65535
  return Path::Unsupported;
}

// The window and the tables the plan's path reads (a time-domain plan reads none)
hipError_t build_tables(scn_plan *p) {
  const uint32_t n = p->d.n;
  hipError_t e;
  if (p->path == Path::TimeDomain) return hipSuccess;
  if ((e = upload(p->d_window, p->h_window)) != hipSuccess) return e;
  switch (p->path) {
    case Path::FusedPow2:
    case Path::FusedMixed: {
      const std::vector<float> tw = twiddles<float>(n);
      // the same values, regrouped per thread of the fused kernel: entry (p-1, t) = W_n^(t p)
      uint32_t rows, threads;
      if (p->path == Path::FusedMixed) scn_mixed_layout(n, &rows, &threads);
      else scn_tw1_layout(n, &rows, &threads);
      std::vector<float> tw1(2 * (size_t)rows * threads);
      for (uint32_t pp = 1; pp <= rows; pp++)
        for (uint32_t t = 0; t < threads; t++) {
          const uint32_t m = (uint32_t)(((uint64_t)t * pp) % n);
          tw1[2 * ((size_t)(pp - 1) * threads + t)] = tw[2 * m];
          tw1[2 * ((size_t)(pp - 1) * threads + t) + 1] = tw[2 * m + 1];
        }
      if ((e = upload(p->d_twiddle, tw)) != hipSuccess) return e;
      if (p->avg > 1u && n == 8192) {  // the averaged kernel's two 4096-point halves and the radix-2 step that joins them
        std::vector<float> half(2 * 15 * 256);
        for (uint32_t pp = 1; pp <= 15; pp++)
          for (uint32_t t = 0; t < 256; t++) {
            const uint32_t m = (2u * t * pp) % n;  // W_4096^(t p) = W_8192^(2 t p)
            half[2 * ((pp - 1) * 256 + t)] = tw[2 * m];
            half[2 * ((pp - 1) * 256 + t) + 1] = tw[2 * m + 1];
          }
        std::vector<double> join = twiddles<double>(n);
        join.resize(n);  // k < 4096
        if ((e = upload(p->d_avg_tw1, half)) != hipSuccess || (e = upload(p->d_avg_tw, join)) != hipSuccess) return e;
      }
      return upload(p->d_tw1_table, tw1);
    }
    case Path::FourStep:  // W_n in float; W_256 in double: the row transform of scn_big.hip
      if ((e = upload(p->d_twiddle, twiddles<float>(n))) != hipSuccess) return e;
      return upload(p->d_twiddle64, twiddles<double>(256));
    case Path::Bluestein: {
      const ScnBluesteinTables t = bluestein_tables(n);
      p->fft_m = t.m;
      p->log2m = t.log2m;
      if ((e = upload(p->d_twiddle64, t.twiddle)) != hipSuccess || (e = upload(p->d_chirp, t.chirp)) != hipSuccess) return e;
      return upload(p->d_bfilter, t.bfilter);
    }
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

int check_slot(scn_plan *p, int slot) {
  if (!p) return scn_fail(SCN_E_INVALID, "null plan");
  if (slot < 0 || slot >= SCN_NUM_SLOTS) return scn_fail(SCN_E_INVALID, "slot %d out of range", slot);
  return SCN_OK;
}

// SCN_PLAN_OVERLAP_SLOTS: the streams of slots 2 and 3 exist from their first use on
int ensure_slot_stream(scn_plan *p, Slot &s) {
  if (s.own_stream && !s.stream) {
    SCN_HIP(hipSetDevice(p->d.device_id));
    SCN_HIP(s.owned_stream.create());
    s.stream = s.owned_stream.get();
  }
  return SCN_OK;
}

// `gen`: the generation of hit regions / counts the coming submit writes (allocated when first used: a plan that only ever
// drives one slot, or submits once per slot, holds one or two of the four region sets -- 201 MB each for the C2 plan)
int ensure_slot_outputs(scn_plan *p, Slot &s, uint32_t gen) {
  SCN_HIP(s.done.create());
  if (p->d.mode == SCN_MODE_TIME_DOMAIN) {
    SCN_HIP(s.h_td.alloc(2 * (size_t)p->d.max_batch));
    return SCN_OK;
  }
  if (p->d.flags & SCN_OUT_HITS) {
    // every resource under its own check: a failed allocation leaves a state the next call completes or fails on again
    const size_t mb = p->d.max_batch;
    SlotGen &g = s.gen_state[gen & 1u];
    SCN_HIP(g.d_hits.alloc(p->hit_region * mb));
    SCN_HIP(g.d_buf_hits.alloc(mb));
    SCN_HIP(g.list_done.create());
    if (!s.h_buf_hits) {
      SCN_HIP(s.h_buf_hits.alloc(mb + 4u));
      s.h_total = reinterpret_cast<unsigned long long *>(s.h_buf_hits.get() + ((mb + 1u) & ~(size_t)1u));
    }
    if (!s.d_total_acc) {
      SCN_HIP(s.d_total_acc.alloc(2));
      SCN_HIP(hipMemset(s.d_total_acc.get(), 0, 2u * sizeof(unsigned long long)));
    }
    SCN_HIP(s.d_offsets.alloc(mb + 1u));
    SCN_HIP(s.h_meta.alloc(2u * 2u * mb));
    SCN_HIP(s.d_list.alloc(p->d.max_hits));
    SCN_HIP(s.h_list.alloc(p->d.max_hits));
    SCN_HIP(s.kernel_done.create());
    if (p->floor) {
      SCN_HIP(s.d_floor.alloc(mb));
      SCN_HIP(s.h_floor.alloc(mb));
    }
  }
  return SCN_OK;
}

extern "C" {

int scn_device_count(int *count) {
  if (!count) return scn_fail(SCN_E_INVALID, "null argument");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    *count = 0;
    return scn_fail(SCN_E_NO_DEVICE, "no HIP device visible");
  }
  *count = n;
  return SCN_OK;
}

int scn_size_path(uint32_t n, uint32_t *path) {
  if (!path) return scn_fail(SCN_E_INVALID, "null argument");
  switch (path_of(SCN_MODE_FREQUENCY_DOMAIN, n)) {
    case Path::FusedPow2:
    case Path::FusedMixed: *path = SCN_PATH_FUSED; break;
    case Path::FourStep: *path = SCN_PATH_FOUR_STEP; break;
    case Path::Bluestein: *path = SCN_PATH_BLUESTEIN; break;
    default: *path = SCN_PATH_UNSUPPORTED;
  }
  return SCN_OK;
}

int scn_plan_create(const scn_plan_desc *desc, scn_plan **out) {
  if (!desc || !out) return scn_fail(SCN_E_INVALID, "null argument");
  *out = nullptr;
  if (desc->struct_size != sizeof(scn_plan_desc))
    return scn_fail(SCN_E_INVALID, "scn_plan_desc.struct_size %u != %zu (ABI mismatch)", desc->struct_size,
                sizeof(scn_plan_desc));
  scn_plan_desc d = *desc;
  if (!d.window_type) d.window_type = SCN_WIN_BLACKMAN_HARRIS;
  if (!d.mode) d.mode = SCN_MODE_FREQUENCY_DOMAIN;
  if (!d.dc_ignore_bins) d.dc_ignore_bins = 4;  // process.cpp:87
  if (d.dc_ignore_bins == SCN_DC_IGNORE_NONE) d.dc_ignore_bins = 0;
  if (d.use_bandwidth == 0.0) d.use_bandwidth = 0.75;  // scan.cpp:65
  if (!d.trigger_count) d.trigger_count = 1047;        // process.cpp:62
  if (!(d.flags & (SCN_OUT_SPECTRUM | SCN_OUT_HITS))) d.flags |= SCN_OUT_SPECTRUM | SCN_OUT_HITS;
  if (!d.max_batch) return scn_fail(SCN_E_INVALID, "max_batch must be >= 1");
  if (!d.max_hits) d.max_hits = (uint32_t)std::min<uint64_t>((uint64_t)d.max_batch * 64u, 1u << 28);
  if (bytes_per_sample(d.sample_kind) == 0) return scn_fail(SCN_E_INVALID, "unknown sample_kind %u", d.sample_kind);
  if (d.sample_kind != SCN_KIND_FLOAT_COMPLEX && (d.enob < 1 || d.enob > 32))
    return scn_fail(SCN_E_INVALID, "enob %u out of range", d.enob);
  if (d.window_type < SCN_WIN_HANN || d.window_type > SCN_WIN_HAMMING) return scn_fail(SCN_E_INVALID, "unsupported window_type %u", d.window_type);
  if (d.mode != SCN_MODE_FREQUENCY_DOMAIN && d.mode != SCN_MODE_TIME_DOMAIN)
    return scn_fail(SCN_E_INVALID, "unsupported mode %u", d.mode);
  const Path path = path_of(d.mode, d.n);
  if (path == Path::Unsupported) return scn_fail(SCN_E_INVALID, "unsupported FFT size %u (16 to 65536)", d.n);
  if (d.n == 0 || d.n > (1u << 24)) return scn_fail(SCN_E_INVALID, "bad sample count %u", d.n);
  if (d.sample_rate == 0) return scn_fail(SCN_E_INVALID, "sample_rate must be > 0");
  const uint32_t avg = d.average ? d.average : 1u;
  if (avg > 1u) {  // (checked before the device: these are properties of the descriptor alone)
    if (d.mode != SCN_MODE_FREQUENCY_DOMAIN) return scn_fail(SCN_E_INVALID, "average %u needs a frequency-domain plan", avg);
    if (!scn_avg_size_supported(d.n)) return scn_fail(SCN_E_INVALID, "average %u: n = %u is not supported (1024, 2048, 4096, 8192)", avg, d.n);
    if (d.max_batch % avg) return scn_fail(SCN_E_INVALID, "average %u does not divide max_batch %u", avg, d.max_batch);
    if (d.average_layout != SCN_AVG_DWELL && d.average_layout != SCN_AVG_SWEEPS)
      return scn_fail(SCN_E_INVALID, "unknown average_layout %u", d.average_layout);
  }
  uint32_t i_lo = 0, i_hi = 0, floor_permille = 0;
  const uint32_t kept = evaluated_bins(d.n, d.dc_ignore_bins, d.use_bandwidth, &i_lo, &i_hi);
  if (d.detect != SCN_DETECT_FIXED && d.detect != SCN_DETECT_FLOOR && d.detect != SCN_DETECT_BASELINE)
    return scn_fail(SCN_E_INVALID, "unknown detect %u", d.detect);
  if (d.detect == SCN_DETECT_BASELINE) {  // (floor_permille is not read)
    if (d.mode != SCN_MODE_FREQUENCY_DOMAIN) return scn_fail(SCN_E_INVALID, "detect = SCN_DETECT_BASELINE needs a frequency-domain plan");
    // (the caller's own flags: a baseline plan names its outputs, the default of "neither -> both" does not apply to it)
    if (!(desc->flags & SCN_OUT_HITS)) return scn_fail(SCN_E_INVALID, "detect = SCN_DETECT_BASELINE needs SCN_OUT_HITS set in flags");
  }
  if (d.detect == SCN_DETECT_FLOOR) {  // (as the average's: properties of the descriptor alone)
    if (d.mode != SCN_MODE_FREQUENCY_DOMAIN) return scn_fail(SCN_E_INVALID, "detect = SCN_DETECT_FLOOR needs a frequency-domain plan");
    if (!(d.flags & SCN_OUT_HITS)) return scn_fail(SCN_E_INVALID, "detect = SCN_DETECT_FLOOR needs SCN_OUT_HITS");
    if (!floor_permille_of(d.floor_permille, &floor_permille))
      return scn_fail(SCN_E_INVALID, "floor_permille %u: 0 (the median), 1 ... 1000 or SCN_FLOOR_MIN", d.floor_permille);
    if (!kept) return scn_fail(SCN_E_INVALID, "detect = SCN_DETECT_FLOOR: the mask (dc_ignore_bins, use_bandwidth) lets no bin through");
  }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return scn_fail(SCN_E_NO_DEVICE, "no HIP device visible");
  if (d.device_id < 0 || d.device_id >= ndev) return scn_fail(SCN_E_INVALID, "device_id %d out of range", d.device_id);
  SCN_HIP(hipSetDevice(d.device_id));

  scn_plan *p = new (std::nothrow) scn_plan();
  if (!p) return scn_fail(SCN_E_NOMEM, "out of host memory");
  p->d = d;
  p->path = path;
  p->avg = avg;
  p->avg_layout = avg > 1u ? d.average_layout : (uint32_t)SCN_AVG_DWELL;
  p->buf_bytes = bytes_per_sample(d.sample_kind) * d.n;
  p->scale = convert_scale(d.sample_kind, d.enob);
  p->i_lo = i_lo;
  p->i_hi = i_hi;
  p->hit_region = std::max<uint32_t>(kept, 1u);
  p->floor = d.detect == SCN_DETECT_FLOOR;
  if (p->floor) p->floor_rank = (uint32_t)((uint64_t)floor_permille * (kept - 1u) / 1000u);
  p->floor_permille = floor_permille;
  p->baseline = d.detect == SCN_DETECT_BASELINE;
  build_window(d.window_type, d.n, p->h_window);

  hipDeviceProp_t prop;
  int st = SCN_OK;
  do {
#define SCN_TRY(call)                                                            \
  if ((call) != hipSuccess) {                                                    \
    st = scn_fail(SCN_E_HIP, "%s failed: %s", #call, hipGetErrorString(hipGetLastError())); \
    break;                                                                       \
  }
    SCN_TRY(hipGetDeviceProperties(&prop, d.device_id));
    p->num_cus = prop.multiProcessorCount;
    // (the fused kernels from 8192 points up store the counts to pinned memory themselves)
    p->direct_counts = d.n >= 8192 && (path == Path::FusedPow2 || path == Path::FusedMixed);
    SCN_TRY(p->stream.create());
    SCN_TRY(p->h2d_stream.create());
    SCN_TRY(p->d2h_stream.create());
    {  // the list stream's kernels are tiny and latency-critical: let the dispatcher take them first
      int lo = 0, hi = 0;
      SCN_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
      SCN_TRY(p->list_stream.create_with_priority(hi));
    }
    for (int k = 0; k < SCN_NUM_SLOTS; k++) {
      Slot &sl = p->slot[k];
      sl.stream = p->stream.get();
      if ((d.flags & SCN_PLAN_OVERLAP_SLOTS) && k > 0) {  // slot 0 keeps the plan's stream (scn_plan_stream)
        // slot 1's stream now, those of slots 2 and 3 when they are first used (ensure_slot_stream): HIP maps streams onto
        // 4 hardware queues, and a two-slot caller should not have five streams competing for them
        sl.own_stream = true;
        sl.stream = nullptr;
        if (k == 1) {
          SCN_TRY(sl.owned_stream.create());
          sl.stream = sl.owned_stream.get();
        }
      }
    }
    SCN_TRY(build_tables(p));
    for (int k = 0; k < SCN_NUM_SLOTS; k++) {
      SCN_TRY(p->slot[k].d_work_counter.alloc(8 * 32));
      SCN_TRY(hipMemsetAsync(p->slot[k].d_work_counter.get(), 0, sizeof(uint32_t) * 8 * 32, p->stream.get()));
    }
    SCN_TRY(hipStreamSynchronize(p->stream.get()));
#undef SCN_TRY
  } while (0);
  if (st != SCN_OK) {
    scn_plan_destroy(p);
    return st;
  }
  *out = p;
  return SCN_OK;
}

// (also the end of a scn_plan_create that failed half way: whatever exists by then is released, the rest was never created)
int scn_plan_destroy(scn_plan *p) {
  if (!p) return SCN_OK;
  (void)hipSetDevice(p->d.device_id);  // the members are released with the plan's device current ...
  p->stream.sync();                    // ... and nothing of the plan's still running
  p->h2d_stream.sync();
  p->d2h_stream.sync();
  p->list_stream.sync();
  for (int i = 0; i < SCN_NUM_SLOTS; i++) p->slot[i].owned_stream.sync();
  delete p;
  return SCN_OK;
}

int scn_plan_average_parts(const scn_plan *p, uint32_t nb, uint32_t *parts) {
  if (!p || !parts) return scn_fail(SCN_E_INVALID, "null argument");
  if (p->avg <= 1u) {
    *parts = 1;
    return SCN_OK;
  }
  if (nb % p->avg) return scn_fail(SCN_E_INVALID, "n_buffers %u is not a multiple of average %u", nb, p->avg);
  *parts = scn_avg_parts(p->d.n, nb / p->avg, p->avg, p->num_cus);
  return SCN_OK;
}

int scn_buffer_bytes(const scn_plan *p, size_t *bytes) {
  if (!p || !bytes) return scn_fail(SCN_E_INVALID, "null argument");
  *bytes = p->buf_bytes;
  return SCN_OK;
}

int scn_host_buffer(scn_plan *p, int slot, void **ptr, size_t *bytes) {
  if (int st = check_slot(p, slot)) return st;
  if (!ptr) return scn_fail(SCN_E_INVALID, "null argument");
  Slot &s = p->slot[slot];
  SCN_HIP(hipSetDevice(p->d.device_id));
  size_t total = p->buf_bytes * p->d.max_batch;
  SCN_HIP(s.h_raw.alloc(total));
  *ptr = s.h_raw.get();
  if (bytes) *bytes = total;
  return SCN_OK;
}

int scn_slot_stream(scn_plan *p, int slot, void **hip_stream) {
  if (int st = check_slot(p, slot)) return st;
  if (!hip_stream) return scn_fail(SCN_E_INVALID, "null argument");
  if (int st = ensure_slot_stream(p, p->slot[slot])) return st;
  *hip_stream = (void *)p->slot[slot].stream;
  return SCN_OK;
}

int scn_plan_stream(scn_plan *p, void **hip_stream) {
  if (!p || !hip_stream) return scn_fail(SCN_E_INVALID, "null argument");
  *hip_stream = (void *)p->stream.get();
  return SCN_OK;
}

int scn_device_spectrum(scn_plan *p, int slot, float **d_power_db) {
  if (int st = check_slot(p, slot)) return st;
  if (!d_power_db) return scn_fail(SCN_E_INVALID, "null argument");
  Slot &s = p->slot[slot];
  if (!s.d_power) {
    SCN_HIP(hipSetDevice(p->d.device_id));
    SCN_HIP(s.d_power.alloc((size_t)p->d.n * p->d.max_batch));
  }
  *d_power_db = s.d_power.get();
  return SCN_OK;
}

int scn_plan_window(const scn_plan *p, float *w, uint32_t n) {
  if (!p || !w) return scn_fail(SCN_E_INVALID, "null argument");
  if (n != p->d.n) return scn_fail(SCN_E_INVALID, "n %u != plan n %u", n, p->d.n);
  memcpy(w, p->h_window.data(), sizeof(float) * n);
  return SCN_OK;
}

}  // extern "C"
