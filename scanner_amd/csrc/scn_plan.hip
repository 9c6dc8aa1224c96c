// scn_plan.hip -- a plan's lifecycle: the device side of its creation (the streams and the tables' uploads: what they hold and every
// number of the plan is resolve_plan's, scn_host.hip), what a slot allocates at its first use, its end (the members release
// themselves, scn_resource.h), and the getters.
#include <cstring>
#include <new>

#include "scn_plan.h"

namespace {

// The window and the tables the plan's path reads (a time-domain plan reads none)
hipError_t build_tables(scn_plan *p) {
  const uint32_t n = p->d.n;
  hipError_t e;
  if (p->path == Path::TimeDomain) return hipSuccess;
  if ((e = upload(p->d_window, p->h_window)) != hipSuccess) return e;
  switch (p->path) {
    case Path::FusedPow2:
    case Path::FusedMixed: {
      uint32_t rows, threads;
      if (p->path == Path::FusedMixed) scn_mixed_layout(n, &rows, &threads);
      else scn_tw1_layout(n, &rows, &threads);
      if ((e = upload(p->d_twiddle, twiddles<float>(n))) != hipSuccess) return e;
      if (p->avg > 1u && n == 8192) {  // the averaged kernel's two 4096-point halves and the radix-2 step that joins them
        const ScnAvgHalfTables t = avg_half_tables();
        if ((e = upload(p->d_avg_tw1, t.half)) != hipSuccess || (e = upload(p->d_avg_tw, t.join)) != hipSuccess) return e;
      }
      return upload(p->d_tw1_table, fused_tw1_table(n, rows, threads));
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
  PlanShape shape;
  if (int st = resolve_plan(desc, &shape)) return st;
  const scn_plan_desc &d = shape.d;

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return scn_fail(SCN_E_NO_DEVICE, "no HIP device visible");
  if (d.device_id < 0 || d.device_id >= ndev) return scn_fail(SCN_E_INVALID, "device_id %d out of range", d.device_id);
  SCN_HIP(hipSetDevice(d.device_id));

  scn_plan *p = new (std::nothrow) scn_plan();
  if (!p) return scn_fail(SCN_E_NOMEM, "out of host memory");
  static_cast<PlanShape &>(*p) = shape;
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
