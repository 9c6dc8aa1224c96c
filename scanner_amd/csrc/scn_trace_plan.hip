// scn_trace_plan.hip -- the sweep trace's side of the C-ABI (scanner_hip.h, "Sweep trace"; kernel: scn_trace.hip; arithmetic:
// scn_trace.h): the plan's three arrays and their geometry, the fold of a collected slot's spectrum into them, their read-out.
//
// As the hit history's, nothing asynchronous ever touches the trace: no kernel of a submit reads or writes it, and the fold runs on
// the slot's side stream (topup_stream_of) and synchronises before it returns.  So every call here is allowed while OTHER slots are
// pending.  max_db and min_db live on the device as ordered keys, which is what atomicMax / atomicMin need; the read-out turns them
// back into the winning values' bits on the host.
#include <cstring>
#include <initializer_list>

#include "scn_plan.h"
#include "scn_trace.h"

// a plan that can have a trace: frequency-domain, with SCN_OUT_HITS (its submits stage their centres), and its submits store a spectrum
int check_trace_plan(const scn_plan *p) {
  if (!p) return scn_fail(SCN_E_INVALID, "null plan");
  if (p->d.mode != SCN_MODE_FREQUENCY_DOMAIN) return scn_fail(SCN_E_INVALID, "time-domain plan: it has no spectrum to trace");
  if (!(p->d.flags & SCN_OUT_HITS)) return scn_fail(SCN_E_INVALID, "plan was created without SCN_OUT_HITS: its submits stage no centre frequencies");
  if (!(p->d.flags & SCN_OUT_SPECTRUM) && !detects_behind(p))
    return scn_fail(SCN_E_INVALID, "a fixed-threshold plan without SCN_OUT_SPECTRUM stores no spectrum");
  return SCN_OK;
}

// The refusals of a fold, before anything is queued.  Where it returns SCN_OK with *folds set, the spectrum is complete -- the
// slot's collect waited for the kernel that wrote it -- and stays until the slot's next submit; the centres lie where that submit
// left them (the slot's pinned copy or the plan's table).  Other slots may be pending: their kernels never touch what a fold writes.
int check_trace_fold(scn_plan *p, int slot, bool owns, const char *none, bool *folds) {
  *folds = false;
  if (int st = check_slot(p, slot)) return st;
  if (int st = check_trace_plan(p)) return st;
  const Slot &s = p->slot[slot];
  if (int st = require_list(s.life, slot, "hit list is still on the device")) return st;
  if (!owns) return scn_fail(SCN_E_STATE, "%s", none);
  if (!s.life.n_buffers) return SCN_OK;  // (no unit, nothing to fold)
  if (!s.spec_power || s.spec_units != s.life.n_buffers) return scn_fail(SCN_E_STATE, "slot %d: its submit stored no spectrum", slot);
  *folds = true;
  return SCN_OK;
}

extern "C" {

int scn_plan_set_trace(scn_plan *p, uint64_t f0_hz, uint32_t cell_hz, uint32_t cells) {
  if (int st = check_trace_plan(p)) return st;
  if (cells)
    if (int st = check_trace_geometry(cell_hz, cells)) return st;
  p->trace_cells = 0;
  if (!cells) return SCN_OK;  // (the allocation stays for the next one, as the history's)
  SCN_HIP(hipSetDevice(p->d.device_id));
  if (cells > p->d_trace_count.capacity()) {  // (the count, allocated last, vouches for all three)
    p->d_trace_count.reset();
    SCN_HIP(p->d_trace_max.grow(cells));
    SCN_HIP(p->d_trace_min.grow(cells));
    SCN_HIP(p->d_trace_count.grow(cells));
  }
  hipStream_t side = p->h2d_stream.get();
  SCN_HIP(hipMemsetD32Async((hipDeviceptr_t)p->d_trace_max.get(), (int)kTraceEmptyMaxKey, cells, side));
  SCN_HIP(hipMemsetD32Async((hipDeviceptr_t)p->d_trace_min.get(), (int)kTraceEmptyMinKey, cells, side));
  SCN_HIP(hipMemsetAsync(p->d_trace_count.get(), 0, sizeof(unsigned long long) * (size_t)cells, side));
  SCN_HIP(hipStreamSynchronize(side));
  p->trace_f0 = f0_hz;
  p->trace_cell_hz = cell_hz;
  p->trace_cells = cells;
  return SCN_OK;
}

int scn_plan_update_trace(scn_plan *p, int slot) {
  bool folds;
  if (int st = check_trace_fold(p, slot, p && p->trace_cells, "the plan has no trace: scn_plan_set_trace was never called, or dropped it", &folds)) return st;
  if (!folds) return SCN_OK;
  Slot &s = p->slot[slot];
  SCN_HIP(hipSetDevice(p->d.device_id));
  ScnTraceArgs a = {};
  set_fold_source(a, p, s);
  a.f0_hz = p->trace_f0;
  a.cell_hz = p->trace_cell_hz;
  a.cells = p->trace_cells;
  a.max_key = p->d_trace_max.get();
  a.min_key = p->d_trace_min.get();
  a.count = p->d_trace_count.get();
  hipStream_t side = topup_stream_of(p, s);
  SCN_HIP(scn_launch_trace_fold(a, p->num_cus, side));
  SCN_HIP(hipStreamSynchronize(side));
  return SCN_OK;
}

int scn_plan_get_trace(scn_plan *p, uint32_t first_cell, uint32_t cells, float *max_db, float *min_db, uint64_t *count) {
  if (int st = check_trace_plan(p)) return st;
  if (int st = check_trace_range(p->trace_cells, first_cell, cells)) return st;
  if (!cells || (!max_db && !min_db && !count)) return SCN_OK;
  SCN_HIP(hipSetDevice(p->d.device_id));
  hipStream_t side = p->h2d_stream.get();
  static_assert(sizeof(float) == sizeof(uint32_t) && sizeof(unsigned long long) == sizeof(uint64_t), "the keys arrive in the caller's arrays");
  if (max_db) SCN_HIP(hipMemcpyAsync(max_db, p->d_trace_max.get() + first_cell, sizeof(uint32_t) * (size_t)cells, hipMemcpyDeviceToHost, side));
  if (min_db) SCN_HIP(hipMemcpyAsync(min_db, p->d_trace_min.get() + first_cell, sizeof(uint32_t) * (size_t)cells, hipMemcpyDeviceToHost, side));
  if (count) SCN_HIP(hipMemcpyAsync(count, p->d_trace_count.get() + first_cell, sizeof(uint64_t) * (size_t)cells, hipMemcpyDeviceToHost, side));
  SCN_HIP(hipStreamSynchronize(side));
  for (float *keys : {max_db, min_db}) {  // key -> the winning value's bits, in place
    if (!keys) continue;
    for (uint32_t c = 0; c < cells; c++) {
      uint32_t key;
      memcpy(&key, keys + c, sizeof(key));
      const uint32_t bits = scn_trace_unkey(key);
      memcpy(keys + c, &bits, sizeof(bits));
    }
  }
  return SCN_OK;
}

}  // extern "C"
