// scn_emitters_plan.hip -- the trace emitters' side of the C-ABI (scanner_hip.h, "Trace emitters"; kernels: scn_emitters.hip;
// arithmetic: scn_emitters.h): a window of the plan's trace segmented into emitter records on the GPU, of which only the page asked
// for crosses to the host, and a host trace merged into the plan's.
//
// As the trace's read-out, both run on the plan's side stream and synchronise before they return: nothing of a submit is queued
// there and no kernel of a submit touches the trace, so both are allowed while slots are pending.  Which plans: the trace's own
// check (scn_trace_plan.hip).
#include <algorithm>
#include <initializer_list>

#include "scn_emitters.h"
#include "scn_plan.h"

extern "C" {

int scn_plan_merge_trace(scn_plan *p, uint32_t first_cell, uint32_t cells, const float *src_max, const float *src_min, const uint64_t *src_count) {
  if (int st = check_trace_plan(p)) return st;
  if (!p->trace_cells) return scn_fail(SCN_E_STATE, "the plan has no trace: scn_plan_set_trace was never called, or dropped it");
  if (int st = check_trace_range(p->trace_cells, first_cell, cells)) return st;
  if (!cells) return SCN_OK;
  if (!src_max || !src_min || !src_count) return scn_fail(SCN_E_INVALID, "null argument");
  for (const float *src : {src_max, src_min})  // (before anything is uploaded: the plan's trace never holds a NaN)
    for (uint32_t c = 0; c < cells; c++)
      if (scn_trace_is_nan(scn_emit_bits(src[c]))) return scn_fail(SCN_E_INVALID, "%s[%u] is a NaN", src == src_max ? "src_max" : "src_min", c);
  SCN_HIP(hipSetDevice(p->d.device_id));
  if (cells > p->d_merge_count.capacity()) {  // (the count, allocated last, vouches for both)
    p->d_merge_count.reset();
    SCN_HIP(p->d_merge_bits.grow(2u * (size_t)cells));
    SCN_HIP(p->d_merge_count.grow(cells));
  }
  static_assert(sizeof(float) == sizeof(uint32_t) && sizeof(unsigned long long) == sizeof(uint64_t), "the caller's arrays are uploaded as they are");
  ScnTraceMergeArgs a = {};
  a.max_key = p->d_trace_max.get();
  a.min_key = p->d_trace_min.get();
  a.count = p->d_trace_count.get();
  a.first_cell = first_cell;
  a.cells = cells;
  a.src_max = p->d_merge_bits.get();
  a.src_min = p->d_merge_bits.get() + cells;
  a.src_count = p->d_merge_count.get();
  hipStream_t side = p->h2d_stream.get();  // (the caller's arrays outlive the copies: the stream is synchronised below)
  SCN_HIP(hipMemcpyAsync(p->d_merge_bits.get(), src_max, sizeof(float) * (size_t)cells, hipMemcpyHostToDevice, side));
  SCN_HIP(hipMemcpyAsync(p->d_merge_bits.get() + cells, src_min, sizeof(float) * (size_t)cells, hipMemcpyHostToDevice, side));
  SCN_HIP(hipMemcpyAsync(p->d_merge_count.get(), src_count, sizeof(uint64_t) * (size_t)cells, hipMemcpyHostToDevice, side));
  SCN_HIP(scn_launch_trace_merge(a, side));
  SCN_HIP(hipStreamSynchronize(side));
  return SCN_OK;
}

int scn_plan_trace_emitters(scn_plan *p, uint32_t first_cell, uint32_t cells, uint32_t line, float threshold_db, uint32_t max_gap, uint32_t first,
                            scn_emitter *out, uint32_t cap, uint32_t *n_emitters) {
  if (int st = check_trace_plan(p)) return st;
  if (!n_emitters) return scn_fail(SCN_E_INVALID, "null argument");
  *n_emitters = 0;
  if (!out && cap) return scn_fail(SCN_E_INVALID, "null out with cap %u", cap);
  if (int st = check_emitters_line(line, threshold_db)) return st;
  if (!p->trace_cells) return scn_fail(SCN_E_STATE, "the plan has no trace: scn_plan_set_trace was never called, or dropped it");
  if (int st = check_trace_range(p->trace_cells, first_cell, cells)) return st;
  if (!cells) return SCN_OK;
  SCN_HIP(hipSetDevice(p->d.device_id));
  SCN_HIP(p->d_emit_tiles.alloc(5u * (size_t)kEmitTilesMax + 1u));
  ScnEmittersArgs a = {};
  a.max_key = p->d_trace_max.get();
  a.min_key = p->d_trace_min.get();
  a.count = p->d_trace_count.get();
  a.f0_hz = p->trace_f0;
  a.cell_hz = p->trace_cell_hz;
  a.first_cell = first_cell;
  a.cells = cells;
  a.line = line;
  a.threshold_bits = scn_emit_bits(threshold_db);
  a.max_gap = max_gap;
  a.tile_last = p->d_emit_tiles.get();
  a.tile_first = a.tile_last + kEmitTilesMax;
  a.tile_starts = a.tile_first + kEmitTilesMax;
  a.carry_last = a.tile_starts + kEmitTilesMax;
  a.carry_starts = a.carry_last + kEmitTilesMax;
  a.total = a.carry_starts + kEmitTilesMax;
  hipStream_t side = p->h2d_stream.get();
  SCN_HIP(scn_launch_emitters_count(a, side));
  uint32_t total = 0;
  SCN_HIP(hipMemcpyAsync(&total, a.total, sizeof(uint32_t), hipMemcpyDeviceToHost, side));
  SCN_HIP(hipStreamSynchronize(side));
  *n_emitters = total;
  const uint32_t want = first < total ? std::min(cap, total - first) : 0u;
  if (want) {
    if (p->d_emit_acc.capacity() < total) SCN_HIP(p->d_emit_acc.grow(total));  // (at most cells / 2 + 1 of them)
    if (p->d_emit_page.capacity() < want) SCN_HIP(p->d_emit_page.grow(want));
    a.acc = p->d_emit_acc.get();
    a.acc_cap = total;
    a.out = p->d_emit_page.get();
    a.first = first;
    a.out_cap = want;  // (first + want <= total: no wrap)
    SCN_HIP(hipMemsetAsync(a.acc, 0, sizeof(ScnEmitterAcc) * (size_t)total, side));
    SCN_HIP(scn_launch_emitters_build(a, side));
    SCN_HIP(scn_launch_emitters_finish(a, side));
    SCN_HIP(hipMemcpyAsync(out, a.out, sizeof(scn_emitter) * (size_t)want, hipMemcpyDeviceToHost, side));
    SCN_HIP(hipStreamSynchronize(side));
  }
  if ((uint64_t)first + cap < total)
    return scn_fail(SCN_E_TRUNCATED, "%u emitters, records [%u, %u) returned: call again with a later first", total, first, first + want);
  return SCN_OK;
}

}  // extern "C"
