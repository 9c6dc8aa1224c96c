// scn_levels_plan.hip -- the level histogram's side of the C-ABI (scanner_hip.h, "Level histogram"; kernels: scn_levels.hip;
// arithmetic: scn_levels.h and scn_trace.h): the plan's counters, their geometry and table of edges, the fold of a collected slot's
// spectrum into them, their read-out and their summary.
//
// As the trace's, nothing asynchronous ever touches the histogram: no kernel of a submit reads or writes it, and the fold runs on
// the slot's side stream (topup_stream_of) and synchronises before it returns.  So every call here is allowed while OTHER slots are
// pending.  Which plans, and what a fold refuses, are the trace's own checks (scn_trace_plan.hip).
#include "scn_levels.h"
#include "scn_plan.h"

extern "C" {

int scn_plan_set_levels(scn_plan *p, uint64_t f0_hz, uint32_t cell_hz, uint32_t cells, const float *edges_db, uint32_t n_edges) {
  if (int st = check_trace_plan(p)) return st;
  if (!cells) {  // (the allocation stays for the next one, as the trace's)
    p->levels_cells = 0;
    return SCN_OK;
  }
  if (int st = check_levels_geometry(cell_hz, cells, n_edges)) return st;
  uint32_t keys[kLevelsKeys];
  if (int st = check_levels_edges(edges_db, n_edges, keys)) return st;
  SCN_HIP(hipSetDevice(p->d.device_id));
  SCN_HIP(p->d_levels_keys.alloc(kLevelsKeys));
  const size_t words = (size_t)cells * (n_edges + 1u);
  p->levels_cells = 0;  // (from here on a failure of the device leaves the plan without a histogram: the header says so)
  if (words > p->d_levels_hist.capacity()) SCN_HIP(p->d_levels_hist.grow(words));
  hipStream_t side = p->h2d_stream.get();  // (`keys` outlives the copy: the stream is synchronised below)
  SCN_HIP(hipMemcpyAsync(p->d_levels_keys.get(), keys, sizeof(keys), hipMemcpyHostToDevice, side));
  SCN_HIP(hipMemsetAsync(p->d_levels_hist.get(), 0, sizeof(unsigned long long) * words, side));
  SCN_HIP(hipStreamSynchronize(side));
  p->levels_f0 = f0_hz;
  p->levels_cell_hz = cell_hz;
  p->levels_edges = n_edges;
  p->levels_cells = cells;
  return SCN_OK;
}

int scn_plan_update_levels(scn_plan *p, int slot) {
  bool folds;
  if (int st = check_trace_fold(p, slot, p && p->levels_cells, "the plan has no level histogram: scn_plan_set_levels was never called, or dropped it", &folds))
    return st;
  if (!folds) return SCN_OK;
  Slot &s = p->slot[slot];
  SCN_HIP(hipSetDevice(p->d.device_id));
  ScnLevelsArgs a = {};
  set_fold_source(a, p, s);
  a.f0_hz = p->levels_f0;
  a.cell_hz = p->levels_cell_hz;
  a.cells = p->levels_cells;
  a.edge_keys = p->d_levels_keys.get();
  a.n_edges = p->levels_edges;
  a.hist = p->d_levels_hist.get();
  hipStream_t side = topup_stream_of(p, s);
  SCN_HIP(scn_launch_levels_fold(a, p->num_cus, side));
  SCN_HIP(hipStreamSynchronize(side));
  return SCN_OK;
}

int scn_plan_get_levels(scn_plan *p, uint32_t first_cell, uint32_t cells, uint64_t *hist) {
  if (int st = check_trace_plan(p)) return st;
  if (int st = check_trace_range(p->levels_cells, first_cell, cells)) return st;
  if (!cells) return SCN_OK;
  if (!hist) return scn_fail(SCN_E_INVALID, "null argument");
  SCN_HIP(hipSetDevice(p->d.device_id));
  hipStream_t side = p->h2d_stream.get();
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters arrive in the caller's array");
  const size_t n_levels = p->levels_edges + 1u;
  SCN_HIP(hipMemcpyAsync(hist, p->d_levels_hist.get() + (size_t)first_cell * n_levels, sizeof(uint64_t) * (size_t)cells * n_levels, hipMemcpyDeviceToHost, side));
  SCN_HIP(hipStreamSynchronize(side));
  return SCN_OK;
}

int scn_plan_levels_summary(scn_plan *p, uint32_t first_cell, uint32_t cells, uint32_t permille, uint32_t level, uint32_t *rank_level, uint64_t *above,
                            uint64_t *total) {
  if (int st = check_trace_plan(p)) return st;
  if (int st = check_trace_range(p->levels_cells, first_cell, cells)) return st;
  if (int st = check_levels_summary(p->levels_cells ? p->levels_edges + 1u : 1u, permille, level)) return st;
  if (!cells || (!rank_level && !above && !total)) return SCN_OK;
  SCN_HIP(hipSetDevice(p->d.device_id));
  if (cells > p->d_levels_rank.capacity()) {  // (the rank, allocated last, vouches for both)
    p->d_levels_rank.reset();
    SCN_HIP(p->d_levels_sums.grow(2u * (size_t)cells));
    SCN_HIP(p->d_levels_rank.grow(cells));
  }
  ScnLevelsSummaryArgs a = {};
  a.hist = p->d_levels_hist.get();
  a.first_cell = first_cell;
  a.cells = cells;
  a.n_levels = p->levels_edges + 1u;
  a.permille = permille;
  a.level = level;
  a.rank_level = p->d_levels_rank.get();
  a.above = p->d_levels_sums.get();
  a.total = p->d_levels_sums.get() + cells;
  hipStream_t side = p->h2d_stream.get();
  SCN_HIP(scn_launch_levels_summary(a, side));
  if (rank_level) SCN_HIP(hipMemcpyAsync(rank_level, a.rank_level, sizeof(uint32_t) * (size_t)cells, hipMemcpyDeviceToHost, side));
  if (above) SCN_HIP(hipMemcpyAsync(above, a.above, sizeof(uint64_t) * (size_t)cells, hipMemcpyDeviceToHost, side));
  if (total) SCN_HIP(hipMemcpyAsync(total, a.total, sizeof(uint64_t) * (size_t)cells, hipMemcpyDeviceToHost, side));
  SCN_HIP(hipStreamSynchronize(side));
  return SCN_OK;
}

}  // extern "C"
