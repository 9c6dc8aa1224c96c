// scn_history_plan.hip -- the hit history's side of the C-ABI (scanner_hip.h, "Hit history"; kernels: scn_history.hip): the plan's
// history words and visits, the fold of a collected slot into them, their read-out, and the confirmed list of a folded slot.
//
// Nothing asynchronous ever touches the history: no kernel of a submit reads or writes it, and the two calls that do -- the fold and
// the confirmation -- run on the slot's side stream (topup_stream_of, as scn_collect_signals) and synchronise before they return.  So
// every call here is allowed while OTHER slots are pending, and none of them waits for, or queues anything in front of, a pending
// slot's kernels.
#include <algorithm>

#include "scn_plan.h"

namespace {

// a plan that can have a history: frequency-domain, with SCN_OUT_HITS
int check_history_plan(const scn_plan *p) {
  if (!p) return scn_fail(SCN_E_INVALID, "null plan");
  if (p->d.mode != SCN_MODE_FREQUENCY_DOMAIN) return scn_fail(SCN_E_INVALID, "time-domain plan: it has no hits to remember");
  if (!(p->d.flags & SCN_OUT_HITS)) return scn_fail(SCN_E_INVALID, "plan was created without SCN_OUT_HITS");
  return SCN_OK;
}

// the submit's first_index (0 for a submit that named no run of the table), inside the history's rows
uint32_t history_first(const scn_plan *p, const Slot &s) {
  const int64_t first = s.cur().table_first;
  return first >= 0 ? (uint32_t)first % p->history_rows : 0u;
}

}  // namespace

extern "C" {

int scn_plan_set_history(scn_plan *p, uint32_t rows) {
  if (int st = check_history_plan(p)) return st;
  p->history_epoch++;  // (whatever was confirmed against the old words is no longer the plan's latest)
  p->history_rows = 0;
  if (!rows) return SCN_OK;  // (the allocation stays for the next one, as the baseline's)
  const size_t count = (size_t)rows * p->d.n;
  SCN_HIP(hipSetDevice(p->d.device_id));
  if (count > p->d_history.capacity()) SCN_HIP(p->d_history.grow(count));
  if (rows > p->d_visits.capacity()) SCN_HIP(p->d_visits.grow(rows));
  hipStream_t side = p->h2d_stream.get();
  SCN_HIP(hipMemsetAsync(p->d_history.get(), 0, sizeof(uint32_t) * count, side));
  SCN_HIP(hipMemsetAsync(p->d_visits.get(), 0, sizeof(uint32_t) * rows, side));
  SCN_HIP(hipStreamSynchronize(side));
  p->history_rows = rows;
  return SCN_OK;
}

int scn_plan_update_history(scn_plan *p, int slot) {
  if (int st = check_slot(p, slot)) return st;
  if (int st = check_history_plan(p)) return st;
  Slot &s = p->slot[slot];
  if (int st = require_list(s.life, slot, "hit list is still on the device")) return st;
  const bool units = s.life.n_buffers != 0;  // (a submit without units left the slot's header fields as they were: it named no table entry)
  if (int st = check_history_fold(p->history_rows, s.life.n_buffers, units && s.cur().table_first >= 0, p->table_count)) return st;
  if (int st = require_unfolded(s.life, slot)) return st;
  on_fold(s.life, ++p->history_epoch);
  if (!units) return SCN_OK;  // (no unit, no visit)
  SCN_HIP(hipSetDevice(p->d.device_id));
  // The regions and the counts are complete -- the slot's collect waited for the kernel that wrote them -- and the fold reads the
  // counts themselves, not the list's offsets: nothing to wait for.  Other slots may be pending: their kernels never read the history.
  ScnHistoryArgs a = {};
  a.regions = s.cur().d_hits.get();
  a.hit_region = p->hit_region;
  a.counts = s.cur().d_buf_hits.get();
  a.history = p->d_history.get();
  a.visits = p->d_visits.get();
  a.n = p->d.n;
  a.n_units = s.life.n_buffers;
  a.rows = p->history_rows;
  a.first = history_first(p, s);
  hipStream_t side = topup_stream_of(p, s);
  SCN_HIP(scn_launch_history_fold(a, p->num_cus, side));
  SCN_HIP(hipStreamSynchronize(side));
  return SCN_OK;
}

int scn_plan_get_history(scn_plan *p, uint32_t first_row, uint32_t rows, uint32_t *history, uint32_t *visits) {
  if (int st = check_history_plan(p)) return st;
  if (int st = check_history_range(p->history_rows, first_row, rows)) return st;
  if (!rows || (!history && !visits)) return SCN_OK;
  SCN_HIP(hipSetDevice(p->d.device_id));
  const size_t n = p->d.n;
  hipStream_t side = p->h2d_stream.get();
  if (history) SCN_HIP(hipMemcpyAsync(history, p->d_history.get() + (size_t)first_row * n, sizeof(uint32_t) * (size_t)rows * n, hipMemcpyDeviceToHost, side));
  if (visits) SCN_HIP(hipMemcpyAsync(visits, p->d_visits.get() + first_row, sizeof(uint32_t) * rows, hipMemcpyDeviceToHost, side));
  SCN_HIP(hipStreamSynchronize(side));
  return SCN_OK;
}

int scn_collect_confirmed(scn_plan *p, int slot, uint32_t m, uint32_t window, uint32_t first, scn_hit *hits, uint32_t cap, uint32_t *n_confirmed) {
  if (int st = check_slot(p, slot)) return st;
  if (!n_confirmed) return scn_fail(SCN_E_INVALID, "null argument");
  *n_confirmed = 0;
  if (!hits && cap) return scn_fail(SCN_E_INVALID, "null hits with cap %u", cap);
  if (int st = check_history_plan(p)) return st;
  if (int st = check_history_window(m, window)) return st;
  Slot &s = p->slot[slot];
  if (int st = require_list(s.life, slot, "hit list is still on the device")) return st;
  if (int st = require_latest_fold(s.life, slot, p->history_epoch, p->history_rows)) return st;
  if (s.life.total_hits == 0) return SCN_OK;
  SCN_HIP(hipSetDevice(p->d.device_id));
  int st = fetch_list(p, s, 0);  // (the hits' offsets come from the scan: wait for it)
  if (st) return st;
  SCN_HIP(s.d_conf_counts.alloc(p->d.max_batch));
  SCN_HIP(s.d_conf_offsets.alloc((size_t)p->d.max_batch + 1u));
  ScnConfirmArgs a = {};
  set_list_source(a, p, s);
  a.history = p->d_history.get();
  a.rows = p->history_rows;
  a.hist_first = history_first(p, s);
  a.m = m;
  a.mask = scn_history_mask(window);
  a.conf_counts = s.d_conf_counts.get();
  a.conf_offsets = s.d_conf_offsets.get();
  ScnCompactArgs scan = compact_args(p, s, 0, 0, nullptr);  // the scan kernel as it is, on the confirmed counts
  scan.counts = s.d_conf_counts.get();
  scan.offsets = s.d_conf_offsets.get();
  hipStream_t side = topup_stream_of(p, s);  // (pending slots are not disturbed)
  SCN_HIP(scn_launch_confirm_count(a, side));
  SCN_HIP(scn_launch_hit_scan(scan, side));
  uint32_t total = 0;
  SCN_HIP(hipMemcpyAsync(&total, s.d_conf_offsets.get() + s.life.n_buffers, sizeof(uint32_t), hipMemcpyDeviceToHost, side));
  SCN_HIP(hipStreamSynchronize(side));
  *n_confirmed = total;
  const uint32_t want = first < total ? std::min(cap, total - first) : 0u;
  if (want) {
    if (s.d_conf_window.capacity() < want) SCN_HIP(s.d_conf_window.grow(want));
    a.out = s.d_conf_window.get();
    a.first = first;
    a.out_cap = want;  // (first + want <= total <= the hits' total < 2^31: no wrap)
    SCN_HIP(scn_launch_confirm_build(a, side));
    SCN_HIP(hipMemcpyAsync(hits, s.d_conf_window.get(), sizeof(scn_hit) * (size_t)want, hipMemcpyDeviceToHost, side));
    SCN_HIP(hipStreamSynchronize(side));
  }
  if ((uint64_t)first + cap < total)
    return scn_fail(SCN_E_TRUNCATED, "%u confirmed records, [%u, %u) returned: call again with a later first", total, first, first + want);
  return SCN_OK;
}

}  // extern "C"
