// scn_collect.hip -- the collect side of the C-ABI: waiting for a slot, its counts and trigger flags, the ordered hit list
// (built behind the launch or on demand, fetched to pinned memory), windows beyond max_hits, signals, the floor.
#include <algorithm>
#include <cstring>

#include "scn_plan.h"

// the first `count` records of the slot's list are in pinned host memory
int fetch_list(scn_plan *p, Slot &s, uint32_t count) {
  if (!s.life.list_built)
    if (int st = build_list(p, s, false)) return st;
  SCN_HIP(hipEventSynchronize(s.cur().list_done.get()));
  count = std::min(count, p->d.max_hits);
  if (count > s.prefetched) {
    // the prediction was short: copy the rest now.  NOT on the list stream: the other slot's list may be queued there
    // behind a launch that is still running, and this copy would wait for it; the list it reads is complete (the event
    // above), so any idle stream will do.
    hipStream_t side = topup_stream_of(p, s);
    SCN_HIP(hipMemcpyAsync(s.h_list.get() + s.prefetched, s.d_list.get() + s.prefetched, sizeof(scn_hit) * (size_t)(count - s.prefetched),
                           hipMemcpyDeviceToHost, side));
    SCN_HIP(hipStreamSynchronize(side));
    s.prefetched = count;
  }
  return SCN_OK;
}

ScnCompactArgs compact_args(const scn_plan *p, const Slot &s, uint32_t first, uint32_t cap, void *out) {
  ScnCompactArgs c;
  set_list_source(c, p, s);
  c.counts = s.cur().d_buf_hits.get();
  c.out = out;
  c.first = first;
  c.out_cap = std::min<uint32_t>(cap, 0x7fffffffu - first);  // first + out_cap must not wrap
  return c;
}

// Scan + compaction of the slot's pending / last submit into d_list, behind everything already queued on the list's
// stream; with `prefetch`, followed by a DMA of the expected number of records into the pinned h_list (the size of a
// copy has to be known when it is queued, long before this batch's own total is: the plan predicts it from the last
// one, and fetch_list tops up whatever is missing).  The DMA goes on the D2H stream behind an event, not behind the list
// kernels on their own stream: scan + compaction + copy in series took longer per submit (~90 us for a C2 list) than the FFT
// launch they run beside (73 us), so the records loop was bound by the list stream; split, each stream has < 50 us of work
// per submit (round 4, profiles/r04_experiments.md section 1: 310 -> 378 Gsamples/s through scn_hits_view from a C++ caller).
// What the copy runs on is the HIP runtime's choice: an SDMA engine with the system runtime (ROCm 7.2), a blit KERNEL with the
// runtime a torch process brings along (ROCm 7.0) -- and a shader that writes host memory beside an HBM-streaming kernel
// stalls it by the PCIe time of its bytes (scripts/ubench/pcie_beside.hip: 70 -> 95 us), which is also why the compaction
// kernel does not store the list into pinned memory itself (measured: 335 Gsamples/s against 378).
int build_list(scn_plan *p, Slot &s, bool prefetch) {
  hipStream_t aux = list_stream_of(p, s);
  ScnCompactArgs c = compact_args(p, s, 0, p->d.max_hits, s.d_list.get());
  SCN_HIP(scn_launch_hit_scan(c, aux));
  SCN_HIP(scn_launch_hit_compact(c, aux));
  s.prefetched = prefetch ? std::min(p->predict, p->d.max_hits) : 0u;
  hipStream_t last = aux;
  if (s.prefetched) {
    if (!s.own_stream) {  // (a slot with a stream of its own keeps its whole chain there: its next kernel is several submits away)
      SCN_HIP(hipEventRecord(s.cur().list_done.get(), aux));
      SCN_HIP(hipStreamWaitEvent(p->d2h_stream.get(), s.cur().list_done.get(), 0));
      last = p->d2h_stream.get();
    }
    SCN_HIP(hipMemcpyAsync(s.h_list.get(), s.d_list.get(), sizeof(scn_hit) * (size_t)s.prefetched, hipMemcpyDeviceToHost, last));
  }
  SCN_HIP(hipEventRecord(s.cur().list_done.get(), last));
  s.cur().list_used = true;
  on_list_built(s.life);
  return SCN_OK;
}

extern "C" {

int scn_wait(scn_plan *p, int slot) {
  if (int st = check_slot(p, slot)) return st;
  Slot &s = p->slot[slot];
  if (int st = require_pending(s.life, slot)) return st;
  SCN_HIP(hipSetDevice(p->d.device_id));
  SCN_HIP(hipEventSynchronize(s.done.get()));
  return SCN_OK;
}

int scn_collect_time_domain(scn_plan *p, int slot, float *max_db, float *min_db, uint8_t *above) {
  int st = check_slot(p, slot);
  if (st) return st;
  if (p->d.mode != SCN_MODE_TIME_DOMAIN) return scn_fail(SCN_E_INVALID, "plan is not in time-domain mode");
  st = scn_wait(p, slot);
  if (st) return st;
  Slot &s = p->slot[slot];
  on_collect_time_domain(s.life);
  const float *mx = s.h_td.get(), *mn = s.h_td.get() + p->d.max_batch;
  for (uint32_t b = 0; b < s.life.n_buffers; b++) {
    if (max_db) max_db[b] = mx[b];
    if (min_db) min_db[b] = mn[b];
    if (above) above[b] = mx[b] >= p->d.threshold;  // process.cpp:226
  }
  return SCN_OK;
}

int scn_collect(scn_plan *p, int slot, float *power_db, scn_hit *hits, uint32_t hit_cap, uint32_t *n_hits,
                uint8_t *trigger) {
  int st = check_slot(p, slot);
  if (st) return st;
  if (p->d.mode != SCN_MODE_FREQUENCY_DOMAIN) return scn_fail(SCN_E_INVALID, "time-domain plan: use scn_collect_time_domain");
  st = scn_wait(p, slot);  // the kernel and the per-buffer counts; the ordered list has an event of its own
  if (st) return st;
  Slot &s = p->slot[slot];
  on_take(s.life);  // (before the argument checks below: a collect they refuse has consumed the submit)
  const uint32_t n = p->d.n, nb = s.life.n_buffers;
  const bool have_hits = (p->d.flags & SCN_OUT_HITS) != 0;
  if ((hits || trigger) && !have_hits) return scn_fail(SCN_E_INVALID, "plan was created without SCN_OUT_HITS");
  if (power_db && !s.cur_power) return scn_fail(SCN_E_INVALID, "plan was created without SCN_OUT_SPECTRUM");

  uint64_t total = 0;
  if (have_hits && nb && s.route.counts == Counts::Reduced) {
    total = *s.h_total;
    if (trigger)  // process.cpp:62, one bit per buffer from the GPU
      for (uint32_t b = 0; b < nb; b++) trigger[b] = (uint8_t)((s.h_buf_hits.get()[b >> 5] >> (b & 31u)) & 1u);
  } else if (have_hits && nb) {
    for (uint32_t b = 0; b < nb; b++) {
      const uint32_t c = s.h_buf_hits.get()[b];
      total += c;
      if (trigger) trigger[b] = c > p->d.trigger_count;  // process.cpp:62
    }
  } else if (trigger) {
    memset(trigger, 0, nb);
  }
  if ((st = on_collect(s.life, have_hits, total))) return st;
  if (have_hits) {  // what the automatic mode goes by at the next submit
    if (total && p->view_age < 0xffffffffu) p->view_age++;
    p->records_wanted = hits != nullptr || p->view_age <= 4u;
    if (total && p->device_list_age < 0xffffffffu) p->device_list_age++;
    p->device_list_wanted = p->device_list_age <= 4u;
    // the prefetch covers this total + 1/16 + twice the change since the total before (the DMA's time is the records loop's
    // period on a hits-only plan: a flat 25 % margin cost 46 us per submit instead of 39; a short prediction costs one small
    // top-up copy at collect)
    const uint64_t change = total > p->last_total ? total - p->last_total : p->last_total - total;
    p->predict = (uint32_t)std::min<uint64_t>(total + std::max<uint64_t>(total / 16u, 2u * change) + 64u, p->d.max_hits);
    p->last_total = (uint32_t)total;
  }
  if (n_hits) *n_hits = (uint32_t)total;
  uint32_t copied = 0;
  if (hits && total) {
    // the compaction kernel has left the first max_hits records, ordered and complete, in device memory
    copied = std::min(std::min((uint32_t)total, hit_cap), p->d.max_hits);
    if ((st = fetch_list(p, s, copied))) return st;
    memcpy(hits, s.h_list.get(), sizeof(scn_hit) * copied);
  }
  if (power_db && nb) {
    SCN_HIP(hipMemcpyAsync(power_db, s.cur_power, sizeof(float) * (size_t)n * nb, hipMemcpyDeviceToHost, s.stream));
    SCN_HIP(hipStreamSynchronize(s.stream));
  }
  if (hits && copied < total)
    return scn_fail(SCN_E_TRUNCATED, "%u hits, %u returned (caller capacity %u, plan max_hits %u): scn_collect_more fetches the rest",
                (uint32_t)total, copied, hit_cap, p->d.max_hits);
  return SCN_OK;
}

int scn_collect_more(scn_plan *p, int slot, uint32_t first, scn_hit *hits, uint32_t hit_cap, uint32_t *n_written) {
  int st = check_slot(p, slot);
  if (st) return st;
  if (!hits || !n_written) return scn_fail(SCN_E_INVALID, "null argument");
  *n_written = 0;
  Slot &s = p->slot[slot];
  if ((st = require_list(s.life, slot, "hit list is still on the device"))) return st;
  if (first >= s.life.total_hits || hit_cap == 0) return SCN_OK;
  SCN_HIP(hipSetDevice(p->d.device_id));
  const uint32_t want = std::min(hit_cap, s.life.total_hits - first);
  if (first + want <= p->d.max_hits) {  // still inside the part the plan keeps
    if ((st = fetch_list(p, s, first + want))) return st;
    memcpy(hits, s.h_list.get() + first, sizeof(scn_hit) * want);
    *n_written = want;
    return SCN_OK;
  }
  // re-run the compaction for the window [first, first + want): regions, counts and offsets stay valid until the
  // slot's next submit
  if ((st = fetch_list(p, s, 0))) return st;  // (the offsets come from the scan; the slot's list must be complete)
  if (s.d_window.capacity() < want) SCN_HIP(s.d_window.grow(want));
  hipStream_t side = topup_stream_of(p, s);  // (fetch_list above waited for the scan: the offsets are there)
  SCN_HIP(scn_launch_hit_compact(compact_args(p, s, first, want, s.d_window.get()), side));
  SCN_HIP(hipMemcpyAsync(hits, s.d_window.get(), sizeof(scn_hit) * want, hipMemcpyDeviceToHost, side));
  SCN_HIP(hipStreamSynchronize(side));
  *n_written = want;
  return SCN_OK;
}

int scn_collect_signals(scn_plan *p, int slot, uint32_t max_gap, uint32_t first, scn_signal *signals, uint32_t cap, uint32_t *n_signals) {
  int st = check_slot(p, slot);
  if (st) return st;
  if (!n_signals) return scn_fail(SCN_E_INVALID, "null argument");
  *n_signals = 0;
  if (!signals && cap) return scn_fail(SCN_E_INVALID, "null signals with cap %u", cap);
  if (p->d.mode != SCN_MODE_FREQUENCY_DOMAIN) return scn_fail(SCN_E_INVALID, "time-domain plan: it has no hits to merge");
  if (!(p->d.flags & SCN_OUT_HITS)) return scn_fail(SCN_E_INVALID, "plan was created without SCN_OUT_HITS");
  Slot &s = p->slot[slot];
  if ((st = require_list(s.life, slot, "hit list is still on the device"))) return st;
  if (s.life.total_hits == 0) return SCN_OK;
  SCN_HIP(hipSetDevice(p->d.device_id));
  if ((st = fetch_list(p, s, 0))) return st;  // (the hits' offsets come from the scan: wait for it)
  SCN_HIP(s.d_sig_counts.alloc(p->d.max_batch));
  SCN_HIP(s.d_sig_offsets.alloc((size_t)p->d.max_batch + 1u));
  ScnSignalArgs a = {};
  set_list_source(a, p, s);
  a.max_gap = max_gap;
  a.sig_counts = s.d_sig_counts.get();
  a.sig_offsets = s.d_sig_offsets.get();
  ScnCompactArgs scan = compact_args(p, s, 0, 0, nullptr);  // the scan kernel as it is, on the signal counts
  scan.counts = s.d_sig_counts.get();
  scan.offsets = s.d_sig_offsets.get();
  hipStream_t side = topup_stream_of(p, s);  // (nothing queued there: pending slots are not disturbed)
  SCN_HIP(scn_launch_signal_count(a, side));
  SCN_HIP(scn_launch_hit_scan(scan, side));
  uint32_t total = 0;
  SCN_HIP(hipMemcpyAsync(&total, s.d_sig_offsets.get() + s.life.n_buffers, sizeof(uint32_t), hipMemcpyDeviceToHost, side));
  SCN_HIP(hipStreamSynchronize(side));
  *n_signals = total;
  const uint32_t want = first < total ? std::min(cap, total - first) : 0u;
  if (want) {
    if (s.d_sig_window.capacity() < want) SCN_HIP(s.d_sig_window.grow(want));
    a.out = s.d_sig_window.get();
    a.first = first;
    a.out_cap = want;  // (first + want <= total <= the hits' total < 2^31: no wrap)
    SCN_HIP(scn_launch_signal_build(a, side));
    SCN_HIP(hipMemcpyAsync(signals, s.d_sig_window.get(), sizeof(scn_signal) * (size_t)want, hipMemcpyDeviceToHost, side));
    SCN_HIP(hipStreamSynchronize(side));
  }
  if ((uint64_t)first + cap < total)
    return scn_fail(SCN_E_TRUNCATED, "%u signals, records [%u, %u) returned: call again with a later first", total, first, first + want);
  return SCN_OK;
}

int scn_collect_floor(scn_plan *p, int slot, float *floor_db) {
  if (int st = check_slot(p, slot)) return st;
  if (!floor_db) return scn_fail(SCN_E_INVALID, "null argument");
  if (!p->floor) return scn_fail(SCN_E_INVALID, "plan was created without detect = SCN_DETECT_FLOOR");
  Slot &s = p->slot[slot];
  if (int st = require_list(s.life, slot, "floor is still available")) return st;
  if (int st = require_unit_floor(s.life, slot)) return st;
  if (s.life.n_buffers) memcpy(floor_db, s.h_floor.get(), sizeof(float) * s.life.n_buffers);  // (in pinned memory since `done`: scn_collect waited for it)
  return SCN_OK;
}

int scn_hits_view(scn_plan *p, int slot, const scn_hit **hits, uint32_t *n) {
  int st = check_slot(p, slot);
  if (st) return st;
  if (!hits || !n) return scn_fail(SCN_E_INVALID, "null argument");
  Slot &s = p->slot[slot];
  if ((st = require_list(s.life, slot, "hit list is still available"))) return st;
  SCN_HIP(hipSetDevice(p->d.device_id));
  *n = std::min(s.life.total_hits, p->d.max_hits);
  p->view_age = 0;  // (a caller that reads the list through the view wants it built eagerly too)
  p->records_wanted = true;
  if (*n && (st = fetch_list(p, s, *n))) return st;
  *hits = s.h_list.get();
  return SCN_OK;
}

}  // extern "C"

int scn_plan_device_hits(scn_plan *p, int slot, const scn_hit **d_list, uint32_t *n, int *device_id, void **list_ready) {
  int st = check_slot(p, slot);
  if (st) return st;
  if (!d_list || !n) return scn_fail(SCN_E_INVALID, "null argument");
  if (list_ready) *list_ready = nullptr;
  Slot &s = p->slot[slot];
  if ((st = require_list(s.life, slot, "hit list is still on the device"))) return st;
  if (s.life.total_hits > p->d.max_hits)
    return scn_fail(SCN_E_TRUNCATED, "slot %d holds %u hits, the plan's device list %u (max_hits): gather from a host list read with scn_collect_more",
                    slot, s.life.total_hits, p->d.max_hits);
  SCN_HIP(hipSetDevice(p->d.device_id));
  p->device_list_age = 0;  // (a caller that sends the list from the device wants it built eagerly too: behind the launch, on the list
  p->device_list_wanted = true;  // stream, instead of here with the host waiting for it -- 56 us per scn_gather_post against 3, r06_experiments.md)
  if (s.life.total_hits) {
    if (!s.life.list_built)
      if ((st = build_list(p, s, false))) return st;
    if (list_ready) *list_ready = (void *)s.cur().list_done.get();
    else SCN_HIP(hipEventSynchronize(s.cur().list_done.get()));
  }
  *d_list = s.d_list.get();
  *n = s.life.total_hits;
  if (device_id) *device_id = p->d.device_id;
  return SCN_OK;
}
