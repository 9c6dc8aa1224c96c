// scn_submit.hip -- the submit side of the C-ABI: the transform's launch on the slot's stream and what follows it there and on
// the side streams (counts, total, floor, the eager list), the frequency table, the floor window, the baseline, and K1 alone for the
// capture path.
#include <algorithm>
#include <cstring>
#include <vector>

#include "scn_plan.h"

namespace {

// The input, the window and the K4 / K5 epilogue: the fields every transform's argument struct carries under the same names
template <class A>
void set_common_args(A &a, const scn_plan *p, const Slot &s, const void *d_raw, uint32_t nb, float *d_power) {
  a.raw = d_raw;
  a.window = p->d_window.get();
  a.power_db = d_power;
  a.n_buffers = nb;
  a.scale = p->scale;
  a.threshold = p->d.threshold;
  a.dc_ignore = p->d.dc_ignore_bins;
  a.i_lo = p->i_lo;
  a.i_hi = p->i_hi;
  a.hits = s.cur().d_hits.get();
  a.hit_region = p->hit_region;
  a.per_buffer_hits = s.cur().d_buf_hits.get();
}

// The slot's handles for the names of its route (SubmitRoute, scn_host.h)
hipEvent_t end_event_of(const Slot &s) {
  return s.route.end == KernelEnd::Done ? s.done.get() : s.route.end == KernelEnd::KernelDone ? s.kernel_done.get() : nullptr;
}
hipStream_t counts_stream_of(const scn_plan *p, const Slot &s) { return s.route.counts_stream == RouteStream::D2H ? p->d2h_stream.get() : s.stream; }

// Averaged plans: the transform of nb buffers = nb / K groups, one spectrum per group (scn_average.hip)
int launch_average(scn_plan *p, Slot &s, const void *d_raw, uint32_t nb, float *d_power, bool hits) {
  const uint32_t n = p->d.n, ng = nb / p->avg;
  const int kind = (int)p->d.sample_kind;
  if (ng) SCN_HIP(s.d_avg_partial.alloc(scn_avg_partial_floats(n, p->d.max_batch / p->avg, p->num_cus)));
  ScnAvgArgs a;
  memset(&a, 0, sizeof(a));
  a.raw = d_raw;
  a.window = p->d_window.get();
  a.twiddle = p->d_twiddle.get();
  a.tw1_table = p->d_tw1_table.get();
  a.tw1_half = p->d_avg_tw1.get();
  a.tw_half = reinterpret_cast<const double2_scn *>(p->d_avg_tw.get());
  a.partial = s.d_avg_partial.get();
  a.power_db = d_power;
  a.n = n;
  a.n_groups = ng;
  a.k = p->avg;
  a.parts = scn_avg_parts(n, ng, p->avg, p->num_cus);
  a.layout = p->avg_layout == SCN_AVG_SWEEPS ? SCN_AVG_L_SWEEPS : SCN_AVG_L_DWELL;
  a.scale = p->scale;
  a.threshold = p->d.threshold;
  a.p_lo = scn_hit_prefilter(p->d.threshold);
  a.dc_ignore = p->d.dc_ignore_bins;
  a.i_lo = p->i_lo;
  a.i_hi = p->i_hi;
  a.hits = s.cur().d_hits.get();
  a.hit_region = p->hit_region;
  a.per_group_hits = s.cur().d_buf_hits.get();
  SCN_HIP(scn_launch_average(kind, p->d.correct_dc != 0 && kind != SCN_KIND_FLOAT_COMPLEX, hits, d_power != nullptr, a, p->num_cus, s.stream));
  return SCN_OK;
}

// The transform of a submit on the slot's stream: the only code that knows which launcher and which argument struct a path
// uses.  From the slot's route: where a fused kernel stores the counts as well (host_hits, or nullptr), and the event a fused
// kernel's own dispatch packet completes (stop, or nullptr)
int launch_transform(scn_plan *p, Slot &s, const void *d_raw, uint32_t nb, float *d_power) {
  uint32_t *const host_hits = s.route.counts == Counts::Stored ? s.h_buf_hits.get() : nullptr;
  const hipEvent_t stop = s.route.end_in_packet ? end_event_of(s) : nullptr;
  if (!nb) {  // an empty submit launches nothing, on any path: a hits-only floor or baseline plan has then not even a spectrum buffer to
    if (stop) SCN_HIP(hipEventRecord(stop, s.stream));  // name, which the fused launchers refused (tests/test_plan_sequences_gpu.py)
    return SCN_OK;
  }
  const uint32_t n = p->d.n;
  const int kind = (int)p->d.sample_kind;
  // (a floor or baseline plan's transform reports the spectrum only: its hits come from the detect kernel behind it, launch_floor / launch_baseline)
  const bool hits = (p->d.flags & SCN_OUT_HITS) != 0 && !detects_behind(p), dc = p->d.correct_dc != 0;
  if (p->avg > 1u) return launch_average(p, s, d_raw, nb, d_power, hits);
  switch (p->path) {
    case Path::FusedPow2:
    case Path::FusedMixed: {
      ScnFftArgs a;
      memset(&a, 0, sizeof(a));
      set_common_args(a, p, s, d_raw, nb, d_power);
      a.twiddle = p->d_twiddle.get();
      a.tw1_table = p->d_tw1_table.get();
      a.p_lo = scn_hit_prefilter(p->d.threshold);
      a.host_hits = host_hits;
      a.work_counter = s.d_work_counter.get();
      for (uint32_t x = 0; x < 8; x++) a.work_base[x] = s.work_base[x];
      if (p->path == Path::FusedMixed) {
        SCN_HIP(scn_launch_mixed(n, kind, dc, hits, d_power != nullptr, a, p->num_cus, s.stream, stop));
        return SCN_OK;
      }
      // (a hits-only plan handed a caller's spectrum destination runs the full kernel)
      SCN_HIP(scn_launch_fft(n, kind, dc, hits, d_power != nullptr, a, p->num_cus, s.stream, stop));
      if (scn_uses_queue(kind, n))
        for (uint32_t x = 0; x < 8; x++) s.work_base[x] += scn_work_shard_count(nb, x);  // what this launch adds (wrapping, like the device side)
      return SCN_OK;
    }
    case Path::FourStep: {
      if (nb) SCN_HIP(s.d_gen_work[0].alloc(sizeof(float) * 2 * (size_t)n * p->d.max_batch));
      ScnBigArgs a;
      set_common_args(a, p, s, d_raw, nb, d_power);
      a.twiddle = p->d_twiddle.get();
      a.work = s.d_gen_work[0].get();
      a.tw256 = reinterpret_cast<const double2_scn *>(p->d_twiddle64.get());
      a.p_lo = scn_hit_prefilter(p->d.threshold);
      const bool int_dc = dc && p->d.sample_kind != SCN_KIND_FLOAT_COMPLEX;
      if (nb && int_dc) SCN_HIP(s.d_gen_work[1].alloc(sizeof(int) * 2 * (size_t)p->d.max_batch));
      a.dc_sums = int_dc ? reinterpret_cast<int *>(s.d_gen_work[1].get()) : nullptr;
      SCN_HIP(scn_launch_big(n, kind, int_dc, hits, d_power != nullptr, a, p->num_cus, s.stream));
      return SCN_OK;
    }
    case Path::Bluestein: {
      for (int g = 0; g < 2 && nb; g++)
        SCN_HIP(s.d_gen_work[g].alloc(2u * sizeof(double) * (size_t)p->fft_m * p->d.max_batch));
      ScnGenericArgs a;
      set_common_args(a, p, s, d_raw, nb, d_power);
      a.twiddle = p->d_twiddle64.get();
      a.work0 = s.d_gen_work[0].get();
      a.work1 = s.d_gen_work[1].get();
      a.n = n;
      a.m = p->fft_m;
      a.log2m = p->log2m;
      a.chirp = p->d_chirp.get();
      a.bfilter = p->d_bfilter.get();
      SCN_HIP(scn_launch_generic(kind, dc, hits, a, p->num_cus, s.stream));
      return SCN_OK;
    }
    default: return scn_fail(SCN_E_STATE, "the plan has no transform");
  }
}

// The spectrum, the mask and the hit outputs: the fields every detect kernel's argument struct carries under the same names
template <class A>
void set_detect_args(A &a, const scn_plan *p, const Slot &s, const float *d_power, uint32_t nu) {
  memset(&a, 0, sizeof(a));
  a.power_db = d_power;
  a.n = p->d.n;
  a.n_units = nu;
  a.threshold = p->d.threshold;
  a.dc_ignore = p->d.dc_ignore_bins;
  a.i_lo = p->i_lo;
  a.i_hi = p->i_hi;
  a.hits = s.cur().d_hits.get();
  a.hit_region = p->hit_region;
  a.counts = s.cur().d_buf_hits.get();
}

// Floor plans: the detect kernel on the spectrum the transform has just stored, behind it on the slot's stream; nu units
int launch_floor(scn_plan *p, Slot &s, const float *d_power, uint32_t nu) {
  if (p->floor_train) {  // a floor window: every bin against the rank among its own reference cells (scn_floor_local.hip)
    ScnFloorLocalArgs a;
    set_detect_args(a, p, s, d_power, nu);
    a.train = p->floor_train;
    a.guard = p->floor_guard;
    a.permille = p->floor_permille;
    a.need = p->d_floor_need.get();
    SCN_HIP(scn_launch_floor_local(a, p->num_cus, s.stream));
    return SCN_OK;
  }
  ScnFloorArgs a;
  set_detect_args(a, p, s, d_power, nu);
  a.rank = p->floor_rank;
  a.floor_db = s.d_floor.get();
  SCN_HIP(scn_launch_floor(a, p->num_cus, s.stream));
  return SCN_OK;
}

// Baseline plans: the detect kernel in the same place, unit u against row (first + u) % rows of the plan's baseline
int launch_baseline(scn_plan *p, Slot &s, const float *d_power, uint32_t nu, uint32_t first) {
  ScnBaselineArgs a;
  set_detect_args(a, p, s, d_power, nu);
  a.baseline_db = p->d_baseline.get();
  a.rows = p->baseline_rows;
  a.first = first % p->baseline_rows;  // (begin_submit refused a plan without rows)
  SCN_HIP(scn_launch_baseline_detect(a, p->num_cus, s.stream));
  return SCN_OK;
}

// Time-domain plans: one kernel, `done` behind it
int submit_time_domain(scn_plan *p, Slot &s, const void *d_raw, uint32_t nb) {
  s.cur_power = nullptr;
  ScnTdArgs a;
  a.raw = d_raw;
  a.n = p->d.n;
  a.n_buffers = nb;
  a.scale = p->scale;
  a.max_db = s.h_td.get();
  a.min_db = s.h_td.get() + p->d.max_batch;
  SCN_HIP(scn_launch_time_domain((int)p->d.sample_kind, p->d.correct_dc != 0, a, p->num_cus, s.stream));
  SCN_HIP(hipEventRecord(s.done.get(), s.stream));
  on_submitted(s.life);
  return SCN_OK;
}

// Where the transform stores the spectrum: the caller's buffer, the plan's for a caller that collects it, a buffer the caller never
// sees for a hits-only floor or baseline plan (the same spectrum-only transform), or nowhere
int spectrum_destination(scn_plan *p, Slot &s, uint32_t nb, float **d_power) {
  const size_t count = (size_t)p->d.n * p->d.max_batch;
  if (!*d_power && (p->d.flags & SCN_OUT_SPECTRUM)) {
    SCN_HIP(s.d_power.alloc(count));
    *d_power = s.d_power.get();
  }
  s.cur_power = *d_power;  // (what the caller may collect)
  if (detects_behind(p) && !*d_power && nb) {
    SCN_HIP(s.d_detect_power.alloc(count));
    *d_power = s.d_detect_power.get();
  }
  return SCN_OK;
}

// What scn_plan_update_baseline and scn_plan_update_trace fold in once this submit is collected: behind spectrum_destination d_power
// is the buffer the transform writes, for every plan kind (nullptr: a hits-only submit that stores no spectrum)
void note_spectrum_source(Slot &s, const float *d_power, uint32_t nb, uint32_t table_first) {
  s.spec_power = d_power;
  s.spec_units = nb;
  s.spec_first = table_first;
}

// A submit with hits takes the slot's other generation and leaves its header fields where the compaction kernel reads them
int stage_headers(scn_plan *p, Slot &s, uint32_t nb, const double *fc, const uint64_t *seq, uint32_t table_first) {
  // this submit's generation; the only thing that can still be using it is the list (compaction + copy) of the submit TWO
  // submits back ON THIS SLOT -- 2 x (slots in use) launches back on the plan -- wait for it on the host, where it never
  // blocks in practice
  // -- and the list of the submit before this one on this slot, whose compaction output (d_list) and pinned copy (h_list)
  // exist once per slot: its prefetch DMA rides the D2H stream, which nothing on the list stream is ordered behind, so the
  // next compaction must not start while it may still be reading d_list (a caller that collected counts only has not
  // waited for it).  Both waits are host-side queries of events that completed long ago in any steady loop.
  s.gen ^= 1u;
  for (const SlotGen &g : s.gen_state)
    if (g.list_used && hipEventQuery(g.list_done.get()) != hipSuccess) SCN_HIP(hipEventSynchronize(g.list_done.get()));
  // the header fields: read by the compaction kernel in place, over PCIe (two 8-byte reads per buffer that has hits;
  // staging copies cost ~7 us each plus ~10 us of cross-engine hand-off, on the list's critical path)
  // the centres: copied when given; a submit that names a range of the plan's device-resident table writes none (the other
  // 8 header bytes per buffer: 2 MB per launch of 262144 128-point buffers, written and then read back over PCIe)
  s.cur().table_first = fc ? -1 : (int64_t)table_first;
  if (fc) memcpy(s.centres(p->d.max_batch), fc, sizeof(double) * nb);
  // sequence ids: copied when given; otherwise a buffer's id is its index and the compaction kernel computes it -- 8 of the
  // 16 header bytes per buffer that made the 16 .. 128-point steps host-bound (524288 buffers per launch: 4 MB less to write)
  s.cur().seq_given = seq != nullptr;
  if (seq) memcpy(s.seq_ids(p->d.max_batch), seq, sizeof(uint64_t) * nb);
  return SCN_OK;
}

// What follows the submit's last compute kernel: the slot's route (submit_route, scn_host.hip), executed
int queue_behind_transform(scn_plan *p, Slot &s, uint32_t nb) {
  const SubmitRoute &r = s.route;
  const hipEvent_t end = end_event_of(s);
  const hipStream_t cnt = counts_stream_of(p, s);
  if (end && !r.end_in_packet) SCN_HIP(hipEventRecord(end, s.stream));
  if (cnt != s.stream) SCN_HIP(hipStreamWaitEvent(cnt, end, 0));
  if (r.list_forks) SCN_HIP(hipStreamWaitEvent(p->list_stream.get(), end, 0));
  if (r.counts == Counts::Reduced)
    SCN_HIP(scn_launch_hit_total(s.cur().d_buf_hits.get(), nb, p->d.trigger_count, s.d_total_acc.get(), s.h_total, s.h_buf_hits.get(), cnt));
  if (r.counts == Counts::Dma)
    SCN_HIP(hipMemcpyAsync(s.h_buf_hits.get(), s.cur().d_buf_hits.get(), sizeof(uint32_t) * nb, hipMemcpyDeviceToHost, cnt));
  // (the way the counts go; a windowed submit has no per-unit floor)
  if (p->floor && r.counts != Counts::None && !s.life.floor_windowed)
    SCN_HIP(hipMemcpyAsync(s.h_floor.get(), s.d_floor.get(), sizeof(float) * nb, hipMemcpyDeviceToHost, cnt));
  if (r.done_behind_counts) SCN_HIP(hipEventRecord(s.done.get(), cnt));
  if (r.list_behind)  // (the prefetch to pinned memory only for a caller that reads the records on the host)
    return build_list(p, s, p->records_wanted);
  return SCN_OK;
}

// fc == nullptr: the buffers carry entries table_first, table_first + 1, ... (wrapping) of the plan's frequency table
int submit_common(scn_plan *p, Slot &s, const void *d_raw, uint32_t nb, const double *fc, const uint64_t *seq,
                  float *d_power, uint32_t table_first = 0) {
  // Averaged plans: from here on nb counts GROUPS -- the outputs, the records' headers, the counts and triggers are per group --
  // and only the transform sees the buffers.  A group's header is that of its first buffer.
  const uint32_t n_raw = nb;
  std::vector<double> group_fc;
  std::vector<uint64_t> group_seq;
  if (p->avg > 1u) nb = group_headers(p->avg, p->avg_layout == SCN_AVG_SWEEPS, nb, fc, seq, group_fc, group_seq);
  const bool hits = (p->d.flags & SCN_OUT_HITS) != 0;
  const SubmitFacts facts = {nb, hits, p->floor && p->floor_train != 0u, p->baseline, p->d.mode == SCN_MODE_TIME_DOMAIN};
  int st = ensure_slot_outputs(p, s, submit_flips(facts) ? s.gen ^ 1u : s.gen);
  if (st) return st;
  if (facts.time_domain) {
    on_submit(s.life, facts);
    return submit_time_domain(p, s, d_raw, nb);
  }
  if ((st = spectrum_destination(p, s, nb, &d_power))) return st;
  note_spectrum_source(s, d_power, nb, table_first);
  if (on_submit(s.life, facts) && (st = stage_headers(p, s, nb, fc, seq, table_first))) return st;
  // what follows the transform, decided once (submit_route, scn_host.hip: the table and the measurements behind it)
  const bool fused = (p->path == Path::FusedPow2 || p->path == Path::FusedMixed) && p->avg == 1u && !detects_behind(p);
  s.route = submit_route({hits, fused, p->direct_counts, s.own_stream, p->records_wanted || p->device_list_wanted, p->d.n, nb});
  if ((st = launch_transform(p, s, d_raw, n_raw, d_power))) return st;
  if (p->floor && nb && (st = launch_floor(p, s, d_power, nb))) return st;
  if (p->baseline && nb && (st = launch_baseline(p, s, d_power, nb, table_first))) return st;
  if ((st = queue_behind_transform(p, s, nb))) return st;
  on_submitted(s.life);
  return SCN_OK;
}

// What every submit checks before anything is queued, in this order: the batch's size, the entry point's own pointers, the averaged
// plan's grouping, a baseline plan's rows (`indexed`: against the table), the slot (free; `host`: its staging buffer exists) -- then the
// plan's device is current and the slot's stream exists
int begin_submit(scn_plan *p, int slot, uint32_t nb, const double *fc, bool null_argument, bool host, bool indexed) {
  Slot &s = p->slot[slot];
  if (nb > p->d.max_batch) return scn_fail(SCN_E_INVALID, "n_buffers %u > max_batch %u", nb, p->d.max_batch);
  if (null_argument) return scn_fail(SCN_E_INVALID, "null argument");
  if (p->avg > 1u)
    if (int st = check_average(p->avg, p->avg_layout == SCN_AVG_SWEEPS, nb, fc)) return st;
  if (p->baseline)
    if (int st = check_baseline_submit(p->baseline_rows, indexed, p->table_count)) return st;
  if (int st = require_free(s.life, slot)) return st;
  if (host && !s.h_raw) return scn_fail(SCN_E_STATE, "slot %d: scn_host_buffer was never called", slot);
  SCN_HIP(hipSetDevice(p->d.device_id));
  return ensure_slot_stream(p, s);
}

// the pinned slot's buffers -> the GPU -> the kernels; fc == nullptr: entries first_index ... of the plan's frequency table
int submit_host(scn_plan *p, int slot, uint32_t nb, const double *fc, const uint64_t *seq, uint32_t first_index, bool indexed) {
  if (int st = begin_submit(p, slot, nb, fc, false, true, indexed)) return st;
  Slot &s = p->slot[slot];
  SCN_HIP(s.d_raw.alloc(p->buf_bytes * p->d.max_batch));
  if (nb) {
    // stage on the h2d stream so this copy overlaps the other slot's kernel; the compute stream
    // picks it up through an event
    SCN_HIP(s.staged.create());
    SCN_HIP(hipMemcpyAsync(s.d_raw.get(), s.h_raw.get(), p->buf_bytes * nb, hipMemcpyHostToDevice, p->h2d_stream.get()));
    SCN_HIP(hipEventRecord(s.staged.get(), p->h2d_stream.get()));
    SCN_HIP(hipStreamWaitEvent(s.stream, s.staged.get(), 0));
  }
  return submit_common(p, s, s.d_raw.get(), nb, fc, seq, nullptr, first_index);
}

int check_indexed(scn_plan *p, uint32_t nb, uint32_t first_index) {
  if (p->d.mode == SCN_MODE_TIME_DOMAIN || !(p->d.flags & SCN_OUT_HITS)) return SCN_OK;  // no records: nothing reads the table
  if (nb && !p->table_count) return scn_fail(SCN_E_STATE, "scn_plan_set_table was never called");
  if (nb && first_index >= p->table_count) return scn_fail(SCN_E_INVALID, "first_index %u outside the table of %u entries", first_index, p->table_count);
  return SCN_OK;
}

}  // namespace

extern "C" {

int scn_submit(scn_plan *p, int slot, uint32_t nb, const double *fc, const uint64_t *seq) {
  if (int st = check_slot(p, slot)) return st;
  if (nb && !fc) return scn_fail(SCN_E_INVALID, "center_freqs is null");
  return submit_host(p, slot, nb, fc, seq, 0, false);
}

int scn_submit_device(scn_plan *p, int slot, const void *d_raw, uint32_t nb, const double *fc, const uint64_t *seq,
                      float *d_power_db) {
  int st = check_slot(p, slot);
  if (st) return st;
  if ((st = begin_submit(p, slot, nb, fc, nb && (!fc || !d_raw), false, false))) return st;
  return submit_common(p, p->slot[slot], d_raw, nb, fc, seq, d_power_db);
}

int scn_submit_indexed(scn_plan *p, int slot, uint32_t nb, uint32_t first_index, const uint64_t *seq) {
  int st = check_slot(p, slot);
  if (st) return st;
  if ((st = check_indexed(p, nb, first_index))) return st;
  return submit_host(p, slot, nb, nullptr, seq, first_index, true);
}

int scn_submit_device_indexed(scn_plan *p, int slot, const void *d_raw, uint32_t nb, uint32_t first_index, const uint64_t *seq,
                              float *d_power_db) {
  int st = check_slot(p, slot);
  if (st) return st;
  if ((st = check_indexed(p, nb, first_index))) return st;
  if ((st = begin_submit(p, slot, nb, nullptr, nb && !d_raw, false, true))) return st;
  return submit_common(p, p->slot[slot], d_raw, nb, nullptr, seq, d_power_db, first_index);
}

int scn_plan_set_table(scn_plan *p, const double *fc, uint32_t count) {
  if (!p) return scn_fail(SCN_E_INVALID, "null plan");
  if (count && !fc) return scn_fail(SCN_E_INVALID, "center_freqs is null");
  const SlotLives lives = lives_of(p);
  if (int st = require_none_pending(lives.life, SCN_NUM_SLOTS, ": its records still read the table")) return st;
  SCN_HIP(hipSetDevice(p->d.device_id));
  // (a list of an already collected submit may still be being completed -- the prefetch of scn_collect, scn_collect_more --
  // from the OLD table: wait for what THIS plan has queued on the streams that read the table, then forget those lists.  Not a
  // device-wide synchronisation: other plans' pipelines and the caller's own streams on this GPU go on undisturbed.)
  SCN_HIP(hipStreamSynchronize(p->list_stream.get()));
  SCN_HIP(hipStreamSynchronize(p->d2h_stream.get()));
  SCN_HIP(hipStreamSynchronize(p->h2d_stream.get()));
  for (int i = 0; i < SCN_NUM_SLOTS; i++)  // (a slot with a stream of its own builds its list there)
    if (p->slot[i].own_stream && p->slot[i].stream) SCN_HIP(hipStreamSynchronize(p->slot[i].stream));
  on_table_change(lives.life, SCN_NUM_SLOTS);
  p->table_count = 0;
  if (!count) return SCN_OK;
  if (count > p->d_table.capacity()) SCN_HIP(p->d_table.grow(count));  // (a caller that re-tables between sweeps keeps its allocation)
  SCN_HIP(hipMemcpyAsync(p->d_table.get(), fc, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, p->list_stream.get()));
  SCN_HIP(hipStreamSynchronize(p->list_stream.get()));  // (fc is the caller's: done with it before returning; the list kernels run on this stream, after the copy)
  p->table_count = count;
  return SCN_OK;
}

int scn_plan_set_floor_window(scn_plan *p, uint32_t train, uint32_t guard) {
  if (!p) return scn_fail(SCN_E_INVALID, "null plan");
  if (!p->floor) return scn_fail(SCN_E_INVALID, "plan was created without detect = SCN_DETECT_FLOOR");
  if (int st = require_none_pending(lives_of(p).life, SCN_NUM_SLOTS, "")) return st;
  if (!train && !guard) {  // back to the unit-wide floor (collected slots keep their lists: nothing of theirs reads the table)
    p->floor_train = p->floor_guard = 0;
    return SCN_OK;
  }
  std::vector<uint16_t> need;
  if (int st = floor_window_ranks(p->d.n, p->d.dc_ignore_bins, p->i_lo, p->i_hi, p->floor_permille, train, guard, need)) return st;
  need.resize(((size_t)p->d.n + 3u) & ~(size_t)3u, 0);  // (whole 8-byte reads: ScnFloorLocalArgs::need)
  SCN_HIP(hipSetDevice(p->d.device_id));
  // (no slot is pending, and a slot's detect kernel is complete when its `done` is: nothing reads the old table any more)
  SCN_HIP(p->d_floor_need.alloc(need.size()));
  SCN_HIP(hipMemcpy(p->d_floor_need.get(), need.data(), sizeof(uint16_t) * need.size(), hipMemcpyHostToDevice));
  p->floor_train = train;
  p->floor_guard = guard;
  return SCN_OK;
}

int scn_plan_set_baseline(scn_plan *p, uint32_t rows, const float *baseline_db) {
  if (!p) return scn_fail(SCN_E_INVALID, "null plan");
  if (!p->baseline) return scn_fail(SCN_E_INVALID, "plan was created without detect = SCN_DETECT_BASELINE");
  if (int st = require_none_pending(lives_of(p).life, SCN_NUM_SLOTS, ": its detect kernel may still read the baseline")) return st;
  // (no slot is pending, and a slot's detect kernel is complete when its `done` is: nothing reads the old rows any more)
  p->baseline_rows = 0;
  if (!rows) return SCN_OK;  // (the allocation stays for the next one, as the table's)
  const size_t count = (size_t)rows * p->d.n;
  SCN_HIP(hipSetDevice(p->d.device_id));
  if (count > p->d_baseline.capacity()) SCN_HIP(p->d_baseline.grow(count));
  if (baseline_db) SCN_HIP(hipMemcpyAsync(p->d_baseline.get(), baseline_db, sizeof(float) * count, hipMemcpyHostToDevice, p->stream.get()));
  else SCN_HIP(hipMemsetD32Async((hipDeviceptr_t)p->d_baseline.get(), 0x7f800000, count, p->stream.get()));  // +inf
  SCN_HIP(hipStreamSynchronize(p->stream.get()));  // (baseline_db is the caller's: done with it before returning; slots with a stream of their own start behind this)
  p->baseline_rows = rows;
  return SCN_OK;
}

int scn_plan_update_baseline(scn_plan *p, int slot, uint32_t op) {
  if (int st = check_slot(p, slot)) return st;
  if (!p->baseline) return scn_fail(SCN_E_INVALID, "plan was created without detect = SCN_DETECT_BASELINE");
  if (int st = require_none_pending(lives_of(p).life, SCN_NUM_SLOTS, ": its detect kernel may still read the baseline")) return st;
  const Slot &s = p->slot[slot];
  if (int st = require_learnable(s.life, slot)) return st;
  if (!p->baseline_rows) return scn_fail(SCN_E_STATE, "the plan has no baseline: scn_plan_set_baseline was never called, or dropped it");
  if (int st = check_baseline_update(p->baseline_rows, s.spec_units, op)) return st;
  if (!s.spec_units) return SCN_OK;
  SCN_HIP(hipSetDevice(p->d.device_id));
  ScnBaselineArgs a;
  memset(&a, 0, sizeof(a));
  a.power_db = s.spec_power;  // (complete: the slot's collect waited for the detect kernel behind the transform that wrote it)
  a.baseline_db = p->d_baseline.get();
  a.n = p->d.n;
  a.n_units = s.spec_units;
  a.rows = p->baseline_rows;
  a.first = s.spec_first % p->baseline_rows;
  a.op = op;
  SCN_HIP(scn_launch_baseline_update(a, p->stream.get()));
  SCN_HIP(hipStreamSynchronize(p->stream.get()));
  return SCN_OK;
}

int scn_plan_get_baseline(scn_plan *p, uint32_t first_row, uint32_t rows, float *out) {
  if (!p) return scn_fail(SCN_E_INVALID, "null plan");
  if (!p->baseline) return scn_fail(SCN_E_INVALID, "plan was created without detect = SCN_DETECT_BASELINE");
  if (int st = check_baseline_range(p->baseline_rows, first_row, rows)) return st;
  if (!rows) return SCN_OK;
  if (!out) return scn_fail(SCN_E_INVALID, "null argument");
  SCN_HIP(hipSetDevice(p->d.device_id));
  const size_t n = p->d.n;
  SCN_HIP(hipMemcpyAsync(out, p->d_baseline.get() + (size_t)first_row * n, sizeof(float) * (size_t)rows * n, hipMemcpyDeviceToHost, p->stream.get()));
  SCN_HIP(hipStreamSynchronize(p->stream.get()));
  return SCN_OK;
}

int scn_convert_raw(scn_plan *p, const void *raw, uint32_t nb, float *out) {
  if (!p || (nb && (!raw || !out))) return scn_fail(SCN_E_INVALID, "null argument");
  if (!nb) return SCN_OK;
  SCN_HIP(hipSetDevice(p->d.device_id));
  const size_t in_bytes = p->buf_bytes * nb, out_bytes = sizeof(float) * 2 * (size_t)p->d.n * nb;
  if (p->d_conv_out.capacity() < (size_t)p->d.n * nb) {  // grow the plan's staging pair (the capture writer converts one record per call: one
    p->d_conv_in.reset();                                // allocation, ever); the output, allocated last, vouches for both
    p->d_conv_out.reset();
    SCN_HIP(p->d_conv_in.alloc(in_bytes));
    SCN_HIP(p->d_conv_out.alloc((size_t)p->d.n * nb));
  }
  SCN_HIP(hipMemcpyAsync(p->d_conv_in.get(), raw, in_bytes, hipMemcpyHostToDevice, p->d2h_stream.get()));
  SCN_HIP(scn_launch_convert((int)p->d.sample_kind, p->d.correct_dc != 0, p->d_conv_in.get(), p->d_conv_out.get(), p->d.n, nb, p->scale, p->d2h_stream.get()));
  SCN_HIP(hipMemcpyAsync(out, p->d_conv_out.get(), out_bytes, hipMemcpyDeviceToHost, p->d2h_stream.get()));
  SCN_HIP(hipStreamSynchronize(p->d2h_stream.get()));
  return SCN_OK;
}

}  // extern "C"
