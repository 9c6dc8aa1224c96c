// scn_plan.h -- what the units of the C-ABI layer share: the plan and its slots, and the helpers more than one of them calls.
// scn_sizes.h: which sizes each kernel family takes, the path of a size (no HIP header).  scn_host.hip: arithmetic and entry points that
// never touch HIP -- a descriptor's defaults, checks and everything derived from it (resolve_plan, resolve_welch) and the contents of
// the tables; scn_plan.hip: the device side of create (streams, uploads), first-use allocation, destroy, getters;
// scn_slot_life.h: what a slot may do next -- every precondition and every transition of its life cycle (no HIP header);
// scn_submit.hip / scn_collect.hip: the two sides of a slot; scn_history_plan.hip: the hit history; scn_trace_plan.hip: the sweep trace;
// scn_welch_plan.hip: the Welch plan.
//
// A plan owns: one HIP stream, the window and twiddle tables, and SCN_NUM_SLOTS independent result slots (double buffering:
// the host fills / drains one slot while the GPU works on the other -- the replacement for the reference's MemoryPool + bounded
// queue, memoryPool.h:32-77 / messageQueue.h:65-91).  No call blocks on the GPU except scn_collect / scn_wait / scn_plan_destroy.
// Ownership is in the types: a ScnDeviceMem / ScnPinnedMem / ScnEvent / ScnStream member (scn_resource.h) owns what it holds
// and releases it with the plan; a raw pointer or hipStream_t borrows.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "scn_host.h"
#include "scn_kernels.h"
#include "scn_resource.h"
#include "scn_slot_life.h"

#define SCN_HIP(call)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return scn_fail(e_ == hipErrorOutOfMemory ? SCN_E_NOMEM : SCN_E_HIP, "%s failed: %s", #call, \
                      hipGetErrorString(e_));                                                      \
  } while (0)

// Everything the FFT kernel writes for the hit list has TWO generations per slot, alternating per submit: the
// compaction of submit k may still be running (beside launch k+1) when launch k+2 starts writing -- with a
// generation of its own nothing has to wait, neither the host at submit nor the compute stream behind a barrier
// packet (measured: ~10 us per launch even when the barrier is already satisfied, ~16 us when it is not).
struct SlotGen {
  ScnDeviceMem<ScnDevHit> d_hits;     // [max_batch][hit_region] per-buffer hit regions (unordered, scn_kernels.hip)
  ScnDeviceMem<uint32_t> d_buf_hits;  // [max_batch] hits per buffer
  ScnEvent list_done;                 // scan + compaction (+ prefetch) finished
  bool list_used = false;             // ... and whether that event has ever been recorded
  bool seq_given = false;             // the submit came with sequence ids (else: the buffer's index)
  int64_t table_first = -1;           // the submit named a range of the plan's frequency table (else -1: its own centres in h_meta)
};

struct Slot {
  ScnStream owned_stream;           // SCN_PLAN_OVERLAP_SLOTS, slots 1 ... : `stream` below when own_stream (first: destroyed last)
  ScnDeviceMem<char> d_gen_work[2];  // scratch of the four-step and Bluestein paths (launch_transform)
  ScnDeviceMem<float> d_avg_partial;  // averaged plans: the partial power sums between the two kernels of scn_average.hip
  ScnPinnedMem<char> h_raw;         // pinned staging, max_batch raw buffers
  ScnDeviceMem<char> d_raw;         // device copy of the staging slot
  ScnDeviceMem<float> d_power;      // [max_batch][N] dB spectra (plan-owned destination)
  float *cur_power = nullptr;       // destination of the pending submit (d_power or the caller's; nullptr: the caller collects none)
  ScnPinnedMem<float> h_td;         // time-domain mode: [2][max_batch] max / min dB, pinned, kernel-written
  SlotGen gen_state[2];             // the hit outputs, one record per generation
  uint32_t gen = 0;                 // generation of the pending / last submit
  SlotGen &cur() { return gen_state[gen]; }
  const SlotGen &cur() const { return gen_state[gen]; }
  // [max_batch] hits per buffer.  The kernel writes device memory (SlotGen::d_buf_hits); a 4*n_buffers-byte D2H copy on
  // the plan's d2h stream (ordered behind the kernel by an event) brings them to the pinned copy,
  // so the compute stream carries nothing but the kernel.  (Letting the kernel store to pinned
  // host memory directly was measured: the PCIe acknowledgements delay every kernel's completion
  // by ~4 us, 5 % of a C2 launch.)
  ScnPinnedMem<uint32_t> h_buf_hits;
  unsigned long long *h_total = nullptr;  // pinned (the tail of h_buf_hits): the batch's total, stored by scn_hit_total_kernel
  ScnDeviceMem<unsigned long long> d_total_acc;  // its two device words
  // the route of the pending / last submit.  counts == Counts::Reduced: its total is (going to be) in *h_total and its trigger flags, one
  // bit per buffer, in the front of h_buf_hits: the counts themselves stayed on the GPU and scn_collect walks nothing
  SubmitRoute route;
  ScnEvent kernel_done, staged;
  hipStream_t stream = nullptr;     // where this slot's kernels run: the plan's compute stream, or its own (SCN_PLAN_OVERLAP_SLOTS)
  // buffer-queue heads of the persistent workgroups (ScnFftArgs::work_counter; 8 heads, never reset) and their values
  // before the next launch (host-tracked).  Per slot: with overlapped slots two launches pull concurrently.
  ScnDeviceMem<uint32_t> d_work_counter;
  uint32_t work_base[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool own_stream = false;
  // the ordered list (scn_hits.hip): offsets = exclusive scan of the counts; h_meta = the submit's MessageHeader
  // fields, pinned, read by the compaction kernel in place; d_list = the first max_hits completed records; h_list =
  // their pinned host copy (prefetched of them are there); d_window = where scn_collect_more re-runs the compaction
  // for a window beyond max_hits
  ScnDeviceMem<uint32_t> d_offsets;
  ScnPinnedMem<double> h_meta;      // pinned, two generations of {[max_batch] doubles, [max_batch] u64}: the current one's arrays
  double *centres(uint32_t max_batch) const { return h_meta.get() + (size_t)2u * max_batch * gen; }
  uint64_t *seq_ids(uint32_t max_batch) const { return reinterpret_cast<uint64_t *>(centres(max_batch) + max_batch); }
  ScnDeviceMem<scn_hit> d_list;     // device [max_hits]
  ScnPinnedMem<scn_hit> h_list;     // pinned [max_hits]
  uint32_t prefetched = 0;          // leading records of the current list that are (being) copied to h_list
  ScnDeviceMem<scn_hit> d_window;   // scratch of scn_collect_more, grown on demand
  // scn_collect_signals: signals per unit and their exclusive scan ([max_batch], [max_batch + 1]; allocated at the first call),
  // and the window of records the build kernel writes before they are copied out (grown on demand, like d_window)
  ScnDeviceMem<uint32_t> d_sig_counts, d_sig_offsets;
  ScnDeviceMem<scn_signal> d_sig_window;
  // scn_collect_confirmed: confirmed records per unit and their exclusive scan, and the window of records the build kernel writes
  // (the same three, allocated and grown the same way)
  ScnDeviceMem<uint32_t> d_conf_counts, d_conf_offsets;
  ScnDeviceMem<scn_hit> d_conf_window;
  // floor-detector plans (scn_floor.hip): floor_db of the pending / last submit's units, kernel-written device memory and the pinned
  // copy a DMA behind the counts' brings (scn_collect_floor reads it).  ONE generation of each is enough, unlike the regions and
  // counts: the only reader of d_floor is that DMA, which is complete when `done` is -- and a slot is not submitted again before
  // its collect has waited for `done` --, and h_floor is promised only until the slot's next submit.
  ScnDeviceMem<float> d_floor;      // [max_batch]
  ScnPinnedMem<float> h_floor;      // [max_batch]
  ScnDeviceMem<float> d_detect_power;  // [max_batch][N] the spectrum the detect kernel reads when the caller keeps none (hits-only floor / baseline plans)
  // what scn_plan_update_baseline and scn_plan_update_trace need of the slot's last submit: the spectrum its transform stored (the
  // caller's buffer, d_power or d_detect_power: still intact, the slot's next submit is what overwrites it; nullptr: it stored
  // none), its units and its first_index
  const float *spec_power = nullptr;
  uint32_t spec_units = 0, spec_first = 0;
  ScnEvent done;
  SlotLife life;                    // what the slot may do next (scn_slot_life.h): written by its on_* functions only
};

// Where the ordered hit list of a submit is built: behind the kernel on the list stream, overlapping the next launch (plus a
// DMA of the expected number of records to pinned host memory), IF the plan's previous collect asked for records; otherwise
// on demand, when a collect call asks -- callers that only want counts / trigger flags pay nothing.  (Measured alternatives,
// profiles/r02_compact_modes5.txt: always in order on the compute stream costs 60 us per step; always on demand puts the
// list on the caller's critical path.)
// What the descriptor alone decides -- d, path, avg, the mask, hit_region, the detector's numbers, direct_counts -- is the PlanShape
// that resolve_plan made (scn_host.h); the rest is what the plan owns on the device and what its collects have learned.
struct scn_plan : PlanShape {
  // (the streams first: destroyed after the slots, the memory and the events that were used on them)
  ScnStream stream;       // compute
  ScnStream h2d_stream;   // staging copies of scn_submit (overlap the other slot's kernel)
  ScnStream d2h_stream;   // per-buffer hit counts back to the host
  ScnStream list_stream;  // the ordered hit list: scan + compaction kernels, the list's DMA
  int num_cus = 0;
  bool records_wanted = false;  // does the caller take hit records? (decides where the next list is built: scn_collect sets it)
  // Callers that read the records in place (scn_collect for the counts, then scn_hits_view -- only when there ARE hits) never
  // pass scn_collect a record buffer: the view marks the plan, and the mark wears off after four collects in a row that had
  // hits and were not followed by a view.  (Until round 5 every scn_collect without a buffer cleared records_wanted, so after
  // any batch without a detection the next submit was not eager and the first batch with hits built its list on demand, on
  // the consumer's critical path.)
  uint32_t view_age = 0xffffffffu;  // collects with hits since the last scn_hits_view (saturating; "never" at first)
  uint32_t device_list_age = 0xffffffffu;  // ... since the last scn_gather_hits_device / scn_gather_post took a slot's list where it lies
  bool device_list_wanted = false;         // the ordered list is built behind every launch, without the prefetch to pinned memory
  uint32_t predict = 0;         // records the next list is expected to hold (last total + a margin, scn_collect): the prefetch size
  uint32_t last_total = 0;      // the total before that: the margin grows with the change between consecutive batches
  // the floor window (scn_plan_set_floor_window, scn_floor_local.hip): train 0 = none, the unit-wide floor above; with one, the
  // table r_i + 1 by fftshift index (floor_window_ranks), padded with zeros to a multiple of 4 entries
  uint32_t floor_train = 0, floor_guard = 0;
  ScnDeviceMem<uint16_t> d_floor_need;
  // baseline plans: what scn_baseline.hip detects against, [baseline_rows][n] (scn_plan_set_baseline; kept allocated when dropped, as d_table)
  ScnDeviceMem<float> d_baseline;
  uint32_t baseline_rows = 0;  // 0: none, every submit is refused
  // the hit history (scn_history.hip; scn_plan_set_history, kept allocated when dropped): [history_rows][n] words by fftshift index
  // and [history_rows] visits.  No kernel of a submit reads or writes them -- only scn_plan_update_history and
  // scn_collect_confirmed, which both return synchronised --, so they may change while other slots are pending.
  ScnDeviceMem<uint32_t> d_history, d_visits;
  uint32_t history_rows = 0;   // 0: none
  uint64_t history_epoch = 0;  // grows with every fold and every scn_plan_set_history: a slot's confirmed list is that of the plan's LATEST fold
  // the sweep trace (scn_trace.hip; scn_plan_set_trace, kept allocated when dropped): per cell the keys of max_db and min_db
  // (scn_trace.h; unkeyed at read-out) and the count.  As the history: only scn_plan_update_trace writes them, and it returns
  // synchronised, so they may change while other slots are pending.
  ScnDeviceMem<uint32_t> d_trace_max, d_trace_min;
  ScnDeviceMem<unsigned long long> d_trace_count;
  uint64_t trace_f0 = 0;
  uint32_t trace_cell_hz = 0, trace_cells = 0;  // cells 0: none
  // the trace emitters (scn_emitters.hip; scn_plan_trace_emitters, scn_plan_merge_trace), each allocated at the first call that needs
  // it and grown on demand: the tiles' five arrays and the total ([5 * kEmitTilesMax + 1]), an accumulator per emitter of the window,
  // the page of records that goes to the host; and what a merge uploads ([2][cells] float bits, [cells] counts)
  ScnDeviceMem<uint32_t> d_emit_tiles, d_merge_bits;
  ScnDeviceMem<ScnEmitterAcc> d_emit_acc;
  ScnDeviceMem<scn_emitter> d_emit_page;
  ScnDeviceMem<unsigned long long> d_merge_count;
  // the level histogram (scn_levels.hip; scn_plan_set_levels, kept allocated when dropped): the counters [cells][n_edges + 1], the
  // table's padded keys as the fold kernel stages them (scn_levels.h), and the summary kernel's outputs, grown to the largest
  // window asked for.  Written as the trace is: by calls that return synchronised only.
  ScnDeviceMem<unsigned long long> d_levels_hist, d_levels_sums;  // sums: [2][window] above, total
  ScnDeviceMem<uint32_t> d_levels_keys, d_levels_rank;
  uint64_t levels_f0 = 0;
  uint32_t levels_cell_hz = 0, levels_cells = 0, levels_edges = 0;  // cells 0: none
  uint32_t fft_m = 0, log2m = 0;     // Bluestein: the transform length, the power of two >= 2n - 1
  ScnDeviceMem<double> d_twiddle64;  // four-step: [256][2] W_256^k; Bluestein: [fft_m][2] W_m^k; in double
  ScnDeviceMem<double> d_table;      // the plan's frequency table (scn_plan_set_table), read by the compaction kernel; grown on demand
  uint32_t table_count = 0;          // entries in use
  ScnDeviceMem<double> d_chirp;      // Bluestein: [n][2], w[i] = exp(-i pi i^2 / n)
  ScnDeviceMem<double> d_bfilter;    // Bluestein: [fft_m][2], FFT_m of the chirp filter / m
  std::vector<float> h_window;
  ScnDeviceMem<float> d_window;
  ScnDeviceMem<scn_v2f> d_twiddle;
  ScnDeviceMem<scn_v2f> d_tw1_table;  // [15][n/16], ScnFftArgs::tw1_table
  ScnDeviceMem<scn_v2f> d_avg_tw1;    // averaged 8192-point plans: ScnAvgArgs::tw1_half ([15][256], W_4096^(t p))
  ScnDeviceMem<double> d_avg_tw;      // ... and ScnAvgArgs::tw_half ([4096][2], W_8192^k in double)
  // scn_convert_raw's device staging (the capture writer calls it per record): plan-owned, grown on demand, never per call
  ScnDeviceMem<char> d_conv_in;
  ScnDeviceMem<scn_v2f> d_conv_out;
  Slot slot[SCN_NUM_SLOTS];
};

// `count` elements of D in device memory, filled from v (a synchronous copy: plan creation only)
template <class D, class T>
hipError_t upload(ScnDeviceMem<D> &dst, const std::vector<T> &v) {
  const hipError_t e = dst.alloc(v.size() * sizeof(T) / sizeof(D));
  return e != hipSuccess ? e : hipMemcpy(dst.get(), v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
}

// the plan's slots as the plan-wide functions of scn_slot_life.h take them
struct SlotLives {
  SlotLife *life[SCN_NUM_SLOTS];
};
inline SlotLives lives_of(scn_plan *p) {
  SlotLives l;
  for (int i = 0; i < SCN_NUM_SLOTS; i++) l.life[i] = &p->slot[i].life;
  return l;
}

// scn_plan.hip
int check_slot(scn_plan *p, int slot);
int ensure_slot_stream(scn_plan *p, Slot &s);
int ensure_slot_outputs(scn_plan *p, Slot &s, uint32_t gen);

// scn_collect.hip
// What the list kernels, the signal kernels and the confirm kernels read of a slot's pending / last submit, under the same names in
// every argument struct: the regions, the hits' offsets, and the submit's header fields where they lie (the slot's pinned copy or the
// plan's table)
// ... of which the centres alone (the trace's fold reads the spectrum, not the regions)
template <class A>
void set_centre_source(A &a, const scn_plan *p, const Slot &s) {
  const SlotGen &g = s.cur();
  const bool table = g.table_first >= 0;
  a.center_freq = table ? p->d_table.get() : s.centres(p->d.max_batch);
  a.table_count = table ? p->table_count : 0u;
  a.table_first = table ? (uint32_t)g.table_first : 0u;
}
template <class A>
void set_list_source(A &a, const scn_plan *p, const Slot &s) {
  const SlotGen &g = s.cur();
  a.regions = g.d_hits.get();
  a.hit_region = p->hit_region;
  a.offsets = s.d_offsets.get();
  set_centre_source(a, p, s);
  a.seq_id = g.seq_given ? s.seq_ids(p->d.max_batch) : nullptr;
  a.n_buffers = s.life.n_buffers;
  a.n = p->d.n;
  a.sample_rate = p->d.sample_rate;
}
// where work on an already complete list goes (top-up copies, scn_collect_more's windows, signals, the hit history): a stream with
// nothing of a pending submit's kernels queued
inline hipStream_t topup_stream_of(const scn_plan *p, const Slot &s) { return s.own_stream ? s.stream : p->h2d_stream.get(); }
// the first `count` records of the slot's list are in pinned host memory (count 0: its scan and compaction are complete)
int fetch_list(scn_plan *p, Slot &s, uint32_t count);
ScnCompactArgs compact_args(const scn_plan *p, const Slot &s, uint32_t first, uint32_t cap, void *out);
int build_list(scn_plan *p, Slot &s, bool prefetch);
// (for scn_gather.hip) the collected slot's ordered list where the compaction kernel left it, in device memory.
// list_ready == nullptr: the call returns when the list is complete (the host waits for the list kernels).  Otherwise *list_ready
// receives the event that marks its completion (nullptr when there is nothing to wait for) and the caller orders its own stream
// behind it (hipStreamWaitEvent): nothing waits on the host -- what scn_gather_post needs to stay out of the sweep loop's way.
int scn_plan_device_hits(scn_plan *p, int slot, const scn_hit **d_list, uint32_t *n, int *device_id, void **list_ready = nullptr);

// the plan detects behind the transform (floor and baseline plans): the transform reports the spectrum only, into a plan-owned buffer
// when the caller keeps none, and the detect kernel that follows it on the slot's stream is the submit's last kernel
inline bool detects_behind(const scn_plan *p) { return p->floor || p->baseline; }

// the stream the slot's ordered list is built and fetched on
inline hipStream_t list_stream_of(const scn_plan *p, const Slot &s) { return s.own_stream ? s.stream : p->list_stream.get(); }

// scn_trace_plan.hip: what the sweep trace and the level histogram (scn_levels_plan.hip) share, stated there once -- the plans that
// can have either; the refusals of a fold of `slot`, in scn_plan_update_trace's order (`owns`: the plan has what the fold writes,
// `none`: the message where it has not; *folds: the submit has a unit to fold); and what a fold kernel reads of the slot's last
// submit (the spectrum it stored, its centres where it left them, the mask), under the names ScnTraceArgs gives them
int check_trace_plan(const scn_plan *p);
int check_trace_fold(scn_plan *p, int slot, bool owns, const char *none, bool *folds);
template <class A>
void set_fold_source(A &a, const scn_plan *p, const Slot &s) {
  a.power_db = s.spec_power;
  set_centre_source(a, p, s);
  a.n = p->d.n;
  a.n_units = s.life.n_buffers;
  a.sample_rate = p->d.sample_rate;
  a.dc_ignore = p->d.dc_ignore_bins;
  a.i_lo = p->i_lo;
  a.i_hi = p->i_hi;
}
