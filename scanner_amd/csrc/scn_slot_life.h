// scn_slot_life.h -- what a slot may do next, stated once.  Plain C++ (no HIP header): tests/cpp/test_slot_life.cpp walks every
// reachable state with g++.
//
// A slot is FREE or PENDING.  A submit makes it pending, a collect takes the submit and makes it free.  A free slot that has
// collected a submit of a plan with SCN_OUT_HITS holds that submit's LIST -- regions, counts and offsets still on the device -- until
// its next submit or the plan's next scn_plan_set_table.  A list can be FOLDED into the plan's hit history once; it is the history's
// LATEST fold until anything else is folded or scn_plan_set_history is called (scn_plan::history_epoch counts both).  A baseline
// plan's slot is LEARNABLE from its first accepted submit on, for good.
//
// Every entry point states its precondition with one require_* and changes the state with one on_*: no unit of the layer writes a
// member of SlotLife itself.  slot_life_table() is the same statement as data, for the CPU program and tests/test_slot_life_gpu.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scn_host.h"

struct SlotLife {
  bool pending = false;         // a submit has been queued and not collected
  bool list_valid = false;      // regions, counts and offsets of the last collected submit are still on the device
  bool list_built = false;      // the scan + compaction of the pending / last submit have been enqueued
  bool floor_windowed = false;  // the pending / last submit ran under a floor window: it has no per-unit floor (scn_collect_floor)
  bool base_submitted = false;  // baseline plans: there has been a submit whose spectrum scn_plan_update_baseline can learn from
  uint64_t folded_epoch = 0;    // scn_plan::history_epoch when the last collected submit was folded into the hit history (0: it was not)
  uint32_t n_buffers = 0;       // units of the pending / last submit (groups on an averaged plan)
  uint32_t total_hits = 0;      // of the last collected submit
};

// -- preconditions: SCN_OK, or the status with the error text set ---------------------------------------------------------------
inline int require_free(const SlotLife &life, int slot) {
  return life.pending ? scn_fail(SCN_E_STATE, "slot %d has an uncollected submit", slot) : SCN_OK;
}
inline int require_pending(const SlotLife &life, int slot) {
  return life.pending ? SCN_OK : scn_fail(SCN_E_STATE, "slot %d has nothing submitted", slot);
}
// the slot holds a list.  what: "hit list is still on the device", "hit list is still available", "floor is still available"
inline int require_list(const SlotLife &life, int slot, const char *what) {
  return life.pending || !life.list_valid ? scn_fail(SCN_E_STATE, "slot %d: no collected submit whose %s", slot, what) : SCN_OK;
}
// no slot of the plan is pending (what the call replaces may still be read by a pending submit's kernels).  why: "", or
// ": its records still read the table", ": its detect kernel may still read the baseline"
inline int require_none_pending(const SlotLife *const *lives, int count, const char *why) {
  for (int i = 0; i < count; i++)
    if (lives[i]->pending) return scn_fail(SCN_E_STATE, "slot %d has an uncollected submit%s", i, why);
  return SCN_OK;
}
inline int require_unfolded(const SlotLife &life, int slot) {
  return life.folded_epoch ? scn_fail(SCN_E_STATE, "slot %d: its submit is already part of the history", slot) : SCN_OK;
}
// (stricter than rows that do not overlap would need -- and never wrong: the words a record is held against are those its own
// submit was folded into, with nothing folded since)
inline int require_latest_fold(const SlotLife &life, int slot, uint64_t plan_epoch, uint32_t history_rows) {
  return !life.folded_epoch || life.folded_epoch != plan_epoch || !history_rows
             ? scn_fail(SCN_E_STATE, "slot %d: its submit is not the history's latest fold (scn_plan_update_history)", slot)
             : SCN_OK;
}
inline int require_learnable(const SlotLife &life, int slot) {
  return life.base_submitted ? SCN_OK : scn_fail(SCN_E_STATE, "slot %d has no collected submit to learn from", slot);
}
inline int require_unit_floor(const SlotLife &life, int slot) {
  return life.floor_windowed
             ? scn_fail(SCN_E_INVALID, "slot %d was submitted under a floor window: every bin has a floor of its own (scn_local_floor_from_spectrum), no unit has one", slot)
             : SCN_OK;
}

// -- transitions ----------------------------------------------------------------------------------------------------------------
struct SubmitFacts {
  uint32_t units;       // buffers of the submit, or groups on an averaged plan
  bool hits;            // the plan reports hits (SCN_OUT_HITS)
  bool floor_windowed;  // a floor plan with a floor window set
  bool baseline;        // a baseline plan
  bool time_domain;     // a time-domain plan: the submit has units and nothing else
};
// the submit writes the other generation of the slot's hit outputs: it has hits to write
inline bool submit_flips(const SubmitFacts &f) { return !f.time_domain && f.hits && f.units != 0; }
// A submit is being queued: whatever the slot's last collected submit left is gone.  Returns submit_flips.  The slot is not pending
// yet -- on_submitted makes it so, when everything has been queued: a submit that fails in between leaves the slot free, without a list.
inline bool on_submit(SlotLife &life, const SubmitFacts &f) {
  life.n_buffers = f.units;
  if (f.time_domain) return false;
  if (f.baseline) life.base_submitted = true;
  life.floor_windowed = f.floor_windowed;
  life.list_valid = false;
  life.list_built = false;
  return submit_flips(f);
}
inline void on_submitted(SlotLife &life) { life.pending = true; }
inline void on_list_built(SlotLife &life) { life.list_built = true; }
// The pending submit is taken: the slot is free.  scn_collect does this BEFORE it checks its arguments against the plan's flags, so
// a collect refused there has consumed the submit and left no list.
inline void on_take(SlotLife &life) { life.pending = false; }
// ... and collected: a plan with hits holds its list from here on.  A total no scn_hit index can hold is refused, total_hits as it was.
inline int on_collect(SlotLife &life, bool have_hits, uint64_t total) {
  life.list_valid = have_hits;
  life.folded_epoch = 0;  // (a new collected submit: not yet part of the hit history)
  if (total > 0x7fffffffu) return scn_fail(SCN_E_INVALID, "%llu hits in one submit: split the batch", (unsigned long long)total);
  life.total_hits = (uint32_t)total;
  return SCN_OK;
}
inline void on_collect_time_domain(SlotLife &life) { on_take(life); }
// the plan's frequency table changes: the records of every collected list would name the new one's entries
inline void on_table_change(SlotLife *const *lives, int count) {
  for (int i = 0; i < count; i++) lives[i]->list_valid = false;
}
// the slot's list becomes the history's latest fold; epoch: scn_plan::history_epoch, already advanced
inline void on_fold(SlotLife &life, uint64_t epoch) { life.folded_epoch = epoch; }

// -- the same as data -----------------------------------------------------------------------------------------------------------
// For each entry point of include/scanner_hip.h that takes a plan: the require_* it calls, in order, and its transition.  The entry
// points do not dispatch through this; the CPU program and the GPU test read it.
enum class SlotReq { None, Free, Pending, List, NonePending, Unfolded, LatestFold, Learnable, UnitFloor };
enum class SlotMove {
  None,
  Submit,             // on_submit, then on_submitted once everything is queued
  Collect,            // on_take, the argument checks, on_collect
  Take,               // on_take alone: where those argument checks refuse the call
  CollectTimeDomain,  // on_collect_time_domain
  TableChange,        // on_table_change
  Fold,               // on_fold with the plan's epoch advanced
  EpochAdvance,       // no slot changes; the plan's epoch advances, so no slot is the latest fold any more
};
struct SlotRequirement {
  SlotReq req;
  const char *text;  // require_list's `what`, require_none_pending's `why`
};
struct SlotLifeRow {
  const char *name;
  SlotRequirement require[2];
  SlotMove move;
};
inline const SlotLifeRow *slot_life_table(size_t *count) {
  constexpr SlotRequirement none = {SlotReq::None, ""}, on_device = {SlotReq::List, "hit list is still on the device"};
  constexpr SlotRequirement baseline_read = {SlotReq::NonePending, ": its detect kernel may still read the baseline"};
  static const SlotLifeRow table[] = {
      {"scn_plan_destroy", {none, none}, SlotMove::None},
      {"scn_plan_average_parts", {none, none}, SlotMove::None},
      {"scn_buffer_bytes", {none, none}, SlotMove::None},
      {"scn_host_buffer", {none, none}, SlotMove::None},
      {"scn_submit", {{SlotReq::Free, ""}, none}, SlotMove::Submit},
      {"scn_submit_device", {{SlotReq::Free, ""}, none}, SlotMove::Submit},
      {"scn_plan_set_table", {{SlotReq::NonePending, ": its records still read the table"}, none}, SlotMove::TableChange},
      {"scn_submit_indexed", {{SlotReq::Free, ""}, none}, SlotMove::Submit},
      {"scn_submit_device_indexed", {{SlotReq::Free, ""}, none}, SlotMove::Submit},
      {"scn_collect", {{SlotReq::Pending, ""}, none}, SlotMove::Collect},
      // (hits or trigger asked of a plan without SCN_OUT_HITS, power_db of a submit without a spectrum: SCN_E_INVALID, the submit gone)
      {"scn_collect/refused", {{SlotReq::Pending, ""}, none}, SlotMove::Take},
      {"scn_collect_more", {on_device, none}, SlotMove::None},
      {"scn_hits_view", {{SlotReq::List, "hit list is still available"}, none}, SlotMove::None},
      {"scn_collect_signals", {on_device, none}, SlotMove::None},
      {"scn_collect_floor", {{SlotReq::List, "floor is still available"}, {SlotReq::UnitFloor, ""}}, SlotMove::None},
      {"scn_plan_set_floor_window", {{SlotReq::NonePending, ""}, none}, SlotMove::None},
      {"scn_plan_set_baseline", {baseline_read, none}, SlotMove::None},
      {"scn_plan_update_baseline", {baseline_read, {SlotReq::Learnable, ""}}, SlotMove::None},
      {"scn_plan_get_baseline", {none, none}, SlotMove::None},
      {"scn_plan_set_history", {none, none}, SlotMove::EpochAdvance},
      {"scn_plan_update_history", {on_device, {SlotReq::Unfolded, ""}}, SlotMove::Fold},
      {"scn_plan_get_history", {none, none}, SlotMove::None},
      {"scn_collect_confirmed", {on_device, {SlotReq::LatestFold, ""}}, SlotMove::None},
      // (the trace and the level histogram: a fold reads the spectrum and the centres of the slot's list, and moves no slot)
      {"scn_plan_set_trace", {none, none}, SlotMove::None},
      {"scn_plan_update_trace", {on_device, none}, SlotMove::None},
      {"scn_plan_get_trace", {none, none}, SlotMove::None},
      {"scn_plan_merge_trace", {none, none}, SlotMove::None},
      {"scn_plan_trace_emitters", {none, none}, SlotMove::None},
      {"scn_plan_set_levels", {none, none}, SlotMove::None},
      {"scn_plan_update_levels", {on_device, none}, SlotMove::None},
      {"scn_plan_get_levels", {none, none}, SlotMove::None},
      {"scn_plan_levels_summary", {none, none}, SlotMove::None},
      {"scn_collect_time_domain", {{SlotReq::Pending, ""}, none}, SlotMove::CollectTimeDomain},
      {"scn_convert_raw", {none, none}, SlotMove::None},
      {"scn_wait", {{SlotReq::Pending, ""}, none}, SlotMove::None},
      {"scn_plan_stream", {none, none}, SlotMove::None},
      {"scn_slot_stream", {none, none}, SlotMove::None},
      {"scn_device_spectrum", {none, none}, SlotMove::None},
      {"scn_plan_window", {none, none}, SlotMove::None},
      {"scn_gather_hits_device", {on_device, none}, SlotMove::None},  // (both through scn_plan_device_hits)
      {"scn_gather_post", {on_device, none}, SlotMove::None},
  };
  *count = sizeof(table) / sizeof(table[0]);
  return table;
}
