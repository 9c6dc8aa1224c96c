"""The library against the table of a slot's life cycle (scanner_amd/csrc/scn_slot_life.h), as tests/cpp/test_slot_life.cpp prints it
(tests/golden/slot_life_table.txt, held to the program by tests/test_slot_life_cpp.py): for every entry point and every state, slot 0
of a fresh plan is brought into the state, the entry point is called with otherwise valid arguments, and its status must be the
table's.  Where the entry point moves the slot, the state afterwards is observed through the statuses of scn_wait, scn_collect_more and
scn_collect_confirmed, which must be the table's for that state.

The plans are as small as plans get -- 16 points, max_batch 2, max_hits 64, a threshold every evaluated bin of noise exceeds, a table
of two entries and a history of two rows: a fixed-threshold plan, a floor plan, a baseline plan with one row, and a time-domain plan
for scn_collect_time_domain.  The floor and the baseline plan -- a hits-only fixed plan can have neither -- also get a trace of eight
cells and a level histogram of four, on grids of their own around the two centres."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from scanner_amd import capi

pytestmark = pytest.mark.gpu

N, FS, VP = 16, 8000000, C.c_void_p
STATUS = {"SCN_OK": capi.OK, "SCN_E_STATE": capi.E_STATE, "SCN_E_INVALID": capi.E_INVALID}
STATES = ["never_submitted", "pending", "collected", "collected_empty", "no_list", "folded", "folded_stale"]
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slot_life_table.txt")) as _fh:
    TABLE = {(e, s): STATUS[st] for e, s, st in (line.split() for line in _fh if line.strip())}
FC = np.array([100e6, 106e6])
TABLE_FC = np.array([200e6, 206e6])
TRACE = (97000000, 1000000, 8)   # f0_hz, cell_hz, cells: the first unit's band starts below it, the second's ends above it
LEVELS = (98000000, 2000000, 4)
EDGES = np.array([-10.0, 0.0, 10.0], np.float32)


class Rig:
    """one fresh plan of a kind, with a host buffer, a table and a history where the kind can have them"""

    def __init__(self, kind):
        self.L, self.kind = capi.lib(), kind
        self.td = kind == "time_domain"
        d = capi.PlanDesc(struct_size=C.sizeof(capi.PlanDesc), n=N, sample_rate=FS, sample_kind=capi.KIND_FLOAT_COMPLEX, enob=12,
                          mode=capi.MODE_TIME_DOMAIN if self.td else capi.MODE_FREQUENCY_DOMAIN, threshold=-200.0, max_batch=2, max_hits=64,
                          trigger_count=1, flags=0 if self.td else capi.OUT_HITS,
                          detect={"floor": capi.DETECT_FLOOR, "baseline": capi.DETECT_BASELINE}.get(kind, capi.DETECT_FIXED))
        self.plan = VP()
        capi.check(self.L.scn_plan_create(C.byref(d), C.byref(self.plan)), "scn_plan_create")
        x = np.random.default_rng(5).standard_normal(2 * N * 2).astype(np.float32)
        self.x = x
        self.raw = torch.from_numpy(x).cuda()
        self.host, size = VP(), C.c_size_t()
        self.ok(self.L.scn_host_buffer(self.plan, 0, C.byref(self.host), C.byref(size)))
        C.memmove(self.host, x.ctypes.data, x.nbytes)
        self.hits = np.empty(64, capi.HIT_DTYPE)
        self.n = C.c_uint32()
        if not self.td:
            self.ok(self.L.scn_plan_set_table(self.plan, TABLE_FC.ctypes.data_as(VP), 2))
            self.ok(self.L.scn_plan_set_history(self.plan, 2))
        if kind in ("floor", "baseline"):
            self.ok(self.L.scn_plan_set_trace(self.plan, *TRACE))
            self.ok(self.L.scn_plan_set_levels(self.plan, *LEVELS, EDGES.ctypes.data_as(VP), EDGES.size))
            self.src = (np.full(2, 1.0, np.float32), np.full(2, -1.0, np.float32), np.full(2, 3, np.uint64))  # a window to merge
        if kind == "baseline":
            self.row = np.zeros(N, np.float32)
            self.ok(self.L.scn_plan_set_baseline(self.plan, 1, self.row.ctypes.data_as(VP)))

    def ok(self, status):
        capi.check(status, "setting up")

    def close(self):
        assert self.L.scn_plan_destroy(self.plan) == TABLE[("scn_plan_destroy", "pending")] == capi.OK  # (whatever state the slot is in)

    def submit(self, slot=0, units=2):
        self.ok(self.L.scn_submit_device(self.plan, slot, self.raw.data_ptr(), units, FC.ctypes.data_as(VP), None, None))

    def collect(self, slot=0, units=2):
        if self.td:
            return self.ok(self.L.scn_collect_time_domain(self.plan, slot, None, None, None))
        trig = np.zeros(2, np.uint8)
        self.ok(self.L.scn_collect(self.plan, slot, None, None, 0, C.byref(self.n), trig.ctypes.data_as(VP)))
        assert self.n.value >= 2 * units and trig[:units].all(), "every buffer of the batch has hits"

    def bring(self, state, units=2):
        if state == "never_submitted":
            return
        self.submit(units=0 if state == "collected_empty" else units)
        if state == "pending":
            return
        self.collect(units=0 if state == "collected_empty" else units)
        if state == "no_list" and not self.td:  # (a time-domain plan's collected slot never has a list)
            self.ok(self.L.scn_plan_set_table(self.plan, TABLE_FC.ctypes.data_as(VP), 2))
        if state in ("folded", "folded_stale"):
            self.ok(self.L.scn_plan_update_history(self.plan, 0))
        if state == "folded_stale":  # another slot folded
            self.submit(slot=1)
            self.collect(slot=1)
            self.ok(self.L.scn_plan_update_history(self.plan, 1))

    def observe(self, state, where):
        """the slot is in `state`, by what three calls that move nothing answer"""
        L, p = self.L, self.plan
        assert L.scn_wait(p, 0) == TABLE[("scn_wait", state)], f"{where}: scn_wait does not answer as in {state}"
        if self.td:
            return
        got = L.scn_collect_more(p, 0, 0, self.hits.ctypes.data_as(VP), 64, C.byref(self.n))
        assert got == TABLE[("scn_collect_more", state)], f"{where}: scn_collect_more does not answer as in {state}"
        got = L.scn_collect_confirmed(p, 0, 1, 1, 0, self.hits.ctypes.data_as(VP), 64, C.byref(self.n))
        assert got == TABLE[("scn_collect_confirmed", state)], f"{where}: scn_collect_confirmed does not answer as in {state}"


def _listless(state):
    return state if state in ("never_submitted", "pending") else "no_list"


def _epoch_advanced(state):
    return "folded_stale" if state == "folded" else state


# entry point -> (the kind of plan, the call, the state an accepted call leaves -- None: the one it found)
ENTRY = {
    "scn_plan_average_parts": ("fixed", lambda r: r.L.scn_plan_average_parts(r.plan, 2, C.byref(r.n)), None),
    "scn_buffer_bytes": ("fixed", lambda r: r.L.scn_buffer_bytes(r.plan, C.byref(C.c_size_t())), None),
    "scn_host_buffer": ("fixed", lambda r: r.L.scn_host_buffer(r.plan, 0, C.byref(VP()), None), None),
    "scn_submit": ("fixed", lambda r: r.L.scn_submit(r.plan, 0, 2, FC.ctypes.data_as(VP), None), lambda s: "pending"),
    "scn_submit_device": ("floor", lambda r: r.L.scn_submit_device(r.plan, 0, r.raw.data_ptr(), 2, FC.ctypes.data_as(VP), None, None), lambda s: "pending"),
    "scn_plan_set_table": ("fixed", lambda r: r.L.scn_plan_set_table(r.plan, TABLE_FC.ctypes.data_as(VP), 2), _listless),
    "scn_submit_indexed": ("baseline", lambda r: r.L.scn_submit_indexed(r.plan, 0, 2, 1, None), lambda s: "pending"),
    "scn_submit_device_indexed": ("fixed", lambda r: r.L.scn_submit_device_indexed(r.plan, 0, r.raw.data_ptr(), 2, 1, None, None), lambda s: "pending"),
    "scn_collect": ("fixed", lambda r: r.L.scn_collect(r.plan, 0, None, None, 0, C.byref(r.n), None), lambda s: "collected"),
    "scn_collect_more": ("fixed", lambda r: r.L.scn_collect_more(r.plan, 0, 1, r.hits.ctypes.data_as(VP), 64, C.byref(r.n)), None),
    "scn_hits_view": ("floor", lambda r: r.L.scn_hits_view(r.plan, 0, C.byref(VP()), C.byref(r.n)), None),
    "scn_collect_signals": ("baseline", lambda r: r.L.scn_collect_signals(r.plan, 0, 0, 0, np.empty(64, capi.SIGNAL_DTYPE).ctypes.data_as(VP), 64, C.byref(r.n)), None),
    "scn_collect_floor": ("floor", lambda r: r.L.scn_collect_floor(r.plan, 0, np.empty(2, np.float32).ctypes.data_as(VP)), None),
    "scn_plan_set_floor_window": ("floor", lambda r: r.L.scn_plan_set_floor_window(r.plan, 0, 0), None),
    "scn_plan_set_baseline": ("baseline", lambda r: r.L.scn_plan_set_baseline(r.plan, 1, r.row.ctypes.data_as(VP)), None),
    "scn_plan_update_baseline": ("baseline", lambda r: r.L.scn_plan_update_baseline(r.plan, 0, capi.BASELINE_MAX), None),
    "scn_plan_get_baseline": ("baseline", lambda r: r.L.scn_plan_get_baseline(r.plan, 0, 1, np.empty(N, np.float32).ctypes.data_as(VP)), None),
    "scn_plan_set_history": ("fixed", lambda r: r.L.scn_plan_set_history(r.plan, 2), _epoch_advanced),
    "scn_plan_update_history": ("baseline", lambda r: r.L.scn_plan_update_history(r.plan, 0), lambda s: "folded"),
    "scn_plan_get_history": ("fixed", lambda r: r.L.scn_plan_get_history(r.plan, 0, 2, np.empty(2 * N, np.uint32).ctypes.data_as(VP), None), None),
    "scn_collect_confirmed": ("baseline", lambda r: r.L.scn_collect_confirmed(r.plan, 0, 1, 2, 0, r.hits.ctypes.data_as(VP), 64, C.byref(r.n)), None),
    "scn_plan_set_trace": ("floor", lambda r: r.L.scn_plan_set_trace(r.plan, *TRACE), None),
    "scn_plan_update_trace": ("floor", lambda r: r.L.scn_plan_update_trace(r.plan, 0), None),
    "scn_plan_get_trace": ("baseline", lambda r: r.L.scn_plan_get_trace(r.plan, 1, 7, np.empty(7, np.float32).ctypes.data_as(VP), np.empty(7, np.float32).ctypes.data_as(VP),
                                                                       np.empty(7, np.uint64).ctypes.data_as(VP)), None),
    "scn_plan_merge_trace": ("floor", lambda r: r.L.scn_plan_merge_trace(r.plan, 3, 2, *(a.ctypes.data_as(VP) for a in r.src)), None),
    "scn_plan_trace_emitters": ("baseline", lambda r: r.L.scn_plan_trace_emitters(r.plan, 0, 8, capi.TRACE_LINE_MAX, -200.0, 0, 0, np.empty(8, capi.EMITTER_DTYPE).ctypes.data_as(VP),
                                                                                 8, C.byref(r.n)), None),
    "scn_plan_set_levels": ("baseline", lambda r: r.L.scn_plan_set_levels(r.plan, *LEVELS, EDGES.ctypes.data_as(VP), EDGES.size), None),
    "scn_plan_update_levels": ("baseline", lambda r: r.L.scn_plan_update_levels(r.plan, 0), None),
    "scn_plan_get_levels": ("floor", lambda r: r.L.scn_plan_get_levels(r.plan, 0, 4, np.empty(16, np.uint64).ctypes.data_as(VP)), None),
    "scn_plan_levels_summary": ("floor", lambda r: r.L.scn_plan_levels_summary(r.plan, 1, 3, 500, 2, np.empty(3, np.uint32).ctypes.data_as(VP), np.empty(3, np.uint64).ctypes.data_as(VP),
                                                                              np.empty(3, np.uint64).ctypes.data_as(VP)), None),
    "scn_collect_time_domain": ("time_domain", lambda r: r.L.scn_collect_time_domain(r.plan, 0, None, None, None), lambda s: "no_list"),
    "scn_convert_raw": ("fixed", lambda r: r.L.scn_convert_raw(r.plan, r.x.ctypes.data_as(VP), 2, np.empty(4 * N, np.float32).ctypes.data_as(VP)), None),
    "scn_wait": ("floor", lambda r: r.L.scn_wait(r.plan, 0), None),
    "scn_plan_stream": ("fixed", lambda r: r.L.scn_plan_stream(r.plan, C.byref(VP())), None),
    "scn_slot_stream": ("fixed", lambda r: r.L.scn_slot_stream(r.plan, 0, C.byref(VP())), None),
    "scn_device_spectrum": ("fixed", lambda r: r.L.scn_device_spectrum(r.plan, 0, C.byref(VP())), None),
    "scn_plan_window": ("fixed", lambda r: r.L.scn_plan_window(r.plan, np.empty(N, np.float32).ctypes.data_as(VP), N), None),
}
# Rows that are not called here.  scn_plan_destroy ends every case, in whatever state the slot is.  The two gather calls need a
# communicator; they reach the slot through the one internal call whose precondition is scn_collect_more's, and tests/test_sweep_gpu.py runs them.
NOT_CALLED = {"scn_plan_destroy", "scn_gather_hits_device", "scn_gather_post", "scn_collect/refused"}


def test_every_row_is_accounted_for():
    assert {e for e, _ in TABLE} == set(ENTRY) | NOT_CALLED
    assert all((e, s) in TABLE for e in ENTRY for s in STATES)


def _states_of(kind):
    return ["never_submitted", "pending", "no_list"] if kind == "time_domain" else STATES


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_entry_point_in_every_state(built_lib, entry):
    kind, call, leaves = ENTRY[entry]
    for state in _states_of(kind):
        rig = Rig(kind)
        try:
            # (a baseline of one row learns from a submit of one unit: more would be SCN_E_INVALID in any state)
            rig.bring(state, units=1 if entry == "scn_plan_update_baseline" else 2)
            got = call(rig)
            assert got == TABLE[(entry, state)], f"{entry} in {state}: status {got}, the table says {TABLE[(entry, state)]}: {rig.L.scn_last_error().decode()}"
            if got == capi.OK:
                rig.observe(leaves(state) if leaves else state, f"after {entry} in {state}")
        finally:
            rig.close()


def test_refused_collect_has_consumed_the_submit(built_lib):
    """scn_collect takes the submit before it checks its arguments against the plan's flags: asked for the spectrum of a plan that
    keeps none, it answers SCN_E_INVALID -- and the submit is gone, with no list left (kept as it was found; the table's row
    `scn_collect/refused`).  In every other state the call is refused as scn_collect is, and changes nothing."""
    power = np.empty(2 * N, np.float32)
    for state in STATES:
        rig = Rig("fixed")
        try:
            rig.bring(state)
            got = rig.L.scn_collect(rig.plan, 0, power.ctypes.data_as(VP), None, 0, C.byref(rig.n), None)
            assert TABLE[("scn_collect/refused", state)] == (capi.OK if state == "pending" else capi.E_STATE)
            assert got == (capi.E_INVALID if state == "pending" else capi.E_STATE), f"in {state}: status {got}"
            rig.observe("no_list" if state == "pending" else state, f"after a refused scn_collect in {state}")
        finally:
            rig.close()


def test_the_two_rules_beside_the_states(built_lib):
    """With ANOTHER slot pending, every call that requires no slot pending is refused whatever slot 0 holds; a list of a submit that ran
    under a floor window has no per-unit floor."""
    for entry in sorted(e for e, s in TABLE if s == "other_slot_pending"):
        kind, call, _ = ENTRY[entry]
        for state in ("never_submitted", "collected"):
            rig = Rig(kind)
            try:
                rig.bring(state, units=1 if entry == "scn_plan_update_baseline" else 2)
                rig.submit(slot=1)
                got = call(rig)
                assert got == TABLE[(entry, "other_slot_pending")] == capi.E_STATE, f"{entry} in {state} with slot 1 pending: status {got}"
                rig.observe(state, f"after {entry}, refused")
            finally:
                rig.close()
    rig = Rig("floor")
    try:
        rig.ok(rig.L.scn_plan_set_floor_window(rig.plan, 2, 0))
        rig.bring("collected")
        rig.ok(rig.L.scn_plan_set_floor_window(rig.plan, 0, 0))  # (what counts is the window the submit ran under)
        got = ENTRY["scn_collect_floor"][1](rig)
        assert got == TABLE[("scn_collect_floor", "collected_windowed")] == capi.E_INVALID, f"status {got}"
    finally:
        rig.close()
