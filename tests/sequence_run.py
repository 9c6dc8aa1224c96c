"""run(script, make_plan, spectrum_of): executes one of tests/sequence_cases.py's plan scripts against whatever make_plan returns --
scanner_amd.Plan on the GPU, a ModelPlan (or a deliberately broken one) on the CPU -- and after every step compares it with a
ModelPlan (tests/sequence_model.py) that it advances itself on the same inputs.  spectrum_of(plan description) gives the model its
spectra: on the GPU those of a twin, a fixed-threshold SCN_OUT_SPECTRUM-only plan with the same transform parameters on the same
input (twin_source), so that the spectrum check is byte identity with the twin and every other check an equality on that spectrum.

Compared: the statuses of refusals, shapes, the spectrum, the full hit list record for record, the trigger bytes, last_n_hits, the
floors (bit for bit, and against the host form), every drawn window of collect_more and collect_signals against slices of the full
lists (nothing written beyond a window), the signals against tests/signals_ref.py and capi.signals_from_hits, baseline read-backs.
NaN positions compare as NaN; nothing else is exempt and nothing has a tolerance.

The hit history's words and visits are compared as integers after every fold and every set, the confirmed pages record for record
against tests/history_ref.py on the model's own hit list; the sweep trace as bits (trace_ref.same) after every fold, merge and set,
accepted or refused; the level histogram's counters and its summary as integers; the emitter pages byte for byte against
tests/emitters_ref.py on the model's trace; nothing written beyond a page.  Beside the model runs a second account of the same state,
kept with the library's host forms alone (scn_history_fold_hits, scn_confirm_hits, scn_trace_fold_spectrum, scn_trace_merge,
scn_trace_emitters, scn_levels_fold_spectrum, scn_levels_summary), and is held to the model at every comparison."""
import ctypes as C
import pprint

import numpy as np

from scanner_amd import capi
from tests import emitters_ref, floor_ref, history_ref, levels_ref, signals_ref, trace_ref
from tests import sequence_cases as cases
from tests import tolerances as tol
from tests.sequence_model import ModelPlan

DETECT = {"fixed": capi.DETECT_FIXED, "floor": capi.DETECT_FLOOR, "window": capi.DETECT_FLOOR, "baseline": capi.DETECT_BASELINE}
COUNTERS = ("scripts", "steps", "refusals", "spectrum_floats", "records", "windows", "window_records", "signals", "floors", "baseline_floats",
            "nan_as_nan", "special_units", "bar_checks", "history_words", "confirmed_records", "trace_cells", "level_counters", "emitter_records",
            "seam_emitters", "caller_buffer_folds", "exempt_records", "tolerances")


def new_stats():
    return dict.fromkeys(COUNTERS, 0)


class SequenceFailure(AssertionError):
    def __init__(self, seed, index, step_index, kind, script, cause):
        self.seed, self.index, self.step_index, self.kind, self.cause = seed, index, step_index, kind, cause
        super().__init__(f"seed {seed} script {index} step {step_index} ({kind}): {type(cause).__name__}: {cause}\n"
                         f"script = {pprint.pformat(script, width=160, sort_dicts=False)}")


def plan_kwargs(d):
    """scanner_amd.Plan's arguments for a plan description"""
    return dict(n=d["n"], sample_rate=cases.FS, threshold=d["threshold"], kind=d["kind"], enob=d["enob"], correct_dc=d["correct_dc"],
                max_batch=d["max_batch"], use_bandwidth=d["use_bandwidth"], dc_ignore_bins=d["dc_ignore_bins"], trigger_count=d["trigger_count"],
                max_hits=d["max_hits"], flags=d["flags"] | (capi.PLAN_OVERLAP_SLOTS if d["overlap"] else 0), average=d["average"],
                average_layout=d["layout"], detect=DETECT[d["detect"]], floor_permille=d["permille"])


def twin_kwargs(d):
    """the twin: the same transform, a fixed threshold nothing reaches, the spectrum only"""
    return dict(n=d["n"], sample_rate=cases.FS, threshold=1e9, kind=d["kind"], enob=d["enob"], correct_dc=d["correct_dc"], max_batch=d["max_batch"],
                flags=capi.OUT_SPECTRUM, average=d["average"], average_layout=d["layout"])


def _to_device(raw):
    import torch

    if raw.size == 0:
        return torch.zeros(8, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1)).cuda()


def twin_source(make=None):
    """spectrum_of for the GPU: one twin plan per script, each input through its slot 0"""

    def spectrum_of(d):
        from scanner_amd import Plan

        plan = (make or Plan)(**twin_kwargs(d))

        def spectra(raw):
            nb = raw.shape[0]
            if nb < d["average"]:
                return np.zeros((0, d["n"]), np.float32)
            plan.submit_device(0, _to_device(raw), nb)
            return plan.collect(0)[0]

        spectra.close = plan.close
        return spectra

    return spectrum_of


def typed(d):
    """how a plan's raw bytes are viewed: f(uint8 [...], nb) -> [nb, ...] in the wire format's type, as cases.scene() returns it"""
    n, kind = d["n"], d["kind"]
    if kind == capi.KIND_FLOAT_COMPLEX:
        return lambda b, nb: b.view(np.complex64).reshape(nb, n)
    if kind == capi.KIND_BYTE_COMPLEX:
        return lambda b, nb: b.view(np.int8).reshape(nb, n, 2)
    if kind == capi.KIND_SHORT:
        return lambda b, nb: b.view(np.int16).reshape(nb, 2, n)
    return lambda b, nb: b.view(np.int16).reshape(nb, n, 2)


def _status(call, *a, **kw):
    try:
        return capi.OK, call(*a, **kw)
    except capi.ScannerError as e:
        _status.last = str(e)
        return e.status, None


_status.last = ""


def _guarded(count, dtype):
    buf = np.zeros(count + 3, dtype)
    buf.view(np.uint8)[:] = 0xA5
    return buf


def _untouched(buf, written):
    return bool(np.all(buf[written:].view(np.uint8) == 0xA5))


def _more(plan, slot, first, cap):
    """scn_collect_more as the C-ABI has it: (status, the records written); on a real plan, into a buffer with a guard behind it"""
    if hasattr(plan, "more_window"):
        return plan.more_window(slot, first, cap)
    buf, got = _guarded(cap, capi.HIT_DTYPE), C.c_uint32()
    st = plan._L.scn_collect_more(plan.handle, slot, first, buf.ctypes.data_as(C.c_void_p), cap, C.byref(got))
    assert got.value <= cap and _untouched(buf, got.value), f"collect_more wrote beyond its window [{first}, {first} + {cap})"
    return st, buf[:got.value].copy()


def _signals(plan, slot, max_gap, first, cap):
    """scn_collect_signals as the C-ABI has it: (status, records [first, first + cap), the total)"""
    if hasattr(plan, "signals_window"):
        return plan.signals_window(slot, max_gap, first, cap)
    buf, total = _guarded(cap, capi.SIGNAL_DTYPE), C.c_uint32()
    st = plan._L.scn_collect_signals(plan.handle, slot, max_gap, first, buf.ctypes.data_as(C.c_void_p), cap, C.byref(total))
    written = max(0, min(cap, total.value - first))
    assert _untouched(buf, written), f"collect_signals wrote beyond its window [{first}, {first} + {cap})"
    return st, buf[:written].copy(), total.value


def _confirmed(plan, slot, m, window, first, cap):
    """scn_collect_confirmed as the C-ABI has it: (status, records [first, first + cap), the total)"""
    if hasattr(plan, "confirmed_window"):
        return plan.confirmed_window(slot, m, window, first, cap)
    buf, total = _guarded(cap, capi.HIT_DTYPE), C.c_uint32()
    st = plan._L.scn_collect_confirmed(plan.handle, slot, m, window, first, buf.ctypes.data_as(C.c_void_p), cap, C.byref(total))
    if st not in (capi.OK, capi.E_TRUNCATED):
        raise capi.ScannerError(st, "scn_collect_confirmed", plan._L.scn_last_error().decode())
    written = max(0, min(cap, total.value - first))
    assert _untouched(buf, written), f"collect_confirmed wrote beyond its window [{first}, {first} + {cap})"
    return st, buf[:written].copy(), total.value


def _emitters(plan, first_cell, cells, line, threshold_db, max_gap, first, cap):
    """scn_plan_trace_emitters as the C-ABI has it: (status, records [first, first + cap), the total)"""
    if hasattr(plan, "emitters_window"):
        return plan.emitters_window(first_cell, cells, line, threshold_db, max_gap, first, cap)
    buf, total = _guarded(cap, capi.EMITTER_DTYPE), C.c_uint32()
    st = plan._L.scn_plan_trace_emitters(plan.handle, first_cell, cells, line, threshold_db, max_gap, first, buf.ctypes.data_as(C.c_void_p), cap, C.byref(total))
    if st not in (capi.OK, capi.E_TRUNCATED):
        raise capi.ScannerError(st, "scn_plan_trace_emitters", plan._L.scn_last_error().decode())
    written = max(0, min(cap, total.value - first))
    assert _untouched(buf, written), f"trace_emitters wrote beyond its window [{first}, {first} + {cap})"
    return st, buf[:written].copy(), total.value


class _Run:
    def __init__(self, d, plan, model, source, stats, check_spectrum):
        self.d, self.plan, self.model, self.source, self.stats, self.check_spectrum = d, plan, model, source, stats, check_spectrum
        self.typed = typed(d)
        self.evaluated = tol.evaluated_mask(d["n"], d["use_bandwidth"], d["dc_ignore_bins"])
        self.is_model = isinstance(plan, ModelPlan)
        self.bar_done = False
        self.mask = dict(dc_ignore_bins=d["dc_ignore_bins"], use_bandwidth=d["use_bandwidth"])
        self.caller = {}      # slot: the caller's device buffer its pending / last submit wrote its spectrum into
        self.host_hist = self.host_trace = self.host_levels = None  # the same state, kept with the library's host forms

    # -- comparisons: equalities only -------------------------------------------------------------------------------------------------
    def same_floats(self, got, want, what, counter):
        """bit for bit; a NaN compares as a NaN, whatever its payload"""
        got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
        assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
        differ = got.view(np.uint32) != want.view(np.uint32)
        both_nan = np.isnan(got) & np.isnan(want)
        bad = differ & ~both_nan
        assert not bad.any(), f"{what}: {int(bad.sum())} values differ, the first at {tuple(int(v) for v in np.argwhere(bad)[0])}"
        self.stats[counter] += got.size
        self.stats["nan_as_nan"] += int((differ & both_nan).sum())

    def same_records(self, got, want, what, counter="records"):
        floor_ref.assert_same_records(got, want, what)
        self.stats[counter] += len(want)

    def both(self, expect, name, *a, model_kw=None, plan_kw=None, **kw):
        """the same call on the plan and on the model: their statuses agree with each other and with the step's; -> (ok, got, want)"""
        st_m, want = _status(getattr(self.model, name), *a, **kw, **(model_kw or {}))
        st_p, got = _status(getattr(self.plan, name), *a, **kw, **(plan_kw or {}))
        assert st_m == expect, f"{name}: the model returns status {st_m}, the script expects {expect}"
        assert st_p == expect, f"{name}: status {st_p}, expected {expect} ({_status.last})"
        if expect != capi.OK:
            self.stats["refusals"] += 1
        return expect == capi.OK, got, want

    # -- steps --------------------------------------------------------------------------------------------------------------------------
    def step(self, st):
        getattr(self, "do_" + st["op"])(st)

    def do_submit(self, st):
        d, slot, nb, k = self.d, st["slot"], st["nb"], self.d["average"]
        raw = cases.scene(d, st["seed"], -(-nb // k), st["specials"])[:nb]
        fc, seq = cases.headers(d, st)
        kw = dict(seq_ids=seq)
        if st["indexed"]:
            kw["first_index"] = st["first_index"]
        else:
            kw["center_freqs"] = fc
        if st["pinned"]:
            for p in (self.plan, self.model):
                p.host_buffer(slot)[:raw.nbytes] = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
            st_m, _ = _status(self.model.submit, slot, nb, typed=self.typed, **kw)
            st_p, _ = _status(self.plan.submit, slot, nb, **kw, **(dict(typed=self.typed) if self.is_model else {}))
            if st_p == capi.OK:
                self.caller[slot] = None
        else:
            st_m, _ = _status(self.model.submit_device, slot, raw, nb, **kw)
            out = {}
            if st.get("out") and not self.is_model:  # the spectrum goes into the caller's memory, and stays there for the folds
                import torch

                out = dict(d_power_db=torch.full((st["units"] * d["n"],), float("nan"), dtype=torch.float32, device="cuda"))
            st_p, _ = _status(self.plan.submit_device, slot, raw if self.is_model else _to_device(raw), nb, **kw, **out)
            if st_p == capi.OK:
                self.caller[slot] = out.get("d_power_db")
        assert st_m == st["expect"], f"submit: the model returns status {st_m}, the script expects {st['expect']}"
        assert st_p == st["expect"], f"submit: status {st_p}, expected {st['expect']} ({_status.last})"
        if st["expect"] != capi.OK:
            self.stats["refusals"] += 1
            return
        units = st["units"]
        spectra = self.model.slot[slot].pending["spectra"]
        ordinary = [u for u in range(units) if u not in st["specials"]]
        if hasattr(self.plan, "average_parts") and k > 1 and units:  # both regimes of the averaged kernels are drawn by K alone
            assert (self.plan.average_parts(nb) > 1) == (k > 2), (self.plan.average_parts(nb), k, units)
        if st["specials"]:  # the special units are what they are meant to be, and their neighbours do not know of them
            plain = self.source(cases.scene(d, st["seed"], units, None))
            self.same_floats(spectra[ordinary], plain[ordinary], "the ordinary units beside special ones, against the same submit without them", "spectrum_floats")
            assert spectra[ordinary].tobytes() == plain[ordinary].tobytes()
            for u, (what, _) in st["specials"].items():
                row = spectra[u]
                if what == "zero":
                    assert np.all(np.isneginf(row)), "an all-zero unit is not all -inf"
                elif what == "nan":
                    assert np.all(np.isnan(row)), f"a unit with a NaN sample holds {int((~np.isnan(row)).sum())} values that are not NaN"
                elif what == "overflow":
                    band = row[self.evaluated]
                    assert np.isposinf(band).any() and np.isfinite(band).any(), "an overflow unit needs a +inf and a finite evaluated bin"
                self.stats["special_units"] += 1
        if self.check_spectrum is not None and not self.bar_done and ordinary:
            self.check_spectrum(d, raw, spectra, ordinary)  # once per plan: the spectrum itself, at the existing bar, ordinary units only
            self.bar_done = True
            self.stats["bar_checks"] += 1

    def _collected(self, slot, total_hits):
        sub = self.model.slot[slot].last
        assert self.plan.last_n_hits == total_hits, f"last_n_hits {self.plan.last_n_hits}, expected {total_hits}"
        return sub

    def do_collect(self, st):
        slot = st["slot"]
        theirs = self.caller.get(slot) if st["expect"] == capi.OK else None
        ok, got, want = self.both(st["expect"], "collect", slot, plan_kw=dict(want_power=False) if theirs is not None else None)
        if not ok:
            return
        if theirs is not None:  # the plan holds no spectrum of this submit: it is where the caller asked for it
            got = (theirs.cpu().numpy().reshape(-1, self.d["n"]), got[1], got[2])
        (p, h, t), (wp, wh, wt) = got, want
        assert (p is None) == (wp is None) and (h is None) == (wh is None) and (t is None) == (wt is None), "which outputs a collect returns"
        if wp is not None:
            self.same_floats(p, wp, "the spectrum against the twin's", "spectrum_floats")
        if wh is not None:
            self.same_records(h, wh, "the full hit list")
            assert np.asarray(t).tobytes() == wt.tobytes(), f"trigger {np.asarray(t).tolist()}, expected {wt.tolist()}"
        self._collected(slot, 0 if wh is None else len(wh))
        self.post(st, slot)

    def do_counts(self, st):
        slot = st["slot"]
        ok, got, want = self.both(st["expect"], "collect_counts", slot)
        if ok:
            assert got == want, f"collect_counts {got}, expected {want}"
            self._collected(slot, want)
            self.post(st, slot)

    def post(self, st, slot):
        d, n = self.d, self.d["n"]
        sub = self.model.slot[slot].last
        hits = sub.get("hits")
        for op in st["post"]:
            if op[0] == "more":
                first = int(op[1] * len(hits))
                cap = max(1, int(op[2] * len(hits)))
                st_p, got = _more(self.plan, slot, first, cap)
                assert st_p == capi.OK, f"collect_more: status {st_p}"
                self.same_records(got, hits[first:first + cap], f"collect_more [{first}, {first} + {cap}) of {len(hits)}", "window_records")
                self.stats["windows"] += 1
            elif op[0] == "signals":
                want = signals_ref.signals(hits, n, cases.FS, op[1])
                signals_ref.assert_same(capi.signals_from_hits(hits, n, cases.FS, op[1]), want, "scn_signals_from_hits against the reference")
                first = len(want) + 2 if op[2] > 1.0 else int(op[2] * len(want))
                cap = int(op[3] * len(want)) + 1
                st_p, got, total = _signals(self.plan, slot, op[1], first, cap)
                assert total == len(want), f"collect_signals(max_gap {op[1]}): {total} signals, expected {len(want)}"
                assert st_p == (capi.E_TRUNCATED if first + cap < total else capi.OK), f"collect_signals: status {st_p} for [{first}, {first} + {cap}) of {total}"
                signals_ref.assert_same(np.ascontiguousarray(got), want[first:first + cap], f"collect_signals(max_gap {op[1]}) [{first}, {first} + {cap})")
                self.stats["signals"] += len(want[first:first + cap])
                self.stats["windows"] += 1
            elif op[0] == "floor":
                st_p, got = _status(self.plan.collect_floor, slot)
                st_m, want = _status(self.model.collect_floor, slot)
                assert st_p == st_m, f"collect_floor: status {st_p}, expected {st_m}"
                if st_m == capi.OK:
                    self.same_floats(got, want, "collect_floor", "floors")
                    host = [capi.floor_from_spectrum(sub["spectra"][u], d["dc_ignore_bins"], d["use_bandwidth"], d["permille"]) for u in range(sub["units"])]
                    self.same_floats(np.array(host, np.float32), want, "scn_floor_from_spectrum against the reference", "floors")
            else:
                assert op[0] == "view"
                st_p, got = _status(self.plan.hits_view, slot)
                st_m, want = _status(self.model.hits_view, slot)
                assert st_p == st_m == capi.OK, f"hits_view: status {st_p}, the model's {st_m}"
                self.same_records(got, want, "hits_view", "window_records")

    def do_set_table(self, st):
        self.both(st["expect"], "set_table", cases.table_of(st))

    def do_set_window(self, st):
        self.both(st["expect"], "set_floor_window", st["train"], st["guard"])

    def do_set_baseline(self, st):
        d, rows = self.d, st["rows"]
        if st["seed"] is None:
            value = rows
        else:  # an independent draw of the same kind, through the same transform: a row per unit, a submit's worth at a time
            top = max(1, d["max_batch"] // d["average"])
            value = np.concatenate([self.source(cases.scene(d, st["seed"] + a, min(top, rows - a), None)) for a in range(0, rows, top)])
            assert value.shape == (rows, d["n"])
        self.both(st["expect"], "set_baseline", value)

    def do_update_baseline(self, st):
        self.both(st["expect"], "update_baseline", st["slot"], st["mode"])

    def do_get_baseline(self, st):
        ok, got, want = self.both(st["expect"], "baseline")
        if ok:
            self.same_floats(got, want, "the baseline read back", "baseline_floats")


    # -- the hit history -------------------------------------------------------------------------------------------------------------------
    def same_ints(self, got, want, what, counter):
        got, want = np.asarray(got), np.asarray(want)
        assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}, expected {want.dtype} {want.shape}"
        bad = np.argwhere(got != want)
        assert not len(bad), f"{what}: {len(bad)} values differ, the first at {bad[0].tolist()}: {got[tuple(bad[0])]}, expected {want[tuple(bad[0])]}"
        self.stats[counter] += got.size

    def check_history(self, where):
        """the whole history against the model's, and the model's against the host forms' account"""
        if self.model.hist is None:
            return
        got, want = self.plan.history(), self.model.history()
        self.same_ints(got[0], want[0], f"the history's words after {where}", "history_words")
        self.same_ints(got[1], want[1], f"the history's visits after {where}", "history_words")
        self.same_ints(self.host_hist[0], want[0], f"scn_history_fold_hits' words after {where}", "history_words")
        self.same_ints(self.host_hist[1], want[1], f"scn_history_fold_hits' visits after {where}", "history_words")

    def do_set_history(self, st):
        ok, _, _ = self.both(st["expect"], "set_history", st["rows"])
        if ok:
            self.host_hist = history_ref.new(st["rows"], self.d["n"]) if st["rows"] else None
        self.check_history("set_history")

    def do_update_history(self, st):
        ok, _, _ = self.both(st["expect"], "update_history", st["slot"])
        sub = self.model.slot[st["slot"]].last
        if ok and sub["units"]:
            capi.history_fold_hits(*self.host_hist, sub["hits"], sub["units"], sub["first"] if sub["indexed"] else 0, sub["seq"])
        self.check_history("update_history, accepted" if ok else "update_history, refused")

    def do_get_history(self, st):
        ok, got, want = self.both(st["expect"], "history")
        if ok:
            self.same_ints(got[0], want[0], "get_history: the words", "history_words")
            self.same_ints(got[1], want[1], "get_history: the visits", "history_words")

    def do_confirmed(self, st):
        slot, m, window = st["slot"], st["m"], st["window"]
        if st["expect"] != capi.OK:
            st_m, _ = _status(self.model.confirmed_window, slot, m, window, 0, 1)
            st_p, _ = _status(_confirmed, self.plan, slot, m, window, 0, 1)
            assert st_m == st["expect"], f"collect_confirmed: the model returns status {st_m}, the script expects {st['expect']}"
            assert st_p == st["expect"], f"collect_confirmed: status {st_p}, expected {st['expect']} ({_status.last})"
            self.stats["refusals"] += 1
            return
        sub = self.model.slot[slot].last
        first_of = sub["first"] if sub["indexed"] else 0
        want = history_ref.confirm(self.model.hist[0], sub["hits"], sub["units"], m, window, first_of, sub["seq"]) if sub["units"] else sub["hits"][:0]
        _, full, total_m = self.model.confirmed_window(slot, m, window, 0, len(sub["hits"]) + 1)
        self.same_records(full, want, "the model's confirmed list against the reference", "confirmed_records")
        if sub["units"]:
            self.same_records(capi.confirm_hits(self.host_hist[0], sub["hits"], sub["units"], m, window, first_of, sub["seq"]), want,
                              "scn_confirm_hits against the reference", "confirmed_records")
        if (m, window) == (1, 1):
            assert len(want) == len(sub["hits"]), "m = window = 1 returns the full list"
        first = len(want) + 2 if st["first"] > 1.0 else int(st["first"] * len(want))
        cap = int(st["cap"] * len(want)) + 1
        st_p, got, total = _confirmed(self.plan, slot, m, window, first, cap)
        assert total == len(want) == total_m, f"collect_confirmed({m}, {window}): {total} records, expected {len(want)}"
        assert st_p == (capi.E_TRUNCATED if first + cap < total else capi.OK), f"collect_confirmed: status {st_p} for [{first}, {first} + {cap}) of {total}"
        self.same_records(np.ascontiguousarray(got), want[first:first + cap], f"collect_confirmed({m}, {window}) [{first}, {first} + {cap})", "confirmed_records")
        self.stats["windows"] += 1

    # -- the sweep trace, its emitters, the level histogram ----------------------------------------------------------------------------
    def _folded(self, slot):
        """(spectra, centres) of what an accepted fold of the slot took, as the model's last collected submit has them"""
        sub = self.model.slot[slot].last
        if self.caller.get(slot) is not None and sub["units"]:
            self.stats["caller_buffer_folds"] += 1
        return sub["spectra"], sub["fc"]

    def check_trace(self, where):
        if self.model.tr is None:
            return
        got, want = self.plan.trace(), self.model.trace()
        assert trace_ref.same(got, want), f"the trace after {where}: {trace_ref.describe(got, want)}"
        assert trace_ref.same(self.host_trace, want), f"the host forms' trace after {where}: {trace_ref.describe(self.host_trace, want)}"
        self.stats["trace_cells"] += 2 * want[0].size

    def do_set_trace(self, st):
        ok, _, _ = self.both(st["expect"], "set_trace", st["f0"], st["cell_hz"], st["cells"])
        if ok:
            self.host_trace = capi.trace_init(st["cells"]) if st["cells"] else None
        self.check_trace("set_trace")

    def do_update_trace(self, st):
        ok, _, _ = self.both(st["expect"], "update_trace", st["slot"])
        if ok:
            spectra, centres = self._folded(st["slot"])
            if len(centres):
                capi.trace_fold_spectrum(self.host_trace, self.model.tr["f0"], self.model.tr["cell_hz"], spectra, cases.FS, centres, **self.mask)
        self.check_trace("update_trace, accepted" if ok else "update_trace, refused")

    def do_get_trace(self, st):
        ok, got, want = self.both(st["expect"], "trace", st["first_cell"], st["cells"])
        if ok:
            assert trace_ref.same(got, want), f"get_trace [{st['first_cell']}, + {st['cells']}): {trace_ref.describe(got, want)}"
            self.stats["trace_cells"] += want[0].size

    def do_merge_trace(self, st):
        window = cases.merge_window(st)
        ok, _, _ = self.both(st["expect"], "merge_trace", *window, st["first"])
        if ok:
            part = tuple(a[st["first"]:st["first"] + st["cells"]] for a in self.host_trace)  # (views: merged in place)
            capi.trace_merge(part, window)
        self.check_trace("merge_trace, accepted" if ok else "merge_trace, refused")

    def do_emitters(self, st):
        d, args = self.d, (st["first_cell"], st["cells"], st["line"], cases.emitter_threshold(self.d, st), st["max_gap"])
        if st["expect"] != capi.OK:
            st_m, _ = _status(self.model.emitters_window, *args, 0, 1)
            st_p, _ = _status(_emitters, self.plan, *args, 0, 1)
            assert st_m == st_p == st["expect"], f"trace_emitters: status {st_p}, the model's {st_m}, the script expects {st['expect']} ({_status.last})"
            self.stats["refusals"] += 1
            return
        window = self.model.trace(st["first_cell"], st["cells"])
        tr = self.model.tr
        want = emitters_ref.emitters(window, tr["f0"], tr["cell_hz"], args[2], args[3], args[4], st["first_cell"]) if st["cells"] else np.zeros(0, capi.EMITTER_DTYPE)
        if st["cells"]:
            host = capi.trace_emitters(window, tr["f0"], tr["cell_hz"], args[2], args[3], args[4], st["first_cell"])
            assert emitters_ref.same(host, want), f"scn_trace_emitters against the reference: {emitters_ref.describe(host, want)}"
        first = len(want) + 2 if st["first"] > 1.0 else int(st["first"] * len(want))
        cap = int(st["cap"] * len(want)) + 1
        st_p, got, total = _emitters(self.plan, *args, first, cap)
        assert total == len(want), f"trace_emitters{args}: {total} emitters, expected {len(want)}"
        assert st_p == (capi.E_TRUNCATED if first + cap < total else capi.OK), f"trace_emitters: status {st_p} for [{first}, {first} + {cap}) of {total}"
        page = want[first:first + cap]
        assert emitters_ref.same(np.ascontiguousarray(got), page), f"trace_emitters{args} [{first}, {first} + {cap}): {emitters_ref.describe(got, page)}"
        self.stats["emitter_records"] += len(page)
        self.stats["seam_emitters"] += int(((page["first_cell"] <= 1023) & (page["last_cell"] >= 1024)).sum())
        self.stats["windows"] += 1

    def check_levels(self, where):
        if self.model.lv is None:
            return
        got, want = self.plan.levels(), self.model.levels()
        assert levels_ref.same(got, want), f"the level histogram after {where}: {levels_ref.describe(got, want)}"
        assert levels_ref.same(self.host_levels, want), f"the host forms' histogram after {where}: {levels_ref.describe(self.host_levels, want)}"
        self.stats["level_counters"] += 2 * want.size

    def do_set_levels(self, st):
        edges = cases.edges_of(self.d, st["edges"])
        ok, _, _ = self.both(st["expect"], "set_levels", st["f0"], st["cell_hz"], st["cells"], edges)
        if ok:
            self.host_levels = levels_ref.new(st["cells"], edges.size) if st["cells"] else None
        self.check_levels("set_levels")

    def do_update_levels(self, st):
        ok, _, _ = self.both(st["expect"], "update_levels", st["slot"])
        if ok:
            spectra, centres = self._folded(st["slot"])
            lv = self.model.lv
            if len(centres):
                capi.levels_fold_spectrum(self.host_levels, lv["f0"], lv["cell_hz"], lv["edges"], spectra, cases.FS, centres, **self.mask)
        self.check_levels("update_levels, accepted" if ok else "update_levels, refused")

    def do_get_levels(self, st):
        ok, got, want = self.both(st["expect"], "levels")
        if ok:
            assert levels_ref.same(got, want), f"get_levels: {levels_ref.describe(got, want)}"
            self.stats["level_counters"] += want.size

    def do_levels_summary(self, st):
        ok, got, want = self.both(st["expect"], "levels_summary", st["permille"], st["level"])
        if ok:
            ref, host = levels_ref.summary(self.model.lv["hist"], st["permille"], st["level"]), capi.levels_summary(self.host_levels, st["permille"], st["level"])
            for name, g, w, r, h in zip(("rank_level", "above", "total"), got, want, ref, host):
                self.same_ints(g, r, f"levels_summary({st['permille']}, {st['level']}): {name} against the reference", "level_counters")
                self.same_ints(h, r, f"scn_levels_summary: {name} against the reference", "level_counters")
                self.same_ints(w, r, f"the model's {name}", "level_counters")


def kind_of(st):
    return st["op"] if st["expect"] == capi.OK else "refusal:" + st["op"]


def run(script, make_plan, spectrum_of, seed=None, index=None, stats=None, check_spectrum=None):
    """Runs every step; a failure is a SequenceFailure that names the seed, the script, the step and its kind and prints the script."""
    d = script["plan"]
    stats = new_stats() if stats is None else stats
    source = spectrum_of(d)
    plan = None
    try:
        plan = make_plan(d)
        ctx = _Run(d, plan, ModelPlan(d, source), source, stats, check_spectrum)
        for k, st in enumerate(script["steps"]):
            try:
                ctx.step(st)
            except Exception as e:  # (a broken plan may also fail with an IndexError: as much a finding as a difference)
                raise SequenceFailure(seed, index, k, kind_of(st), script, e) from e
            stats["steps"] += 1
        stats["scripts"] += 1
    finally:
        if plan is not None:
            plan.close()
        getattr(source, "close", lambda: None)()
    return stats
