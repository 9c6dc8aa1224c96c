"""ModelPlan: the methods of scanner_amd.Plan that tests/sequence_cases.py's scripts use, restated in numpy from the text of
include/scanner_hip.h and the reference modules (tests/floor_ref.py, local_floor_ref.py, baseline_ref.py, signals_ref.py, history_ref.py,
trace_ref.py, levels_ref.py, emitters_ref.py).  What a plan does over its life -- the table, the floor window, the baseline's rows, each
slot's pending and last collected submit, the hit history with its epoch, the sweep trace and the level histogram with their
geometries -- is plain numpy state here, and every refusal carries the header's status.

The spectrum source is pluggable: every output but the spectrum is an equality on the plan's own stored spectrum, so any
deterministic source does.  numpy_source() is the CPU's: numpy's FFT in float64 on the oracle's converted, windowed samples, rounded
to float32, the mean power over the group for K > 1.  tests/sequence_run.py hands a ModelPlan the spectra of a twin plan on the GPU.

The small `_...` hooks exist so that tests/test_sequence_cases_cpu.py can break one rule at a time in a subclass."""
import numpy as np

from scanner_amd import capi
from tests import baseline_ref, emitters_ref, floor_ref, history_ref, levels_ref, local_floor_ref, signals_ref, trace_ref
from tests.sequence_cases import FS, members


def numpy_source(oracle_mod):
    """spectrum_of for the CPU: plan description -> f(raw [nb, ...]) -> float32 [units, n]"""

    def spectrum_of(plan):
        n, k = plan["n"], plan["average"]
        o = oracle_mod.Oracle(n, FS, kind=plan["kind"], enob=plan["enob"], correct_dc=plan["correct_dc"])
        w = o.window().astype(np.float64)

        def spectra(raw):
            nb = raw.shape[0]
            units = nb // k
            out = np.empty((units, n), np.float32)
            with np.errstate(all="ignore"):
                x = np.stack([o.convert(raw[b]) for b in range(nb)]) if nb else np.zeros((0, n), np.complex64)
                X = np.fft.fft(x.astype(np.complex128) * w, axis=1)
                P = (X.real * X.real + X.imag * X.imag).astype(np.float32)  # (the plan's power is a float: 2^68 squared is +inf)
                for g in range(units):
                    m = P[members(g, units, k, plan["layout"])].astype(np.float64)
                    out[g] = (5.0 * np.log10(m.mean(axis=0))).astype(np.float32)
            return out

        return spectra

    return spectrum_of


def refuse(status, why):
    raise capi.ScannerError(status, "model", why)


class _Slot:
    def __init__(self):
        self.pending = None     # the submit in flight: a dict
        self.last = None        # the last collected submit
        self.list_valid = False
        self.base = None        # (spectra, first, units) of the last accepted submit: what update_baseline folds in
        self.host = None
        self.counts = np.zeros(0, np.int64)  # hits per unit of the last accepted submit
        self.folded = 0         # the plan's history epoch when the last collected submit was folded into the history (0: it was not)
        self.units_before = 0   # units of the accepted submit before the last one
        self.spec = None        # float32 [top, n]: the slot's spectrum memory -- a submit of u units writes rows [0, u), the rest stays
        self.centres = None     # float64 [top]: the same for the centres a submit without an index stages


class ModelPlan:
    def __init__(self, plan, spectra):
        self.d = plan
        self.n, self.average, self.layout, self.flags = plan["n"], plan["average"], plan["layout"], plan["flags"]
        self.max_batch = plan["max_batch"]
        self.max_hits = plan["max_hits"] or min(64 * self.max_batch, 1 << 28)  # (the descriptor's zero defaults)
        self.trigger_count = plan["trigger_count"] or 1047
        self.mask = dict(use_bandwidth=plan["use_bandwidth"], dc_ignore_bins=plan["dc_ignore_bins"])
        self.buffer_bytes = capi.BYTES_PER_SAMPLE[plan["kind"]] * self.n
        self.spectra = spectra
        self.table = None
        self.window = (0, 0)
        self.rows = None  # float32 [rows, n]
        self.slot = [_Slot() for _ in range(capi.NUM_SLOTS)]
        self.last_n_hits = self.last_n_signals = self.last_n_confirmed = self.last_n_emitters = 0
        self.can_history = bool(self.flags & capi.OUT_HITS)
        self.can_trace = self.can_history and (bool(self.flags & capi.OUT_SPECTRUM) or plan["detect"] != "fixed")
        self.hist = None   # (words uint32 [rows, n] by fftshift index, visits uint32 [rows])
        self.epoch = 0     # grows with every set_history and every accepted update_history
        self.tr = None     # dict(f0, cell_hz, trace=(max_db, min_db, count))
        self.lv = None     # dict(f0, cell_hz, edges, hist)

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- the hooks ------------------------------------------------------------------------------------------------------------------
    def _any_pending(self):
        return any(s.pending is not None for s in self.slot)

    def _rows_of(self, first, units, rows):
        return baseline_ref.rows_of(first, units, rows)

    def _entry(self, g):
        """the table entry group g of an indexed submit carries, relative to first_index: the GROUP's index"""
        return g

    def _fold_slot(self, slot):
        return slot

    def _fold(self, rows, spectra, first, op):
        return baseline_ref.update(rows, spectra, first, op)

    def _total(self, slot, counts):
        return int(counts.sum())

    def _new_window(self, train, guard):
        return (train, guard)

    # -- the detectors on one submit's spectra ----------------------------------------------------------------------------------------
    def _detect(self, spectra, fc, seq, first):
        d, n = self.d, self.n
        units = spectra.shape[0]
        common = dict(fs=FS, trigger_count=self.trigger_count, **self.mask)
        floors = None
        if not units:
            return np.zeros(0, capi.HIT_DTYPE), np.zeros(0, np.uint8), np.zeros(0, np.float32), np.zeros(0, np.int64)
        if d["detect"] == "baseline":
            hits, trig = [], np.zeros(units, np.uint8)
            row = self._rows_of(first, units, self.rows.shape[0])
            for u in range(units):  # (unit by unit: the hook names each unit's row)
                h, t = baseline_ref.detect(spectra[u:u + 1], self.rows[row[u]:row[u] + 1], 0, d["threshold"], fc[u:u + 1], seq[u:u + 1], FS,
                                           self.trigger_count, **self.mask)
                hits.append(h)
                trig[u] = t[0]
            hits = np.concatenate(hits)
        elif d["detect"] in ("floor", "window") and self.window != (0, 0):
            _, hits, trig = local_floor_ref.detect(spectra, d["threshold"], self.window[0], self.window[1], d["permille"], fc, seq, **common)
        elif d["detect"] in ("floor", "window"):
            floors, hits, trig = floor_ref.detect(spectra, d["threshold"], d["permille"], fc, seq, **common)
        else:  # fixed: the evaluated bins whose reported float is > threshold
            hits, trig = [], np.zeros(units, np.uint8)
            for u in range(units):
                ii, jj = floor_ref.hit_bins(spectra[u], np.float32(d["threshold"]), **self.mask)
                r = np.zeros(ii.size, capi.HIT_DTYPE)
                r["seq_id"], r["i"], r["power_db"] = seq[u], ii, spectra[u][jj]
                r["freq_hz"] = floor_ref._freq_hz(fc[u], ii, n, FS)
                hits.append(r)
                trig[u] = ii.size > self.trigger_count
            hits = np.concatenate(hits)
        counts = np.array([int((hits["seq_id"] == s).sum()) for s in seq], np.int64)  # (every script's seq_ids differ from unit to unit)
        return hits, trig, floors, counts

    # -- submits ----------------------------------------------------------------------------------------------------------------------
    def host_buffer(self, slot):
        s = self.slot[slot]
        if s.host is None:
            s.host = np.zeros(self.max_batch * self.buffer_bytes, np.uint8)
        return s.host

    def submit(self, slot, n_buffers, center_freqs=None, seq_ids=None, first_index=None, typed=None):
        """the pinned slot's first n_buffers buffers; typed: how to view the bytes (the runner's, as to_raw())"""
        self._submit(slot, None, n_buffers, center_freqs, seq_ids, first_index, host=True, typed=typed)

    def submit_device(self, slot, raw, n_buffers, center_freqs=None, seq_ids=None, first_index=None):
        self._submit(slot, raw, n_buffers, center_freqs, seq_ids, first_index, host=False)

    def _submit(self, slot, raw, nb, fc, seq, first_index, host, typed=None):
        s, k = self.slot[slot], self.average
        indexed = first_index is not None
        have_hits = bool(self.flags & capi.OUT_HITS)
        if indexed and have_hits:  # check_indexed
            if nb and self.table is None:
                refuse(capi.E_STATE, "no table")
            if nb and first_index >= self.table.size:
                refuse(capi.E_INVALID, "first_index outside the table")
        if nb > self.max_batch:
            refuse(capi.E_INVALID, "n_buffers > max_batch")
        if nb % k:
            refuse(capi.E_INVALID, "n_buffers is not a multiple of average")
        units = nb // k
        if fc is not None and k > 1:
            fc = np.asarray(fc, np.float64)
            for g in range(units):
                if not np.all(fc[members(g, units, k, self.layout)] == fc[members(g, units, k, self.layout)[0]]):
                    refuse(capi.E_INVALID, "center_freqs differ inside a group")
        if self.d["detect"] == "baseline":
            if self.rows is None:
                refuse(capi.E_STATE, "no baseline")
            if indexed and self.rows.shape[0] not in (1, 0 if self.table is None else self.table.size):
                refuse(capi.E_STATE, "rows neither 1 nor the table's count")
        if s.pending is not None:
            refuse(capi.E_STATE, "slot pending")
        if host and s.host is None:
            refuse(capi.E_STATE, "host_buffer was never called")
        if host:
            raw = typed(s.host[:nb * self.buffer_bytes].copy(), nb)
        first_of = [int(members(g, units, k, self.layout)[0]) for g in range(units)]
        if indexed:
            first = int(first_index)
            fc_units = np.array([self.table[(first + self._entry(g)) % self.table.size] for g in range(units)], np.float64) if have_hits else np.zeros(units)
        else:
            first = 0
            fc_units = np.asarray(fc, np.float64)[first_of] if units else np.zeros(0)
        seq_units = np.asarray(first_of, np.uint64) if seq is None else np.asarray(seq, np.uint64)[first_of]
        spectra = self.spectra(raw[:nb]) if units else np.zeros((0, self.n), np.float32)
        sub = dict(units=units, spectra=spectra, windowed=self.window != (0, 0), first=first, indexed=indexed and units > 0, fc=fc_units, seq=seq_units)
        s.units_before = (s.last or {}).get("units", 0)  # (of the slot's last collected submit: it is free, nothing is pending)
        top = max(1, self.max_batch // k)
        if s.spec is None:
            s.spec, s.centres = np.full((top, self.n), np.nan, np.float32), np.zeros(top)
        s.spec[:units] = spectra
        if not indexed:
            s.centres[:units] = fc_units
        if have_hits:
            sub["hits"], sub["trig"], sub["floors"], counts = self._detect(spectra, fc_units, seq_units, first)
            sub["total"] = self._total(slot, counts)
            s.counts = counts
        if self.d["detect"] == "baseline":
            s.base = (spectra, first, units)
        s.pending, s.list_valid = sub, False

    # -- collects ---------------------------------------------------------------------------------------------------------------------
    def _take(self, slot):
        s = self.slot[slot]
        if s.pending is None:
            refuse(capi.E_STATE, "nothing submitted")
        s.last, s.pending = s.pending, None
        s.list_valid = bool(self.flags & capi.OUT_HITS)
        s.folded = 0  # (a new collected submit: not yet part of the history)
        self.last_n_hits = s.last.get("total", 0)
        return s.last

    def collect(self, slot):
        sub = self._take(slot)
        p = sub["spectra"].copy() if self.flags & capi.OUT_SPECTRUM else None
        if not self.flags & capi.OUT_HITS:
            return p, None, None
        return p, sub["hits"].copy(), sub["trig"].copy()

    def collect_counts(self, slot):
        return self._take(slot).get("total", 0)

    def _listed(self, slot):
        s = self.slot[slot]
        if s.pending is not None or not s.list_valid:
            refuse(capi.E_STATE, "no collected submit whose list is still valid")
        return s.last

    def more_window(self, slot, first, cap):
        """scn_collect_more as the C-ABI has it: (status, the records written)"""
        return capi.OK, self._listed(slot)["hits"][first:first + cap].copy()

    def signals_window(self, slot, max_gap, first, cap):
        """scn_collect_signals as the C-ABI has it: (status, records [first, first + cap), the total)"""
        if not self.flags & capi.OUT_HITS:
            refuse(capi.E_INVALID, "no SCN_OUT_HITS")
        sub = self._listed(slot)
        sig = signals_ref.signals(sub["hits"], self.n, FS, max_gap)
        self.last_n_signals = len(sig)
        return (capi.E_TRUNCATED if first + cap < len(sig) else capi.OK), sig[first:first + cap].copy(), len(sig)

    def collect_floor(self, slot):
        if self.d["detect"] not in ("floor", "window"):
            refuse(capi.E_INVALID, "not a floor plan")
        sub = self._listed(slot)
        if sub["windowed"]:
            refuse(capi.E_INVALID, "submitted under a floor window")
        return sub["floors"].copy()

    def hits_view(self, slot):
        sub = self._listed(slot)
        return sub["hits"][:min(len(sub["hits"]), self.max_hits)].copy()

    # -- state changes ----------------------------------------------------------------------------------------------------------------
    def set_table(self, center_freqs):
        if self._any_pending():
            refuse(capi.E_STATE, "a slot is pending")
        self._set_table(center_freqs)

    def _set_table(self, center_freqs):
        fc = np.array(center_freqs, np.float64).reshape(-1)
        for s in self.slot:
            s.list_valid = False
        self.table = fc if fc.size else None

    def set_floor_window(self, train, guard=0):
        if self.d["detect"] not in ("floor", "window"):
            refuse(capi.E_INVALID, "not a floor plan")
        if self._any_pending():
            refuse(capi.E_STATE, "a slot is pending")
        if (train, guard) != (0, 0) and not local_floor_ref.valid(self.n, train, guard, **self.mask):
            refuse(capi.E_INVALID, "the window's limits, or a bin without a cell")
        self._set_floor_window(train, guard)

    def _set_floor_window(self, train, guard):
        self.window = self._new_window(train, guard)

    def set_baseline(self, baseline):
        if self.d["detect"] != "baseline":
            refuse(capi.E_INVALID, "not a baseline plan")
        if self._any_pending():
            refuse(capi.E_STATE, "a slot is pending")
        self._set_baseline(baseline)

    def _set_baseline(self, baseline):
        if isinstance(baseline, (int, np.integer)):
            self.rows = np.full((int(baseline), self.n), np.inf, np.float32) if baseline else None
        else:
            self.rows = np.array(baseline, np.float32).reshape(-1, self.n)

    def update_baseline(self, slot, op=capi.BASELINE_MAX):
        if self.d["detect"] != "baseline":
            refuse(capi.E_INVALID, "not a baseline plan")
        if self._any_pending():
            refuse(capi.E_STATE, "a slot is pending")
        base = self.slot[self._fold_slot(slot)].base
        if base is None:
            refuse(capi.E_STATE, "no collected submit to learn from")
        if self.rows is None:
            refuse(capi.E_STATE, "no baseline")
        spectra, first, units = base
        if op not in (capi.BASELINE_SET, capi.BASELINE_MAX) or units > self.rows.shape[0]:
            refuse(capi.E_INVALID, "an unknown op, or more units than rows")
        if units:
            self.rows = self._fold(self.rows, spectra, self._rows_of(first, 1, self.rows.shape[0])[0], op)

    def baseline(self, first_row=0, rows=None):
        if self.d["detect"] != "baseline":
            refuse(capi.E_INVALID, "not a baseline plan")
        have = 0 if self.rows is None else self.rows.shape[0]
        rows = max(0, have - first_row) if rows is None else rows
        if first_row + rows > have:
            refuse(capi.E_INVALID, "rows outside the baseline")
        return np.zeros((0, self.n), np.float32) if not rows else self.rows[first_row:first_row + rows].copy()

    # -- the hit history ("Hit history") ------------------------------------------------------------------------------------------------
    def _history_first(self, sub):
        """the `first` of a unit's row (first + u) % rows: the submit's first_index, 0 for a submit that named its own centres"""
        return sub["first"] if sub["indexed"] else 0

    def _already_folded(self, s):
        return s.folded != 0

    def _is_latest(self, s):
        """no other fold and no set_history since the slot's own"""
        return s.folded != 0 and s.folded == self.epoch

    def _fold_list_ok(self, s):
        """a fold needs what a list needs: a collected submit, no submit and no set_table since"""
        return s.pending is None and s.list_valid

    def _need_history_plan(self):
        if not self.can_history:
            refuse(capi.E_INVALID, "no SCN_OUT_HITS")

    def set_history(self, rows):
        self._need_history_plan()
        self.epoch += 1
        self.hist = history_ref.new(int(rows), self.n) if rows else None

    def update_history(self, slot):
        self._need_history_plan()
        s = self.slot[slot]
        if not self._fold_list_ok(s):
            refuse(capi.E_STATE, "no collected submit whose list is still on the device")
        sub = s.last
        if self.hist is None:
            refuse(capi.E_STATE, "no history")
        rows = self.hist[0].shape[0]
        if sub["units"] > rows:
            refuse(capi.E_INVALID, "more units than rows")
        if sub["indexed"] and rows not in (1, self.table.size):
            refuse(capi.E_STATE, "an indexed submit, rows neither 1 nor the table's count")
        if self._already_folded(s):
            refuse(capi.E_STATE, "already folded")
        self.epoch += 1
        s.folded = self.epoch
        if sub["units"]:
            self.hist = history_ref.fold(*self.hist, sub["hits"], sub["units"], self._history_first(sub), sub["seq"])

    def history(self, first_row=0, rows=None):
        self._need_history_plan()
        have = 0 if self.hist is None else self.hist[0].shape[0]
        rows = max(0, have - first_row) if rows is None else rows
        if first_row + rows > have:
            refuse(capi.E_INVALID, "rows outside the history")
        if not rows:
            return np.zeros((0, self.n), np.uint32), np.zeros(0, np.uint32)
        return self.hist[0][first_row:first_row + rows].copy(), self.hist[1][first_row:first_row + rows].copy()

    def confirmed_window(self, slot, m, window, first, cap):
        """scn_collect_confirmed as the C-ABI has it: (status, records [first, first + cap), the total)"""
        self._need_history_plan()
        if not 1 <= m <= window <= 32:
            refuse(capi.E_INVALID, "1 <= m <= window <= 32")
        s = self.slot[slot]
        if not self._fold_list_ok(s):
            refuse(capi.E_STATE, "no collected submit whose list is still on the device")
        if not self._is_latest(s) or self.hist is None:
            refuse(capi.E_STATE, "not the history's latest fold")
        sub = s.last
        conf = history_ref.confirm(self.hist[0], sub["hits"], sub["units"], m, window, self._history_first(sub), sub["seq"]) if sub["units"] else sub["hits"][:0]
        self.last_n_confirmed = len(conf)
        return (capi.E_TRUNCATED if first + cap < len(conf) else capi.OK), conf[first:first + cap].copy(), len(conf)

    def collect_confirmed(self, slot, m, window, first=0, cap=None):
        st, got, total = self.confirmed_window(slot, m, window, first, 1 << 31 if cap is None else cap)
        if st != capi.OK:
            refuse(st, "truncated")
        return got

    # -- the sweep trace and the level histogram ("Sweep trace", "Level histogram") --------------------------------------------------------
    def _source_slot(self, slot):
        """the slot whose spectrum and centres a fold of `slot` reads"""
        return slot

    def _fold_count(self, s):
        """how many units of the slot's spectrum memory a fold takes: those of its last collected submit"""
        return s.last["units"]

    def _fold_entry(self, g):
        """the table entry, relative to first_index, whose centre unit g of an indexed submit is folded at: the GROUP's"""
        return g

    def _resets(self, old, new):
        """every set_trace and every set_levels empties what it sets, whatever was there"""
        return True

    def _levels_grid(self):
        return self.lv["f0"], self.lv["cell_hz"]

    def _need_trace_plan(self):
        if not self.can_trace:
            refuse(capi.E_INVALID, "a plan that cannot have a trace")

    def _fold_source(self, slot, have):
        """the refusals of a fold, then (spectra, centres) of what it folds -- None where the submit had no units"""
        self._need_trace_plan()
        if not self._fold_list_ok(self.slot[slot]):
            refuse(capi.E_STATE, "no collected submit whose list is still on the device")
        if not have:
            refuse(capi.E_STATE, "no trace / no level histogram")
        s = self.slot[self._source_slot(slot)]
        units = self._fold_count(s)
        if not units:
            return None
        sub = s.last
        if sub["indexed"]:
            centres = np.array([self.table[(sub["first"] + self._fold_entry(g)) % self.table.size] for g in range(units)], np.float64)
        else:
            centres = s.centres[:units].copy()
        return s.spec[:units].copy(), centres

    def set_trace(self, f0_hz, cell_hz, cells):
        self._need_trace_plan()
        if cells and (cell_hz == 0 or cells > capi.TRACE_CELLS_MAX):
            refuse(capi.E_INVALID, "the trace's limits")
        new = (int(f0_hz), int(cell_hz), int(cells))
        if not cells:
            self.tr = None
        elif self.tr is None or self._resets((self.tr["f0"], self.tr["cell_hz"], self.tr["trace"][0].size), new):
            self.tr = dict(f0=new[0], cell_hz=new[1], trace=trace_ref.new(new[2]))

    def update_trace(self, slot):
        src = self._fold_source(slot, self.tr is not None)
        if src is not None:
            self.tr["trace"] = trace_ref.fold(self.tr["trace"], self.tr["f0"], self.tr["cell_hz"], src[0], FS, src[1], **self.mask)

    def _trace_window(self, first, cells):
        self._need_trace_plan()
        have = 0 if self.tr is None else self.tr["trace"][0].size
        cells = max(0, have - first) if cells is None else cells
        if first + cells > have:
            refuse(capi.E_INVALID, "cells outside the trace")
        if not cells:
            return trace_ref.new(0)
        return tuple(a[first:first + cells].copy() for a in self.tr["trace"])

    def trace(self, first=0, cells=None):
        return self._trace_window(first, cells)

    def _merge(self, window, first):
        t = self.tr["trace"]
        merged = trace_ref.merge(tuple(a[first:first + window[0].size] for a in t), window)
        out = tuple(a.copy() for a in t)
        for a, m in zip(out, merged):
            a[first:first + window[0].size] = m
        self.tr["trace"] = out

    def merge_trace(self, max_db, min_db, count, first=0):
        self._need_trace_plan()
        window = tuple(np.ascontiguousarray(a, dt).reshape(-1) for a, dt in zip((max_db, min_db, count), (np.float32, np.float32, np.uint64)))
        if self.tr is None:
            refuse(capi.E_STATE, "no trace")
        if first + window[0].size > self.tr["trace"][0].size or np.isnan(window[0]).any() or np.isnan(window[1]).any():
            refuse(capi.E_INVALID, "a range outside the trace, or a NaN in the window")
        if window[0].size:
            self._merge(window, first)

    def emitters_window(self, first_cell, cells, line, threshold_db, max_gap, first, cap):
        """scn_plan_trace_emitters as the C-ABI has it: (status, records [first, first + cap), the total)"""
        self._need_trace_plan()
        if line > capi.TRACE_LINE_SPREAD or np.isnan(np.float32(threshold_db)):
            refuse(capi.E_INVALID, "the line, or a NaN threshold")
        if self.tr is None:
            refuse(capi.E_STATE, "no trace")
        window = self._trace_window(first_cell, cells)
        em = emitters_ref.emitters(window, self.tr["f0"], self.tr["cell_hz"], line, threshold_db, max_gap, first_cell) if window[0].size else np.zeros(0, capi.EMITTER_DTYPE)
        self.last_n_emitters = len(em)
        return (capi.E_TRUNCATED if first + cap < len(em) else capi.OK), em[first:first + cap].copy(), len(em)

    def trace_emitters(self, threshold_db, line=capi.TRACE_LINE_MAX, max_gap=0, first_cell=0, cells=None, first=0, cap=None):
        st, got, total = self.emitters_window(first_cell, cells, line, threshold_db, max_gap, first, 1 << 31 if cap is None else cap)
        if st != capi.OK:
            refuse(st, "truncated")
        return got

    def set_levels(self, f0_hz, cell_hz, cells, edges_db):
        self._need_trace_plan()
        if not cells:
            self.lv = None
            return
        edges = np.ascontiguousarray(edges_db, np.float32).reshape(-1)
        if cell_hz == 0 or cells > capi.TRACE_CELLS_MAX or not levels_ref.edges_valid(edges) or cells * (edges.size + 1) > capi.LEVELS_WORDS_MAX:
            refuse(capi.E_INVALID, "the histogram's limits, or its edges")
        new = (int(f0_hz), int(cell_hz), int(cells), edges.tobytes())
        if self.lv is None or self._resets((self.lv["f0"], self.lv["cell_hz"], self.lv["hist"].shape[0], self.lv["edges"].tobytes()), new):
            self.lv = dict(f0=new[0], cell_hz=new[1], edges=edges.copy(), hist=levels_ref.new(new[2], edges.size))

    def update_levels(self, slot):
        src = self._fold_source(slot, self.lv is not None)
        if src is not None:
            f0, cell_hz = self._levels_grid()
            self.lv["hist"] = levels_ref.fold(self.lv["hist"], f0, cell_hz, self.lv["edges"], src[0], FS, src[1], **self.mask)

    def levels(self, first=0, cells=None):
        self._need_trace_plan()
        have = 0 if self.lv is None else self.lv["hist"].shape[0]
        cells = max(0, have - first) if cells is None else cells
        if first + cells > have:
            refuse(capi.E_INVALID, "cells outside the histogram")
        return np.zeros((0, 0), np.uint64) if self.lv is None else self.lv["hist"][first:first + cells].copy()

    def levels_summary(self, permille=500, level=0, first=0, cells=None):
        hist = self.levels(first, cells)
        if permille > 1000 or level >= (hist.shape[1] if self.lv is not None else 1):
            refuse(capi.E_INVALID, "permille above 1000, or a level the table does not have")
        return levels_ref.summary(hist, permille, level)
