"""ModelPlan: the methods of scanner_amd.Plan that tests/sequence_cases.py's scripts use, restated in numpy from the text of
include/scanner_hip.h and the reference modules (tests/floor_ref.py, local_floor_ref.py, baseline_ref.py, signals_ref.py).  What a
plan does over its life -- the table, the floor window, the baseline's rows, each slot's pending and last collected submit -- is
plain numpy state here, and every refusal carries the header's status.

The spectrum source is pluggable: every output but the spectrum is an equality on the plan's own stored spectrum, so any
deterministic source does.  numpy_source() is the CPU's: numpy's FFT in float64 on the oracle's converted, windowed samples, rounded
to float32, the mean power over the group for K > 1.  tests/sequence_run.py hands a ModelPlan the spectra of a twin plan on the GPU.

The small `_...` hooks exist so that tests/test_sequence_cases_cpu.py can break one rule at a time in a subclass."""
import numpy as np

from scanner_amd import capi
from tests import baseline_ref, floor_ref, local_floor_ref, signals_ref
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
        self.last_n_hits = self.last_n_signals = 0

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
        sub = dict(units=units, spectra=spectra, windowed=self.window != (0, 0), first=first)
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
