"""`Plan`: thin object wrapper over one scn_plan handle.

Mirrors what one consumer thread of the reference owns (ProcessSamples + SampleQueue ctor
arguments: process.h:74-85, messageQueue.h:141-146).  Device memory handed to
``submit_device`` is a torch tensor (plumbing only); results come back as numpy arrays.
"""
import ctypes as C

import numpy as np

from . import capi


class Plan:
    def __init__(self, n, sample_rate=8000000, threshold=10.0, kind=capi.KIND_FLOAT_COMPLEX, enob=12,
                 correct_dc=False, max_batch=1, use_bandwidth=0.75, dc_ignore_bins=4, trigger_count=1047,
                 max_hits=0, flags=capi.OUT_SPECTRUM | capi.OUT_HITS, device_id=0,
                 window_type=capi.WIN_BLACKMAN_HARRIS, mode=capi.MODE_FREQUENCY_DOMAIN, average=1,
                 average_layout=capi.AVG_DWELL, detect=capi.DETECT_FIXED, floor_permille=0, floor_window=None, baseline=None):
        """detect = capi.DETECT_BASELINE: a bin is a hit when it exceeds the stored spectrum of its unit's table entry by more than
        `threshold`, then an offset in the plan's dB scale; baseline = a float32 array [rows, n] (or a row count: that many rows of
        +inf) is set_baseline's argument, and a plan without one refuses every submit (scanner_hip.h, "Baseline detector").
        floor_window = (train, guard), floor plans only: each bin's floor is the rank among its own reference cells, the evaluated
        bins guard < |i' - i| <= guard + train away (set_floor_window; scanner_hip.h, "Floor window").
        detect = capi.DETECT_FLOOR: a bin is a hit when it exceeds its own unit's floor -- the value of rank floor_permille
        (0: the median, capi.FLOOR_MIN: the minimum, 1000: the maximum) among the unit's evaluated bins -- by more than
        `threshold`, then an offset in the plan's dB scale; collect_floor returns the floors (scanner_hip.h, "Floor detector").
        average = K > 1: every K buffers of a submit form a group (average_layout: capi.AVG_DWELL, buffers gK ... gK+K-1,
        or capi.AVG_SWEEPS, buffers g, g+G, ...) whose mean power spectrum is what the plan reports and detects on; the
        outputs of collect are then per group (scanner_hip.h)."""
        self._L = capi.lib()
        d = capi.PlanDesc()
        d.struct_size = C.sizeof(capi.PlanDesc)
        d.n = n
        d.sample_rate = int(sample_rate)
        d.sample_kind = kind
        d.enob = enob
        d.correct_dc = int(bool(correct_dc))
        d.window_type = window_type
        d.mode = mode
        d.threshold = threshold
        d.dc_ignore_bins = capi.DC_IGNORE_NONE if dc_ignore_bins == 0 else dc_ignore_bins
        d.use_bandwidth = use_bandwidth
        d.trigger_count = trigger_count
        d.max_batch = max_batch
        d.max_hits = max_hits
        d.flags = flags
        d.device_id = device_id
        d.average = average
        d.average_layout = average_layout
        d.detect = detect
        d.floor_permille = floor_permille
        self.average, self.average_layout = max(1, int(average)), average_layout
        self.n, self.kind, self.max_batch, self.flags, self.device_id = n, kind, max_batch, flags, device_id
        self.sample_rate = int(sample_rate)
        self.use_bandwidth = use_bandwidth
        self.buffer_bytes = capi.BYTES_PER_SAMPLE[kind] * n
        self._h = C.c_void_p()
        capi.check(self._L.scn_plan_create(C.byref(d), C.byref(self._h)), "scn_plan_create")
        self._nb = [0] * capi.NUM_SLOTS
        self._keep = [None] * capi.NUM_SLOTS
        self._submit_device, self._collect, self._n_hits = self._L.scn_submit_device, self._L.scn_collect, C.c_uint32()
        self._submit_device_indexed = self._L.scn_submit_device_indexed
        self._baseline_rows = 0
        self._history_rows = 0
        self._trace_cells = 0
        self._levels_shape = (0, 0)
        try:
            if floor_window is not None:
                self.set_floor_window(*floor_window)
            if baseline is not None:
                self.set_baseline(baseline)
        except Exception:
            self.close()
            raise

    # -- lifetime -----------------------------------------------------------
    @property
    def handle(self):
        """the scn_plan* (for C-ABI calls that take a plan: scn_gather_hits_device)"""
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.scn_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def groups(self, n_buffers):
        """Spectra (and trigger bytes) a submit of n_buffers buffers yields: n_buffers / average."""
        assert n_buffers % self.average == 0, f"n_buffers {n_buffers} is not a multiple of average {self.average}"
        return n_buffers // self.average

    def average_parts(self, n_buffers):
        """Workgroups that share one group's buffers in a submit of n_buffers (scn_plan_average_parts)."""
        parts = C.c_uint32()
        capi.check(self._L.scn_plan_average_parts(self._h, n_buffers, C.byref(parts)), "scn_plan_average_parts")
        return parts.value

    # -- staging ------------------------------------------------------------
    def host_buffer(self, slot):
        """The pinned staging slot as a writable uint8 numpy view (max_batch raw buffers)."""
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        capi.check(self._L.scn_host_buffer(self._h, slot, C.byref(ptr), C.byref(nbytes)), "scn_host_buffer")
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(nbytes.value,))

    @staticmethod
    def _meta(nb, center_freqs, seq_ids):
        fc = np.zeros(nb, np.float64) if center_freqs is None else np.ascontiguousarray(center_freqs, np.float64)
        seq = None if seq_ids is None else np.ascontiguousarray(seq_ids, np.uint64)
        assert fc.size == nb and (seq is None or seq.size == nb)
        return fc, seq

    def set_table(self, center_freqs):
        """scn_plan_set_table: the frequency table the source retunes through (frequencyTable.cpp:31-36), uploaded once; a
        submit with `first_index` then tags buffer b with entry (first_index + b) % len(table) and sends no per-buffer centres."""
        fc = np.ascontiguousarray(center_freqs, np.float64).reshape(-1)
        capi.check(self._L.scn_plan_set_table(self._h, fc.ctypes.data_as(C.c_void_p), fc.size), "scn_plan_set_table")

    def set_floor_window(self, train, guard=0):
        """scn_plan_set_floor_window: from the next submit on every bin is held against the floor of its own neighbourhood --
        `train` evaluated-or-masked bins on either side beyond `guard` bins, the masked ones taking up distance only.  (0, 0)
        returns to the unit-wide floor.  Not while a slot is pending; a windowed slot has no collect_floor."""
        capi.check(self._L.scn_plan_set_floor_window(self._h, int(train), int(guard)), "scn_plan_set_floor_window")

    def set_baseline(self, baseline):
        """scn_plan_set_baseline: the stored spectra a baseline plan's units are held against, float32 [rows, n] in natural bin order;
        unit u of a submit reads row (first_index + u) % rows.  An int makes that many rows of +inf -- armed, nothing can hit: where
        learning with update_baseline starts --, 0 drops the baseline.  Not while a slot is pending."""
        if isinstance(baseline, (int, np.integer)):
            rows, ptr = int(baseline), None
        else:
            arr = np.ascontiguousarray(baseline, np.float32)
            assert arr.ndim == 2 and arr.shape[1] == self.n, f"a baseline is [rows, {self.n}]"
            rows, ptr = arr.shape[0], arr.ctypes.data_as(C.c_void_p)
        capi.check(self._L.scn_plan_set_baseline(self._h, rows, ptr), "scn_plan_set_baseline")
        self._baseline_rows = rows

    def update_baseline(self, slot, op=capi.BASELINE_MAX):
        """scn_plan_update_baseline: fold the spectra of the slot's last collected submit into the rows of its units, on the GPU --
        capi.BASELINE_SET copies them, capi.BASELINE_MAX keeps the larger per bin (max-hold).  No slot may be pending."""
        capi.check(self._L.scn_plan_update_baseline(self._h, slot, int(op)), "scn_plan_update_baseline")

    def baseline(self, first_row=0, rows=None):
        """scn_plan_get_baseline: rows [first_row, first_row + rows) of the baseline (to its end by default), float32 [rows, n]."""
        rows = max(0, self._baseline_rows - int(first_row)) if rows is None else int(rows)
        out = np.empty((rows, self.n), np.float32)
        capi.check(self._L.scn_plan_get_baseline(self._h, int(first_row), rows, out.ctypes.data_as(C.c_void_p)), "scn_plan_get_baseline")
        return out

    def set_history(self, rows):
        """scn_plan_set_history: give the plan a hit history of `rows` rows, all zero (0 drops it) -- one uint32 per table entry and
        fftshift index, bit k the visit k visits ago (scanner_hip.h, "Hit history").  Allowed while slots are pending."""
        capi.check(self._L.scn_plan_set_history(self._h, int(rows)), "scn_plan_set_history")
        self._history_rows = int(rows)

    def update_history(self, slot):
        """scn_plan_update_history: fold the hits of the slot's last collected submit into the rows of its units, on the GPU -- every
        word of those rows shifts left by one and takes the bin's hit bit.  Once per submit; other slots may be pending."""
        capi.check(self._L.scn_plan_update_history(self._h, slot), "scn_plan_update_history")

    def history(self, first_row=0, rows=None):
        """scn_plan_get_history: (history uint32 [rows, n] by fftshift index, visits uint32 [rows]) of rows [first_row, first_row +
        rows) (to the history's end by default)."""
        rows = max(0, self._history_rows - int(first_row)) if rows is None else int(rows)
        hist, visits = np.empty((rows, self.n), np.uint32), np.empty(rows, np.uint32)
        capi.check(self._L.scn_plan_get_history(self._h, int(first_row), rows, hist.ctypes.data_as(C.c_void_p), visits.ctypes.data_as(C.c_void_p)),
                   "scn_plan_get_history")
        return hist, visits

    def collect_confirmed(self, slot, m, window, first=0, cap=None):
        """scn_collect_confirmed: the records of the slot's last collected -- and folded -- submit whose bin was a hit in at least m of
        the last `window` visits of its table entry, this one included: a subsequence of collect's list (HIT_DTYPE), bit for bit.
        cap=None returns records [first, end) (one call for the total, one for the records); with an explicit cap the C-ABI's own
        behaviour shows: ScannerError(E_TRUNCATED) when first + cap falls short of the total."""
        total = C.c_uint32()
        if cap is None:
            st = self._L.scn_collect_confirmed(self._h, slot, int(m), int(window), int(first), None, 0, C.byref(total))
            if st != capi.E_TRUNCATED:
                capi.check(st, "scn_collect_confirmed")
            cap = max(0, total.value - int(first))
        out = np.zeros(cap, capi.HIT_DTYPE)
        if cap:
            capi.check(self._L.scn_collect_confirmed(self._h, slot, int(m), int(window), int(first), out.ctypes.data_as(C.c_void_p), cap,
                                                     C.byref(total)), "scn_collect_confirmed")
        self.last_n_confirmed = total.value
        return out[: max(0, min(cap, total.value - int(first)))]

    def set_trace(self, f0_hz, cell_hz, cells):
        """scn_plan_set_trace: give the plan a sweep trace of `cells` empty cells of cell_hz hertz from f0_hz up (0 cells drops it) --
        per cell the largest and smallest dB value folded into it and their number (scanner_hip.h, "Sweep trace").  Plans with
        OUT_HITS whose submits store a spectrum; allowed while slots are pending."""
        capi.check(self._L.scn_plan_set_trace(self._h, int(f0_hz), int(cell_hz), int(cells)), "scn_plan_set_trace")
        self._trace_cells = int(cells)

    def update_trace(self, slot):
        """scn_plan_update_trace: fold the spectrum of the slot's last collected submit into the trace, on the GPU -- every evaluated
        bin into the cell of the frequency its hit record would carry.  Other slots may be pending; folding a slot twice counts twice."""
        capi.check(self._L.scn_plan_update_trace(self._h, slot), "scn_plan_update_trace")

    def trace(self, first=0, cells=None):
        """scn_plan_get_trace: (max_db float32, min_db float32, count uint64) of cells [first, first + cells) (to the trace's end by
        default); an empty cell reads (-inf, +inf, 0)."""
        cells = max(0, self._trace_cells - int(first)) if cells is None else int(cells)
        max_db, min_db, count = np.empty(cells, np.float32), np.empty(cells, np.float32), np.empty(cells, np.uint64)
        capi.check(self._L.scn_plan_get_trace(self._h, int(first), cells, max_db.ctypes.data_as(C.c_void_p), min_db.ctypes.data_as(C.c_void_p),
                                              count.ctypes.data_as(C.c_void_p)), "scn_plan_get_trace")
        return max_db, min_db, count

    def merge_trace(self, max_db, min_db, count, first=0):
        """scn_plan_merge_trace: the host window (max_db float32, min_db float32, count uint64) joined into cells [first, first +
        len(max_db)) of the plan's trace, on the GPU, as capi.trace_merge joins two host traces -- the counts added, the larger
        maximum and the smaller minimum kept.  How the root of a sharded sweep takes the ranks' traces in before it asks for the
        band's emitters.  A NaN in max_db or min_db is refused; allowed while slots are pending."""
        max_db, min_db, count = (np.ascontiguousarray(a, dt).reshape(-1) for a, dt in zip((max_db, min_db, count), (np.float32, np.float32, np.uint64)))
        assert max_db.size == min_db.size == count.size
        capi.check(self._L.scn_plan_merge_trace(self._h, int(first), max_db.size, max_db.ctypes.data_as(C.c_void_p), min_db.ctypes.data_as(C.c_void_p),
                                                count.ctypes.data_as(C.c_void_p)), "scn_plan_merge_trace")

    def trace_emitters(self, threshold_db, line=capi.TRACE_LINE_MAX, max_gap=0, first_cell=0, cells=None, first=0, cap=None):
        """scn_plan_trace_emitters: the emitters of cells [first_cell, first_cell + cells) of the plan's trace (to its end by default),
        segmented on the GPU (EMITTER_DTYPE array, ordered by first_cell): one record per run of cells whose `line` (capi.TRACE_LINE_*)
        is above threshold_db, runs joined across up to max_gap off cells -- in absolute hertz, whatever units, centres and sweeps the
        cells were folded from.  cap=None returns records [first, end) (one call for the total, one for the records); with an
        explicit cap the C-ABI's own behaviour shows: ScannerError(E_TRUNCATED) when first + cap falls short of the total.
        last_n_emitters holds the total."""
        cells = max(0, self._trace_cells - int(first_cell)) if cells is None else int(cells)
        total = C.c_uint32()
        args = (self._h, int(first_cell), cells, int(line), float(threshold_db), int(max_gap), int(first))
        if cap is None:
            st = self._L.scn_plan_trace_emitters(*args, None, 0, C.byref(total))
            if st != capi.E_TRUNCATED:
                capi.check(st, "scn_plan_trace_emitters")
            cap = max(0, total.value - int(first))
        out = np.zeros(cap, capi.EMITTER_DTYPE)
        st = self._L.scn_plan_trace_emitters(*args, out.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(total))
        self.last_n_emitters = total.value
        capi.check(st, "scn_plan_trace_emitters")
        return out[: max(0, min(cap, total.value - int(first)))]

    def set_levels(self, f0_hz, cell_hz, cells, edges_db):
        """scn_plan_set_levels: give the plan a level histogram of `cells` cells of cell_hz hertz from f0_hz up and the
        len(edges_db) + 1 levels the edges (float32, strictly increasing, no NaN) cut the dB axis into, every counter 0 (0 cells
        drops it) -- scanner_hip.h, "Level histogram".  The plans that can have a trace; allowed while slots are pending."""
        edges = np.ascontiguousarray(edges_db, np.float32).reshape(-1)
        capi.check(self._L.scn_plan_set_levels(self._h, int(f0_hz), int(cell_hz), int(cells), edges.ctypes.data_as(C.c_void_p), edges.size),
                   "scn_plan_set_levels")
        self._levels_shape = (int(cells), edges.size + 1 if cells else 0)

    def update_levels(self, slot):
        """scn_plan_update_levels: fold the spectrum of the slot's last collected submit into the level histogram, on the GPU --
        every evaluated bin that is not a NaN counts once, in the trace's cell and the level of its dB value.  Other slots may be
        pending; folding a slot twice counts twice."""
        capi.check(self._L.scn_plan_update_levels(self._h, slot), "scn_plan_update_levels")

    def levels(self, first=0, cells=None):
        """scn_plan_get_levels: the counters uint64 [cells, n_levels] of cells [first, first + cells) (to the end by default)."""
        have, n_levels = self._levels_shape
        cells = max(0, have - int(first)) if cells is None else int(cells)
        hist = np.empty((cells, n_levels), np.uint64)
        capi.check(self._L.scn_plan_get_levels(self._h, int(first), cells, hist.ctypes.data_as(C.c_void_p)), "scn_plan_get_levels")
        return hist

    def levels_summary(self, permille=500, level=0, first=0, cells=None):
        """scn_plan_levels_summary, reduced on the GPU: (rank_level uint32, above uint64, total uint64) per cell of [first, first +
        cells) -- the smallest level whose cumulative count exceeds floor(permille * (total - 1) / 1000) (500: the median's level;
        0xFFFFFFFF in an empty cell), the counts of the levels >= level (over total: the occupancy above edges_db[level - 1]), and
        all counts."""
        cells = max(0, self._levels_shape[0] - int(first)) if cells is None else int(cells)
        rank, above, total = np.empty(cells, np.uint32), np.empty(cells, np.uint64), np.empty(cells, np.uint64)
        capi.check(self._L.scn_plan_levels_summary(self._h, int(first), cells, int(permille), int(level), rank.ctypes.data_as(C.c_void_p),
                                                   above.ctypes.data_as(C.c_void_p), total.ctypes.data_as(C.c_void_p)), "scn_plan_levels_summary")
        return rank, above, total

    def submit(self, slot, n_buffers, center_freqs=None, seq_ids=None, first_index=None):
        """Process the first n_buffers raw buffers of the pinned slot (async)."""
        if first_index is not None:
            assert center_freqs is None, "a submit names its centres or a run of the plan's table, not both"
            seq = None if seq_ids is None else np.ascontiguousarray(seq_ids, np.uint64)
            capi.check(self._L.scn_submit_indexed(self._h, slot, n_buffers, int(first_index),
                                                  None if seq is None else seq.ctypes.data_as(C.c_void_p)), "scn_submit_indexed")
            self._nb[slot] = n_buffers
            return
        fc, seq = self._meta(n_buffers, center_freqs, seq_ids)
        capi.check(self._L.scn_submit(self._h, slot, n_buffers, fc.ctypes.data_as(C.c_void_p),
                                      None if seq is None else seq.ctypes.data_as(C.c_void_p)), "scn_submit")
        self._nb[slot] = n_buffers

    def submit_device(self, slot, d_raw, n_buffers=None, center_freqs=None, seq_ids=None, d_power_db=None,
                      sync_producer=True, first_index=None):
        """Process raw IQ already in device memory (a torch tensor or an int address).

        The plan runs on its own non-blocking HIP stream.  With sync_producer (default) the
        torch stream that produced `d_raw` is drained first, so a tensor that was just
        written (`.cuda()`, a generator kernel) is complete before the plan reads it; pass
        False when the caller has already ordered the two streams."""
        if hasattr(d_raw, "data_ptr"):
            if sync_producer:
                import torch

                torch.cuda.current_stream(d_raw.device).synchronize()
            nbytes = d_raw.numel() * d_raw.element_size()
            if n_buffers is None:
                n_buffers = nbytes // self.buffer_bytes
            assert d_raw.is_contiguous() and nbytes >= n_buffers * self.buffer_bytes
            ptr = d_raw.data_ptr()
        else:
            ptr = int(d_raw)
        out_ptr = None
        if d_power_db is not None:
            assert d_power_db.is_contiguous() and d_power_db.numel() >= (n_buffers // self.average) * self.n
            out_ptr = C.c_void_p(d_power_db.data_ptr())
        if first_index is not None:  # a run of the plan's frequency table (set_table)
            assert center_freqs is None, "a submit names its centres or a run of the plan's table, not both"
            seq = None if seq_ids is None else np.ascontiguousarray(seq_ids, np.uint64)
            capi.check(self._L.scn_submit_device_indexed(self._h, slot, C.c_void_p(ptr), n_buffers, int(first_index),
                                                         None if seq is None else seq.ctypes.data_as(C.c_void_p), out_ptr),
                       "scn_submit_device_indexed")
        else:
            fc, seq = self._meta(n_buffers, center_freqs, seq_ids)
            capi.check(self._L.scn_submit_device(self._h, slot, C.c_void_p(ptr), n_buffers,
                                                 fc.ctypes.data_as(C.c_void_p),
                                                 None if seq is None else seq.ctypes.data_as(C.c_void_p), out_ptr),
                       "scn_submit_device")
        self._nb[slot] = n_buffers
        self._keep[slot] = (d_raw, d_power_db)  # keep the tensors alive until collected

    # -- the same two calls without the conveniences: for loops whose step is tens of microseconds ---------------
    def submit_prepared(self, slot, raw_ptr, n_buffers, fc_ptr, seq_ptr, out_ptr):
        """scn_submit_device with everything already a C value (device addresses as ints / c_void_p, the header arrays as
        pointers the caller keeps alive): one ctypes call, no array conversion, nothing retained.  A 2048-buffer launch takes
        24 us on the GPU; submit_device + collect cost more than that in Python alone."""
        st = self._submit_device(self._h, slot, raw_ptr, n_buffers, fc_ptr, seq_ptr, out_ptr)
        if st:
            capi.check(st, "scn_submit_device")
        self._nb[slot] = n_buffers

    def submit_prepared_indexed(self, slot, raw_ptr, n_buffers, first_index, seq_ptr, out_ptr):
        """scn_submit_device_indexed the same way: the centres are a run of the plan's table (set_table)."""
        st = self._submit_device_indexed(self._h, slot, raw_ptr, n_buffers, first_index, seq_ptr, out_ptr)
        if st:
            capi.check(st, "scn_submit_device_indexed")
        self._nb[slot] = n_buffers

    def collect_counts(self, slot, trigger_ptr=None):
        """scn_collect for the per-buffer counts / trigger flags only; returns the batch's total number of hits."""
        st = self._collect(self._h, slot, None, None, 0, C.byref(self._n_hits), trigger_ptr)
        if st:
            capi.check(st, "scn_collect")
        self.last_n_hits = self._n_hits.value
        return self.last_n_hits

    def wait(self, slot):
        capi.check(self._L.scn_wait(self._h, slot), "scn_wait")

    def collect(self, slot, want_power=True, want_hits=True, hit_cap=None, hits_out=None):
        """Block on the slot and return (power_db [B,n] | None, hits (HIT_DTYPE) | None, trigger uint8[B] | None), B the
        submit's buffers -- or its groups, n_buffers / average, on an averaged plan.
        The hit list arrives ordered by (buffer, i) and complete from the GPU.  With hit_cap=None every hit is returned
        however many there are (the part beyond the plan's pinned list is fetched with scn_collect_more); with an
        explicit hit_cap the C-ABI's own behaviour shows: ScannerError(E_TRUNCATED) when more hits exist.
        hits_out: a caller-owned HIT_DTYPE array to receive the records (its length is the capacity): a loop that
        collects every step should not pay for a fresh 12 MB allocation and its page faults each time."""
        nb = self._nb[slot] // self.average
        have_hits = bool(self.flags & capi.OUT_HITS)
        power = np.empty((nb, self.n), np.float32) if (want_power and self.flags & capi.OUT_SPECTRUM) else None
        want_hits = want_hits and have_hits
        cap = (nb * 64 + 1024) if hit_cap is None else hit_cap
        if hits_out is not None:
            assert hits_out.dtype == capi.HIT_DTYPE and hits_out.flags.c_contiguous
            cap, hit_cap = len(hits_out), len(hits_out)
        hits = (hits_out if hits_out is not None else np.empty(cap, capi.HIT_DTYPE)) if want_hits else None
        trig = np.zeros(nb, np.uint8) if have_hits else None
        n_hits = C.c_uint32()
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        st = self._L.scn_collect(self._h, slot, vp(power), vp(hits), cap if want_hits else 0, C.byref(n_hits),
                                 vp(trig))
        self._keep[slot] = None
        self.last_n_hits = n_hits.value
        if st == capi.E_TRUNCATED and want_hits and hit_cap is None:
            hits = self.collect_more(slot, 0, n_hits.value)
            st = capi.OK
        capi.check(st, "scn_collect")
        if want_hits:
            hits = hits[: min(n_hits.value, len(hits))]
        return power, hits, trig

    def collect_more(self, slot, first, count):
        """Records [first, first+count) of the ordered hit list of the slot's last collected submit (scn_collect_more)."""
        out = np.empty(count, capi.HIT_DTYPE)
        done = 0
        while done < count:
            got = C.c_uint32()
            capi.check(self._L.scn_collect_more(self._h, slot, first + done, out[done:].ctypes.data_as(C.c_void_p),
                                                count - done, C.byref(got)), "scn_collect_more")
            if not got.value:
                break
            done += got.value
        return out[:done]

    def collect_signals(self, slot, max_gap=0, first=0, cap=None):
        """scn_collect_signals: the hits of the slot's last collected submit merged into signals on the GPU (SIGNAL_DTYPE array,
        ordered by (buffer, first_i); every hit takes part, however many the plan's max_hits keeps).  A run of hits no more
        than max_gap non-hit bins apart is one signal.  cap=None returns records [first, end) (one call for the total, one for
        the records); with an explicit cap the C-ABI's own behaviour shows: ScannerError(E_TRUNCATED) when first + cap falls
        short of the total."""
        total = C.c_uint32()
        if cap is None:
            st = self._L.scn_collect_signals(self._h, slot, int(max_gap), int(first), None, 0, C.byref(total))
            if st != capi.E_TRUNCATED:
                capi.check(st, "scn_collect_signals")
            cap = max(0, total.value - int(first))
        out = np.zeros(cap, capi.SIGNAL_DTYPE)
        if cap:
            capi.check(self._L.scn_collect_signals(self._h, slot, int(max_gap), int(first), out.ctypes.data_as(C.c_void_p), cap,
                                                   C.byref(total)), "scn_collect_signals")
        self.last_n_signals = total.value
        return out[: max(0, min(cap, total.value - int(first)))]

    def collect_floor(self, slot):
        """scn_collect_floor: floor_db float32[B] of the slot's last collected submit, one per buffer (per group on an averaged
        plan).  Floor-detector plans only (detect=capi.DETECT_FLOOR); a slot submitted under a floor window has no per-unit floor and
        raises ScannerError(E_INVALID), as the library does."""
        out = np.empty(self._nb[slot] // self.average, np.float32)
        capi.check(self._L.scn_collect_floor(self._h, slot, out.ctypes.data_as(C.c_void_p)), "scn_collect_floor")
        return out

    def hits_view(self, slot):
        """Zero-copy numpy view of the plan's pinned ordered hit list (valid until the slot's next submit)."""
        ptr, n = C.c_void_p(), C.c_uint32()
        capi.check(self._L.scn_hits_view(self._h, slot, C.byref(ptr), C.byref(n)), "scn_hits_view")
        if not n.value:
            return np.zeros(0, capi.HIT_DTYPE)
        raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n.value * capi.HIT_DTYPE.itemsize,))
        return raw.view(capi.HIT_DTYPE)

    def collect_time_domain(self, slot):
        """Time-domain plans: (max_db float32[B], min_db float32[B], above uint8[B]) -- process.cpp:203-237."""
        nb = self._nb[slot]
        mx, mn, ab = np.empty(nb, np.float32), np.empty(nb, np.float32), np.zeros(nb, np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        capi.check(self._L.scn_collect_time_domain(self._h, slot, vp(mx), vp(mn), vp(ab)), "scn_collect_time_domain")
        self._keep[slot] = None
        return mx, mn, ab

    def convert_raw(self, raw):
        """K1 alone on the GPU: raw buffers (numpy, the plan's wire format) -> complex64 [B, n]."""
        raw = np.ascontiguousarray(raw)
        nb = raw.nbytes // self.buffer_bytes
        out = np.empty((nb, self.n), np.complex64)
        capi.check(self._L.scn_convert_raw(self._h, raw.ctypes.data_as(C.c_void_p), nb, out.ctypes.data_as(C.c_void_p)),
                   "scn_convert_raw")
        return out

    # -- plumbing -----------------------------------------------------------
    @property
    def stream_handle(self):
        s = C.c_void_p()
        capi.check(self._L.scn_plan_stream(self._h, C.byref(s)), "scn_plan_stream")
        return s.value or 0

    def slot_stream_handle(self, slot):
        """The stream slot's kernels run on (differs per slot only with capi.PLAN_OVERLAP_SLOTS)."""
        s = C.c_void_p()
        capi.check(self._L.scn_slot_stream(self._h, slot, C.byref(s)), "scn_slot_stream")
        return s.value or 0

    def window(self):
        w = np.empty(self.n, np.float32)
        capi.check(self._L.scn_plan_window(self._h, w.ctypes.data_as(C.c_void_p), self.n), "scn_plan_window")
        return w


class WelchPlan:
    """Streaming 65 536-pt, 50 %-overlap Welch PSD (BASELINE config C5) -- wrapper over scn_welch."""

    def __init__(self, n=65536, segments_per_psd=16, max_psd=1, device_id=0, window_type=capi.WIN_BLACKMAN_HARRIS,
                 kind=capi.KIND_FLOAT_COMPLEX, enob=0, correct_dc=False):
        self._L = capi.lib()
        d = capi.WelchDesc()
        d.struct_size = C.sizeof(capi.WelchDesc)
        d.n, d.segments_per_psd, d.window_type, d.max_psd, d.device_id = n, segments_per_psd, window_type, max_psd, device_id
        d.sample_kind, d.enob, d.correct_dc = kind, enob, int(bool(correct_dc))
        self.n, self.k, self.max_psd, self.hop, self.kind = n, segments_per_psd, max_psd, n // 2, kind
        self.bytes_per_sample = capi.BYTES_PER_SAMPLE[kind]
        self._h = C.c_void_p()
        capi.check(self._L.scn_welch_create(C.byref(d), C.byref(self._h)), "scn_welch_create")
        self._npsd = [0] * capi.NUM_SLOTS
        self._keep = [None] * capi.NUM_SLOTS

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.scn_welch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def samples(self, n_psd):
        n = C.c_size_t()
        capi.check(self._L.scn_welch_samples(self._h, n_psd, C.byref(n)), "scn_welch_samples")
        return n.value

    def partition(self, n_psd):
        """(parts, column groups, segments per column group) of a submit of n_psd PSDs -- scn_welch_partition."""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        capi.check(self._L.scn_welch_partition(self._h, n_psd, C.byref(a), C.byref(b), C.byref(c)), "scn_welch_partition")
        return a.value, b.value, c.value

    def host_buffer(self, slot):
        """pinned staging view (max_psd PSDs worth of samples): complex64 for float samples, bytes for the integer wire formats"""
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        capi.check(self._L.scn_welch_host_buffer(self._h, slot, C.byref(ptr), C.byref(nbytes)), "scn_welch_host_buffer")
        if self.kind != capi.KIND_FLOAT_COMPLEX:
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(nbytes.value,))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(nbytes.value // 4,)).view(np.complex64)

    def submit(self, slot, n_psd):
        capi.check(self._L.scn_welch_submit(self._h, slot, n_psd), "scn_welch_submit")
        self._npsd[slot] = n_psd

    def submit_device(self, slot, d_samples, n_psd, d_psd_db=None, sync_producer=True):
        if sync_producer:
            import torch

            torch.cuda.current_stream(d_samples.device).synchronize()
        assert d_samples.is_contiguous() and d_samples.numel() * d_samples.element_size() >= self.samples(n_psd) * self.bytes_per_sample
        out = None if d_psd_db is None else C.c_void_p(d_psd_db.data_ptr())
        capi.check(self._L.scn_welch_submit_device(self._h, slot, C.c_void_p(d_samples.data_ptr()), n_psd, out),
                   "scn_welch_submit_device")
        self._npsd[slot] = n_psd
        self._keep[slot] = (d_samples, d_psd_db)

    def collect(self, slot, want_psd=True):
        nb = self._npsd[slot]
        out = np.empty((nb, self.n), np.float32) if want_psd else None
        capi.check(self._L.scn_welch_collect(self._h, slot, None if out is None else out.ctypes.data_as(C.c_void_p)),
                   "scn_welch_collect")
        self._keep[slot] = None
        return out
